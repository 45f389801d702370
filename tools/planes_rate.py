"""Rate of image networks of another channel count: a YOLOv3-416-shaped cfg at channels=1 and channels=4 ([net] yolo_input=planes) against the
three-channel network, bf16, batch 32, one process.

Every network runs `detect_images` (the STRETCH fit of a ragged batch + the network + threshold + NMS; host-resident packed images in, records out) on
the six tests/golden/images jpgs cycled to 32: as RGB, as their grey plane (the mean of R, G and B), and as four planes (R, G, B, grey).  The three run in
alternating rounds on one created stream; per round the median wall time of a step, then the median over rounds.  With N != 3 the first two convs run as
two launches of the tiled kernel where the RGB network runs the fused first-stage kernel, so a lower rate is expected there; `layers_ms` (yolo_time_layers)
shows where the difference sits.

  python tools/planes_rate.py [--steps 30] [--warmup 5] [--rounds 5] [--out profiles/r18_planes_rate.json]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JPGS = ["dog.jpg", "eagle.jpg", "giraffe.jpg", "horses.jpg", "kite.jpg", "person.jpg"]


def planes_of(rgb, n):
    grey = np.round(rgb.astype(np.float32).mean(axis=2)).astype(np.uint8)
    return {1: grey[:, :, None], 3: rgb, 4: np.concatenate([rgb, grey[:, :, None]], axis=2)}[n].copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from PIL import Image
    from yolo_tensorflow_amd import hip, darknet_io as IO

    B = args.batch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    photos = [np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "images", n)).convert("RGB")) for n in JPGS]
    post = dict(score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)
    nets = {}
    for n in (3, 1, 4):
        txt = IO.cfg_text("yolov3").replace("channels=3", "channels=%d" % n)
        if n != 3:
            txt = IO.with_planes_input(txt)
        eng = hip.Engine(txt, max_batch=B, dtype=hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=0, stream=stream.cuda_stream)
        eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
        packed = hip.pack_images([planes_of(photos[i % len(photos)], n) for i in range(B)], channels=n)
        nets[n] = (eng, packed)

    def timed(n):
        eng, packed = nets[n]
        for _ in range(args.warmup):
            eng.detect_images(packed, fit=hip.FIT_STRETCH, **post)
        ts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            eng.detect_images(packed, fit=hip.FIT_STRETCH, **post)          # (copies its records to the host: synchronises)
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    rounds = {n: [] for n in nets}
    for _ in range(args.rounds):
        for n in nets:
            rounds[n].append(timed(n))
    out = {"workload": "yolov3-416-shaped cfg, bf16, batch %d, detect_images (STRETCH) on the six test jpgs cycled: channels=3 vs yolo_input=planes with channels=1 / 4" % B,
           "steps": args.steps, "rounds": args.rounds, "networks": {}}
    for n, (eng, packed) in nets.items():
        ms = float(np.median(rounds[n]))
        layers = eng.time_layers(B, 10)
        table = hip.plan_table(IO.with_planes_input(IO.cfg_text("yolov3").replace("channels=3", "channels=%d" % n)), dtype=hip.BF16, max_batch=B)[1].splitlines()
        out["networks"]["channels=%d" % n] = {
            "step_ms": ms, "rounds_ms": rounds[n], "img_per_s": B / (ms / 1e3), "packed_source_bytes": int(packed[0].size),
            "first_layers": [" ".join(table[i].split()[1:4]) for i in range(3)], "layers_ms_0_1_2": [float(v) for v in layers[:3]], "network_ms": float(np.sum(layers)),
        }
        eng.close()
    base = out["networks"]["channels=3"]["step_ms"]
    for k, v in out["networks"].items():
        v["step_over_rgb"] = v["step_ms"] / base
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
