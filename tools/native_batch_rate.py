"""Native-size batch rate: what a folder of photos costs against the pre-resized headline, YOLOv3-416, bf16, batch 32, one process.

  (a) the pre-resized step: uint8 [32, 416, 416, 3] on the device, yolo_detect_graph -- bench.py's headline form;
  (b) the native-size step: the six tests/golden/images jpgs at their own sizes, cycled to 32, packed and device-resident,
      yolo_detect_images_graph (STRETCH fit + the same network + threshold + NMS, one graph).
(a) and (b) run in alternating rounds on one created stream, timed with events (median step per round, median over rounds).

  python tools/native_batch_rate.py [--steps 100] [--warmup 10] [--rounds 5] [--kernel-stats STATS_CSV]

--only native: time (b) alone (the process to run under `rocprofv3 --kernel-trace --stats`); --kernel-stats: read that run's
kernel_stats.csv and add the ingest kernel's (k_fit_images) average duration and its bandwidth to the line.  Prints one JSON line.
Bytes of the ingest: the packed source bytes (each counted once, an upper bound of what a downscaling fit reads) plus the network
input written (32 x 416 x 416 x 8 bf16); GB/s against 8 TB/s, the MI355X's HBM peak."""
import argparse
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JPGS = ["dog.jpg", "eagle.jpg", "giraffe.jpg", "horses.jpg", "kite.jpg", "person.jpg"]
HBM_PEAK_GBS = 8000.0


def ingest_stats(path):
    """(calls, average ns) of the fit kernel in a rocprofv3 kernel_stats.csv"""
    with open(path) as fh:
        for row in csv.DictReader(fh):
            if "k_fit_images" in row["Name"]:
                return int(row["Calls"]), float(row["AverageNs"])
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only", choices=["both", "native"], default="both")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()

    import torch
    from PIL import Image
    from yolo_tensorflow_amd import hip, darknet_io as IO

    B, S, max_out = args.batch, 416, 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    txt = IO.cfg_text("yolov3")
    eng = hip.Engine(txt, max_batch=B, dtype=hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=0, stream=stream.cuda_stream)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
    plan_path = os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b%d_bf16.json" % (S, B))
    plan_loaded = False
    if os.path.exists(plan_path):
        plan = json.load(open(plan_path))
        if plan.get("num_cfgs") == hip.op_conv_num_cfgs() and len(plan["cfgs"]) == eng.num_layers:
            eng.set_tile_configs(plan["cfgs"]); plan_loaded = True

    rng = np.random.default_rng(1)
    pre = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)).to(dev)
    photos = [np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "images", n)).convert("RGB")) for n in JPGS]
    buf, descs = hip.pack_images([photos[i % len(photos)] for i in range(B)])
    pix = torch.from_numpy(buf).to(dev)
    boxes_a = torch.zeros(B * max_out * 6, dtype=torch.int32, device=dev); counts_a = torch.zeros(B, dtype=torch.int32, device=dev)
    boxes_b = torch.zeros_like(boxes_a); counts_b = torch.zeros_like(counts_a)
    post = dict(score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)

    def step_a():
        eng.detect_graph(pre, boxes_a, counts_a, **post)

    def step_b():
        eng.detect_images_graph(pix, descs, boxes_b, counts_b, fit=hip.FIT_STRETCH, **post)

    def timed(step):
        for _ in range(args.warmup):
            step()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        torch.cuda.synchronize(dev)
        ev[0].record(stream)
        for i in range(args.steps):
            step()
            ev[i + 1].record(stream)
        torch.cuda.synchronize(dev)
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]))

    ta, tb = [], []
    for _ in range(args.rounds):
        if args.only == "both":
            ta.append(timed(step_a))
        tb.append(timed(step_b))
    src_bytes = int(buf.size)
    dst_bytes = B * S * S * 8 * 2
    out = {
        "workload": "yolov3-416 bf16 batch %d: pre-resized u8 graph step vs native-size graph step (the six test jpgs cycled)" % B,
        "tile_plan": os.path.basename(plan_path) if plan_loaded else "built-in",
        "source_sizes_hw": sorted({(int(d["h"]), int(d["w"])) for d in descs}),
        "pre_resized_step_ms": float(np.median(ta)) if ta else None,
        "native_step_ms": float(np.median(tb)),
        "pre_resized_rounds_ms": ta, "native_rounds_ms": tb,
        "native_over_pre_resized": float(np.median(tb) / np.median(ta)) if ta else None,
        "native_img_per_s": B / (float(np.median(tb)) / 1e3),
        "ingest_bytes": {"source": src_bytes, "input_written": dst_bytes},
    }
    if args.kernel_stats:
        st = ingest_stats(args.kernel_stats)
        if st:
            calls, ns = st
            gbs = (src_bytes + dst_bytes) / ns
            out["ingest_kernel"] = {"calls": calls, "avg_us": ns / 1e3, "gb_per_s": gbs, "frac_of_8tbs": gbs / HBM_PEAK_GBS,
                                    "share_of_native_step": (ns / 1e6) / float(np.median(tb))}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
