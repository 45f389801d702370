#!/usr/bin/env python3
"""What frame averaging costs: YOLOv3-416, bf16, batch 32, the `detect` step replayed from its captured graph, with
yolo_set_frame_average(1) -- today's lean decode -- and (3) -- ring store + mean + full decode -- in the SAME process on the same box, the two
settings interleaved over several rounds.  One JSON line: both step times (median over the rounds, ms), their ratio, the decode layers' own
times from yolo_time_layers, and calib_tflops (the register-resident MFMA yardstick bench.py prints) so lines from different boxes compare.

    python tools/frame_average_rate.py [--batch 32] [--size 416] [--frames 3] [--steps 40] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    from yolo_tensorflow_amd import hip, darknet_io as IO
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)          # a created stream can be captured (bench.py does the same)
    torch.cuda.set_stream(stream)
    txt = IO.cfg_text("yolov3") if args.size == 416 else IO.with_input_size(IO.cfg_text("yolov3"), args.size)
    secs = IO.parse_cfg(txt)
    eng = hip.Engine(txt, max_batch=args.batch, dtype=hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=0, stream=stream.cuda_stream)
    eng.set_weights(IO.synth_weights(secs, seed=0))
    images = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (args.batch, args.size, args.size, 3), dtype=np.uint8)).to(dev)
    max_out = 20
    boxes = torch.zeros(args.batch * max_out * 6, dtype=torch.int32, device=dev); counts = torch.zeros(args.batch, dtype=torch.int32, device=dev)
    heads = [i for i, s in enumerate(secs[1:]) if s["type"] == "yolo"]

    def step_ms(K):
        eng.set_frame_average(K)          # drops the captured step: eager, capture, then replays
        for _ in range(4):
            eng.detect_graph(images, boxes, counts, max_out=max_out)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            eng.detect_graph(images, boxes, counts, max_out=max_out)
        eng.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    times = {1: [], args.frames: []}
    for _ in range(args.rounds):
        for K in times:
            times[K].append(step_ms(K))
    decode = {}
    for K in times:          # the [yolo] layers' launches alone (full decode in both settings: yolo_time_layers never runs the lean form)
        eng.set_frame_average(K)
        ms = eng.time_layers(args.batch, 10)
        decode[K] = [round(float(ms[i]), 4) for i in heads]
    ct, cg = hip.calibrate()
    t1, tk = statistics.median(times[1]), statistics.median(times[args.frames])
    print(json.dumps({"tool": "frame_average_rate", "net": "yolov3-%d" % args.size, "dtype": "bf16", "batch": args.batch, "frames": args.frames,
                      "step_ms_k1": round(t1, 4), "step_ms_k%d" % args.frames: round(tk, 4), "ratio": round(tk / t1, 4),
                      "rounds_ms_k1": [round(v, 4) for v in times[1]], "rounds_ms_k%d" % args.frames: [round(v, 4) for v in times[args.frames]],
                      "decode_layers_ms_full_k1": decode[1], "decode_layers_ms_k%d" % args.frames: decode[args.frames],
                      "ring_mib": round((args.frames + 1) * args.batch * eng.rows * eng.attrs * 4 / 2 ** 20, 1),
                      "calib_tflops": round(ct, 1), "clock_ghz": round(cg, 3)}))
    eng.close()


if __name__ == "__main__":
    main()
