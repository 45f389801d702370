#!/usr/bin/env python3
"""Device time of the XNOR layers (xconv.hip, the int8 MFMA) next to the dense bf16 kernels on identical shapes, in one process: the
yolov2-tiny-voc-shaped XNOR-Net detector of tools/make_cfgs.py --xnor (xnor=1 on every conv but the first and the last two) at its own
input size, and the same cfg with the key removed -- the same weight stream, the same images.  Alternated round by round:
yolo_time_layers for every layer of both, yolo_time_forward for the whole forward.

    python tools/xnor_rate.py [batch=32] [dtype=bf16] [rounds=7] [iters=50] [out=profiles/r20_xnor_rate.json]
writes (and prints) one JSON object: per conv layer of the cfg its shape, the median microseconds of the xnor and of the dense network and
their ratio (the yardstick: an xnor layer should not be slower than the dense layer of its shape), both networks' whole-forward img/s, and
the box's calib_tflops."""
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from yolo_tensorflow_amd import hip, darknet_io as IO
import make_cfgs


def main():
    a = sys.argv[1:]
    batch = int(a[0]) if len(a) > 0 else 32
    dtype = a[1] if len(a) > 1 else "bf16"
    rounds = int(a[2]) if len(a) > 2 else 7
    iters = int(a[3]) if len(a) > 3 else 50
    out_path = a[4] if len(a) > 4 else os.path.join(ROOT, "profiles", "r20_xnor_rate.json")
    texts = {"xnor": make_cfgs.xnor_yolov2_tiny_voc(), "dense": make_cfgs.xnor_yolov2_tiny_voc(xnor=False)}
    secs = IO.parse_cfg(texts["xnor"])
    size = int(secs[0]["width"])
    shapes = IO.layer_shapes(secs)
    flat = IO.synth_weights(secs, seed=0)
    img = np.random.default_rng(0).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)
    engines = {}
    for name, text in texts.items():
        eng = hip.Engine(text, max_batch=batch, dtype=getattr(hip, dtype.upper()), semantics=hip.SEM_DARKNET)
        eng.set_weights(flat)
        eng.forward(img, want_detections=False)
        eng.time_layers(batch, 10); eng.time_forward(batch, 10)          # warm-up
        engines[name] = eng
    layer_us = {n: [] for n in engines}; fwd_ms = {n: [] for n in engines}
    for _ in range(rounds):
        for name, eng in engines.items():
            layer_us[name].append(eng.time_layers(batch, iters).astype(np.float64) * 1e3)
            fwd_ms[name].append(float(eng.time_forward(batch, iters)[0]))
    calib_tflops, calib_ghz = hip.calibrate(0.4, f16=dtype == "fp16")
    med = {n: np.median(np.stack(layer_us[n]), axis=0) for n in engines}
    lo = {n: np.min(np.stack(layer_us[n]), axis=0) for n in engines}; hi = {n: np.max(np.stack(layer_us[n]), axis=0) for n in engines}
    out = {"cfg": "yolov2-tiny-voc-xnor", "size": size, "batch": batch, "dtype": dtype, "rounds": rounds, "iters": iters,
           "calib_tflops": round(calib_tflops, 1), "calib_clock_ghz": round(calib_ghz, 3), "layers": []}
    for i, s in enumerate(secs[1:]):
        if s["type"] != "convolutional":
            continue
        k = int(s["size"])
        gflop = 2.0 * k * k * shapes[i][4] * int(s["filters"]) * shapes[i][1] * shapes[i][2] * batch / 1e9
        row = {"layer": i, "kernel": "xconv (i8 MFMA)" if int(s.get("xnor", 0)) else "dense", "size": k, "cin": shapes[i][4], "filters": int(s["filters"]), "extent": [shapes[i][1], shapes[i][2]],
               "gflop": round(gflop, 2)}
        for n in ("xnor", "dense"):
            row[n + "_us"] = round(float(med[n][i]), 2); row[n + "_us_min"] = round(float(lo[n][i]), 2); row[n + "_us_max"] = round(float(hi[n][i]), 2)
            row[n + "_tops"] = round(gflop / 1e3 / (float(med[n][i]) * 1e-6), 1)
        row["xnor_over_dense"] = round(row["xnor_us"] / row["dense_us"], 3)
        out["layers"].append(row)
    for n in ("xnor", "dense"):
        m = float(np.median(fwd_ms[n]))
        out[n + "_forward_ms"] = round(m, 4); out[n + "_img_per_s"] = round(batch / (m * 1e-3), 1)
        engines[n].close()
    out["slower_xnor_layers"] = [r["layer"] for r in out["layers"] if r["kernel"] != "dense" and r["xnor_over_dense"] > 1.0]
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
