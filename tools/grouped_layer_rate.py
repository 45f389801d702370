#!/usr/bin/env python3
"""Device time of ONE grouped 3x3 conv next to the dense 3x3 conv of the same channels and extent (the tiled kernel), alternated in one
process through two cfgs that differ only in the `groups` key: a 1x1 conv from the image to `channels`, the 3x3 conv under test, a 1x1
class conv, [avgpool], [softmax]; yolo_time_layers gives the middle layer's time.

    python tools/grouped_layer_rate.py [channels=128] [extent=64] [groups=32] [batch=32] [dtype=bf16] [rounds=7] [iters=100]
prints one JSON line: per variant the median and the spread (min .. max) of the rounds in microseconds, the achieved GB/s over the layer's
algorithmic bytes (input + output tensor + filters, each once), the ratio grouped / dense, and the box's calib_tflops."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolo_tensorflow_amd import hip, darknet_io as IO


def cfg(channels, extent, groups):
    conv = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=1\npad=1\n%sactivation=leaky\n\n"
    return ("[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (extent, extent) + conv % (channels, 1, "") + conv % (channels, 3, "groups=%d\n" % groups if groups > 1 else "") +
            "[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")


def main():
    a = sys.argv[1:]
    channels, extent, groups, batch = (int(a[i]) if len(a) > i else d for i, d in enumerate((128, 64, 32, 32)))
    dtype = a[4] if len(a) > 4 else "bf16"
    rounds = int(a[5]) if len(a) > 5 else 7
    iters = int(a[6]) if len(a) > 6 else 100
    engines = {}
    for name, g in (("grouped", groups), ("dense", 1)):
        text = cfg(channels, extent, g)
        eng = hip.Engine(text, max_batch=batch, dtype=getattr(hip, dtype.upper()), semantics=hip.SEM_DARKNET)
        eng.set_weights(IO.synth_weights(IO.parse_cfg(text), seed=0))
        eng.forward(np.random.default_rng(0).integers(0, 256, (batch, extent, extent, 3), dtype=np.uint8), want_detections=False)
        eng.time_layers(batch, 20)          # warm-up
        engines[name] = eng
    us = {"grouped": [], "dense": []}
    for _ in range(rounds):
        for name in ("grouped", "dense"):
            us[name].append(float(engines[name].time_layers(batch, iters)[1]) * 1e3)
    calib_tflops, calib_ghz = hip.calibrate(0.4, f16=dtype == "fp16")
    out = {"channels": channels, "extent": extent, "groups": groups, "batch": batch, "dtype": dtype, "rounds": rounds, "iters": iters,
           "calib_tflops": round(calib_tflops, 1), "calib_clock_ghz": round(calib_ghz, 3)}
    for name, g in (("grouped", groups), ("dense", 1)):
        nbytes = 2.0 * (2 * batch * extent * extent * channels + channels * (channels // g) * 9)
        med = float(np.median(us[name]))
        out[name] = {"us": round(med, 2), "us_min": round(min(us[name]), 2), "us_max": round(max(us[name]), 2), "algorithmic_mb": round(nbytes / 1e6, 2),
                     "gb_per_s": round(nbytes / (med * 1e-6) / 1e9, 1)}
        engines[name].close()
    out["grouped_over_dense"] = round(out["grouped"]["us"] / out["dense"]["us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
