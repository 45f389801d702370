#!/usr/bin/env python3
"""Device time of ONE dense conv of a size above 3 on the tiled kernel next to (a) the same layer run by the grouped kernel with one group
(gconv.hip; YOLO_DENSE_AS_GROUPED at plan time -- sizes up to 7, not the first layer) and (b) the dense 3x3 conv of the same extent,
channels and stride, all alternated in one process.  Each variant is a network of a 1x1 conv from the image to the layer's input
channels, the conv under test, a 1x1 class conv, [avgpool], [softmax]; yolo_time_layers gives the middle layer's time.

    python tools/wide_conv_rate.py [batch=32] [rounds=7] [iters=50] [dtypes=bf16,fp16]
prints one JSON line per (shape, dtype): per variant the median and the spread (min .. max) of the interleaved rounds in microseconds and
the TFLOP/s over the layer's own multiply-adds, the ratio wide / grouped, and the box's calib_tflops."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolo_tensorflow_amd import hip, darknet_io as IO

SHAPES = [          # (name, extent, cin, cout, size, stride, pad)
    ("alexnet_conv1_11x11s4", 227, 3, 96, 11, 4, 0),
    ("alexnet_conv2_5x5", 27, 96, 256, 5, 1, 2),
    ("5x5_128_52", 52, 128, 128, 5, 1, 2),
    ("7x7_64_104", 104, 64, 64, 7, 1, 3),
]


def cfg(extent, cin, cout, size, stride, pad):
    conv = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=%d\npad=0\npadding=%d\nactivation=leaky\n\n"
    return ("[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (extent, extent) + conv % (cin, 1, 1, 0) + conv % (cout, size, stride, pad) +
            "[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")


def engine(text, batch, dtype, as_grouped):
    if as_grouped:
        os.environ["YOLO_DENSE_AS_GROUPED"] = "1"
    try:
        eng = hip.Engine(text, max_batch=batch, dtype=getattr(hip, dtype.upper()), semantics=hip.SEM_DARKNET)
    except hip.YoloError:
        return None
    finally:
        os.environ.pop("YOLO_DENSE_AS_GROUPED", None)
    extent = eng.size
    eng.set_weights(IO.synth_weights(IO.parse_cfg(text), seed=0))
    eng.forward(np.random.default_rng(0).integers(0, 256, (batch, extent, extent, 3), dtype=np.uint8), want_detections=False)
    eng.time_layers(batch, 10)          # warm-up
    return eng


def main():
    a = sys.argv[1:]
    batch, rounds, iters = (int(a[i]) if len(a) > i else d for i, d in enumerate((32, 7, 50)))
    dtypes = (a[3] if len(a) > 3 else "bf16,fp16").split(",")
    for dtype in dtypes:
        calib_tflops, calib_ghz = hip.calibrate(0.4, f16=dtype == "fp16")
        for name, extent, cin, cout, size, stride, pad in SHAPES:
            text = cfg(extent, cin, cout, size, stride, pad)
            engines = {"wide": engine(text, batch, dtype, False)}
            grouped_ok = size <= 7          # GCONV_MAX_SIZE
            if grouped_ok:
                engines["grouped_g1"] = engine(text, batch, dtype, True)
                # the two plans differ in the kernel of layer 1 and in nothing else: tiled against the grouped layer kind ("kernel=-")
                rows = []
                for as_grouped in (False, True):
                    os.environ.pop("YOLO_DENSE_AS_GROUPED", None)
                    if as_grouped:
                        os.environ["YOLO_DENSE_AS_GROUPED"] = "1"
                    rc, table = hip.plan_table(text, dtype=getattr(hip, dtype.upper()), max_batch=batch)
                    os.environ.pop("YOLO_DENSE_AS_GROUPED", None)
                    assert rc == 0, table
                    rows.append(table.splitlines()[1])
                assert rows[0].startswith("1 convolutional kernel=tiled") and rows[1].startswith("1 convolutional kernel=- "), rows
            # the dense 3x3 of the same extent, channels and stride (padding 1): the cost per tap next to it
            engines["dense3x3"] = engine(cfg(extent, cin, cout, 3, stride, 1), batch, dtype, False)
            us = {k: [] for k in engines}
            for _ in range(rounds):
                for k, eng in engines.items():
                    us[k].append(float(eng.time_layers(batch, iters)[1]) * 1e3)
            out = {"shape": name, "extent": extent, "cin": cin, "cout": cout, "size": size, "stride": stride, "pad": pad, "batch": batch, "dtype": dtype,
                   "rounds": rounds, "iters": iters, "calib_tflops": round(calib_tflops, 1), "calib_clock_ghz": round(calib_ghz, 3)}
            for k, eng in engines.items():
                ks, kp = (3, 1) if k == "dense3x3" else (size, pad)
                ho = (extent + 2 * kp - ks) // stride + 1
                flop = 2.0 * batch * ho * ho * cout * cin * ks * ks
                med = float(np.median(us[k]))
                out[k] = {"us": round(med, 2), "us_min": round(min(us[k]), 2), "us_max": round(max(us[k]), 2), "tflops": round(flop / (med * 1e-6) / 1e12, 2)}
                eng.close()
            if grouped_ok:
                out["wide_over_grouped"] = round(out["wide"]["us"] / out["grouped_g1"]["us"], 3)
            else:
                out["grouped_g1"] = "not served: the grouped kernel takes sizes up to 7"
            out["tflops_share_of_3x3"] = round(out["wide"]["tflops"] / out["dense3x3"]["tflops"], 3)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
