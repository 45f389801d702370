#!/usr/bin/env python3
"""Forward rate of a map network (a cfg with `yolo_output=map`, e.g. what `tools/make_cfgs.py --unet DIR` writes): images/s, and for
every [deconvolutional] layer its time (yolo_time_layers) and TFLOP/s next to the 3x3 convs of the same network and to what the chip
sustains on a register-resident MFMA loop in the same run (yolo_calibrate, bench.py's roofline.calib_tflops).

    python tools/segmenter_rate.py CFG [batch=8] [dtype=bf16] [iters=30]
prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolo_tensorflow_amd import hip, darknet_io as IO


def main():
    text = IO.cfg_text(sys.argv[1])
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    dtype = sys.argv[3] if len(sys.argv) > 3 else "bf16"
    iters = int(sys.argv[4]) if len(sys.argv) > 4 else 30
    secs = IO.parse_cfg(text)
    shapes = IO.layer_shapes(secs)
    eng = hip.Engine(text, max_batch=batch, dtype=getattr(hip, dtype.upper()), semantics=hip.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(secs, seed=0))
    eng.time_forward(batch, 5)
    total_ms, conv_ms = eng.time_forward(batch, iters)
    per = eng.time_layers(batch, iters)
    calib_tflops, calib_ghz = hip.calibrate(0.4, f16=dtype == "fp16")
    layers = []
    for i, s in enumerate(secs[1:]):
        if s["type"] not in ("deconvolutional", "convolutional"):
            continue
        k = int(s.get("size", 1))
        _, h, w, cout, cin = shapes[i]
        if s["type"] == "deconvolutional":          # 2 size^2 cin filters per INPUT pixel
            ih, iw = (shapes[i - 1][1], shapes[i - 1][2]) if i > 0 else (int(secs[0]["height"]), int(secs[0]["width"]))
            flops = 2.0 * k * k * cin * cout * ih * iw * batch
        else:
            flops = 2.0 * k * k * cin * cout * h * w * batch
        layers.append({"layer": i, "type": s["type"], "size": k, "stride": int(s.get("stride", 1)), "cin": cin, "cout": cout, "out_hw": [h, w],
                       "ms": round(float(per[i]), 4), "gflop": round(flops / 1e9, 2), "tflops": round(flops / (float(per[i]) * 1e-3) / 1e12, 2) if per[i] > 0 else None})
    print(json.dumps({"cfg": os.path.basename(sys.argv[1]), "batch": batch, "dtype": dtype, "input_hw": list(eng.input_hw), "map_hwc": list(eng.map_geometry()),
                      "ms_per_forward": round(total_ms, 4), "conv_ms_per_forward": round(conv_ms, 4), "images_per_sec": round(batch * 1e3 / total_ms, 1),
                      "calib_tflops": round(calib_tflops, 1), "calib_clock_ghz": round(calib_ghz, 3), "layers": layers}))
    eng.close()


if __name__ == "__main__":
    main()
