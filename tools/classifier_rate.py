#!/usr/bin/env python3
"""Forward rate of a shipped classifier topology (yolo_time_forward): images/s, conv ms per forward, and how many [shortcut] layers run
as a launch of their own (k_shortcut: a `from` tensor of another shape, or an activation; k_add: matched, linear, not folded), next to
what the chip sustains on a register-resident MFMA loop in the same run (calib_tflops).

    python tools/classifier_rate.py [name=resnet50|resnext50|...] [batch=32] [dtype=bf16] [iters=30]
prints one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolo_tensorflow_amd import hip, darknet_io as IO


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
    batch = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    dtype = sys.argv[3] if len(sys.argv) > 3 else "bf16"
    iters = int(sys.argv[4]) if len(sys.argv) > 4 else 30
    text = IO.cfg_text(name)
    secs = IO.parse_cfg(text)
    shapes = IO.layer_shapes(secs)
    general = matched_slope = 0
    for i, s in enumerate(secs[1:]):
        if s["type"] != "shortcut":
            continue
        f = int(s["from"]); f = f if f >= 0 else i + f
        same = shapes[f][1:4] == shapes[i][1:4]
        act = s.get("activation", "linear")
        if not same or act != "linear":
            general += 1
            matched_slope += same and act in ("leaky", "relu", "relie")
    eng = hip.Engine(text, max_batch=batch, dtype=getattr(hip, dtype.upper()), semantics=hip.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(secs, seed=0))
    eng.time_forward(batch, 5)
    total_ms, conv_ms = eng.time_forward(batch, iters)
    calib_tflops, calib_ghz = hip.calibrate(0.4, f16=dtype == "fp16")
    print(json.dumps({"name": name, "batch": batch, "dtype": dtype, "size": eng.size, "ms_per_forward": round(total_ms, 4), "conv_ms_per_forward": round(conv_ms, 4),
                      "images_per_sec": round(batch * 1e3 / total_ms, 1), "conv_tflops": round(eng.conv_flops() * batch / (conv_ms * 1e-3) / 1e12, 1),
                      "calib_tflops": round(calib_tflops, 1), "calib_clock_ghz": round(calib_ghz, 3),
                      "k_shortcut_launches": general, "of_which_a_fold_of_matched_slope_shortcuts_would_absorb": int(matched_slope)}))
    eng.close()


if __name__ == "__main__":
    main()
