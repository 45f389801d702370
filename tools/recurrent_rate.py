#!/usr/bin/env python
"""Rates of the recurrent layers on one GPU (NOTEBOOK, "Recurrent layers"; profiles/r14_recurrent_*.json).

  python tools/recurrent_rate.py --layers OUT.json     # one [lstm] / [gru] output=1024 step over a 1024-wide producer at batch 1 and 32 (yolo_time_layers),
                                                       #   the gate GEMM's weight bytes / time next to calib_copy_gbs of the same run
  python tools/recurrent_rate.py --connected OUT.json  # the yardstick: N = 8 and 6 [connected] output=1024 layers over the same producer, summed -- the matrix
                                                       #   work of that [lstm] / [gru] step as separate layers (uses nothing a commit without recurrent layers lacks)
  python tools/recurrent_rate.py --video DIR OUT.json  # step rate of the cfgs `tools/make_cfgs.py --video DIR` wrote, batch 1 and 32, bf16
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolo_tensorflow_amd import hip, darknet_io as IO  # noqa: E402

HEAD = "[net]\nbatch=1\nwidth=8\nheight=8\nchannels=3\n\n[convolutional]\nbatch_normalize=1\nfilters=16\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"      # 8 x 8 x 16: 1024 values
TAIL = "[connected]\noutput=10\nactivation=linear\n\n[softmax]\n"
ITERS = 200


def layer_ms(cfg, batch, layers, dtype=hip.BF16):
    """mean time of the named layers' launches (ms each), from yolo_time_layers over ITERS passes after a warm-up"""
    eng = hip.Engine(cfg, max_batch=batch, dtype=dtype, semantics=hip.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(cfg), seed=1))
    img = np.random.default_rng(0).integers(0, 256, (batch, 8, 8, 3), dtype=np.uint8)
    eng.forward(img, want_detections=False)
    eng.time_layers(batch, 20)
    ms = eng.time_layers(batch, ITERS)
    eng.close()
    return [float(ms[i]) for i in layers]


def main():
    mode, out = sys.argv[1], sys.argv[-1]
    res = {"mode": mode, "dtype": "bf16", "iters": ITERS}
    if mode == "--connected":
        for n, name in ((8, "lstm"), (6, "gru")):
            cfg = HEAD + "[connected]\noutput=1024\nactivation=linear\n\n" * n + TAIL
            for batch in (1, 32):
                ms = layer_ms(cfg, batch, range(1, 1 + n))
                res["connected_x%d_for_%s_b%d_ms" % (n, name, batch)] = sum(ms)
    elif mode == "--layers":
        res["calib_copy_gbs"] = float(hip.calibrate_copy())
        for kind, gates in (("lstm", 8), ("gru", 6)):
            cfg = HEAD + "[%s]\noutput=1024\n\n" % kind + TAIL
            for batch in (1, 32):
                ms = layer_ms(cfg, batch, [1])[0]
                wbytes = gates * 1024 * 1024 * 2
                res["%s_b%d_ms" % (kind, batch)] = ms
                res["%s_b%d_weight_gbs" % (kind, batch)] = wbytes / (ms * 1e-3) / 1e9
    elif mode == "--video":
        d = sys.argv[2]
        res["iters"] = 100
        for name in sorted(os.listdir(d)):
            if not name.endswith(".cfg"):
                continue
            cfg = open(os.path.join(d, name)).read()
            for batch in (1, 32):
                eng = hip.Engine(cfg, max_batch=batch, dtype=hip.BF16, semantics=hip.SEM_DARKNET)
                eng.set_weights(IO.synth_weights(IO.parse_cfg(cfg), seed=1))
                h, w = eng.input_hw
                eng.forward(np.random.default_rng(0).integers(0, 256, (batch, h, w, 3), dtype=np.uint8), want_detections=False)
                eng.time_forward(batch, 10, conv=False)
                ms, _ = eng.time_forward(batch, 100, conv=False)
                res["%s_b%d_steps_per_s" % (name[:-4], batch)] = 1e3 / ms
                res["%s_b%d_frames_per_s" % (name[:-4], batch)] = batch * 1e3 / ms
                eng.close()
    else:
        raise SystemExit(__doc__)
    with open(out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
