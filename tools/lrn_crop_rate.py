#!/usr/bin/env python3
"""What [crop], [normalization] and the centre-crop fit cost, measured in one process on one device.

    python tools/lrn_crop_rate.py [batch=32] [iters=30]

* rate: yolo_time_forward of cfg/zoo/alexnet-lrn.cfg and cfg/zoo/alexnet.cfg (bf16, fp16): the difference is one crop and two LRN launches (and the first
  conv on the tiled kernel over a layer tensor instead of the staged image);
* layers: yolo_time_layers of alexnet-lrn -- its [crop] and both [normalization] launches -- next to the same cfg with each [normalization] replaced by
  `[activation] activation=relu`, whose k_activate launch reads and writes the same tensor (in place: as many bytes as the out-of-place LRN moves);
* fit: the wall time of Engine.forward_images over the same `batch` images (the committed photographs, repeated) with FIT_CENTER_CROP and with
  FIT_LETTERBOX into a small network, so that the fit launch is most of the step.
Prints one JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from yolo_tensorflow_amd import hip, darknet_io as IO  # noqa: E402


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 32
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    out = {"batch": batch, "iters": iters, "rate": {}, "layers": {}, "fit": {}}
    lrn_text = IO.cfg_text("alexnet-lrn")
    twin_text = lrn_text.replace("[normalization]\nsize=5\nalpha=0.0001\nbeta=0.75\nkappa=2\n", "[activation]\nactivation=relu\n")
    assert twin_text.count("[activation]") == 2
    for dtype in ("bf16", "fp16"):
        for name, text in (("alexnet-lrn", lrn_text), ("alexnet", IO.cfg_text("alexnet")), ("alexnet-lrn-as-activation", twin_text)):
            secs = IO.parse_cfg(text)
            eng = hip.Engine(text, max_batch=batch, dtype=getattr(hip, dtype.upper()), semantics=hip.SEM_DARKNET)
            eng.set_weights(IO.synth_weights(secs, seed=0))
            eng.time_forward(batch, 5)
            total_ms, _ = eng.time_forward(batch, iters)
            out["rate"]["%s/%s" % (name, dtype)] = {"ms_per_forward": round(total_ms, 4), "images_per_sec": round(batch * 1e3 / total_ms, 1)}
            if name != "alexnet":
                eng.time_layers(batch, 3)
                ms = eng.time_layers(batch, iters)
                shapes = IO.layer_shapes(secs)
                # bytes of a launch: its output tensor written and as many read (the crop reads its window only), 8-channel granules of 2 bytes
                moved = lambda i: 2 * shapes[i][1] * shapes[i][2] * (-(-shapes[i][3] // 8) * 8) * 2 * batch
                out["layers"]["%s/%s" % (name, dtype)] = [
                    {"layer": i, "type": s["type"], "hwc": list(shapes[i][1:4]), "ms": round(float(ms[i]), 5),
                     "GB_per_s": round(moved(i) / (float(ms[i]) * 1e-3) / 1e9, 1) if ms[i] > 0 else None}
                    for i, s in enumerate(secs[1:]) if s["type"] in ("crop", "normalization", "activation")]
            eng.close()
    from PIL import Image
    img_dir = os.path.join(ROOT, "tests", "golden", "images")
    photos = [np.ascontiguousarray(np.asarray(Image.open(os.path.join(img_dir, n)).convert("RGB"))) for n in sorted(os.listdir(img_dir)) if n.endswith(".jpg")]
    imgs = [photos[i % len(photos)] for i in range(batch)]
    cfg = "[net]\nwidth=256\nheight=256\nchannels=3\n\n[convolutional]\nfilters=8\nsize=3\nstride=4\npad=1\nactivation=leaky\n\n[convolutional]\nfilters=8\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n"
    eng = hip.Engine(cfg, max_batch=batch, dtype=hip.BF16, semantics=hip.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(cfg), seed=0))
    packed = hip.pack_images(imgs)
    for rnd in range(3):          # the order alternates: neither fit is always the one that runs warm
        for fit_name, fit in (("center_crop", hip.FIT_CENTER_CROP), ("letterbox", hip.FIT_LETTERBOX))[::1 if rnd % 2 == 0 else -1]:
            eng.forward_images(packed, fit=fit, want_detections=False); eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                eng.forward_images(packed, fit=fit, want_detections=False)
            eng.synchronize()
            out["fit"].setdefault(fit_name, []).append(round((time.perf_counter() - t0) * 1e3 / iters, 4))
    eng.close()
    out["fit"]["unit"] = "ms per forward_images call of %d images (host copy of %d bytes included)" % (batch, packed[0].nbytes)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
