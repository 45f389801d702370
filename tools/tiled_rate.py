"""Tiled detection rate: what cutting a large image into windows costs on the device against what a user does today on the host.
YOLOv3-416, bf16, tests/golden/images/kite.jpg (1352 x 900), tile 416, overlap 64: 4 x 3 = 12 windows (checked), max_batch 12 = one network step.

  (a) Engine.detect_tiled on the whole image: one host-to-device copy of the image, the windowed fit, the network, the cross-window merge,
      ONE NMS over the image, records in the image's pixels;
  (b) the yardstick: Engine.detect_images over the 12 host-made crops (cut and packed once, outside the timed window): one copy of the
      crops, the fit, the same network step, NMS per WINDOW only -- no merge, boxes in each crop's own pixels, duplicates left in.
Both take host buffers and return host records, so every call ends in a device synchronise; they run in one process in alternating rounds,
each round a host-clock window of at least --seconds after --warmup calls; the median call time of every round and the spread over the
rounds are reported.  (a) - (b) is what the merge costs on top of an identical network step, less what (b) pays to copy 12 overlapping crops
instead of one image.

The tool also prints how many boxes the tiled call keeps on kite.jpg against the single 416 x 416 stretch of the whole image, at the same
thresholds.  The weights are SYNTHETIC: that is a count of boxes, not an accuracy claim.

  python tools/tiled_rate.py [--seconds 1.0] [--rounds 5] [--warmup 5] [--out FILE]      prints one JSON line (and writes it to FILE)

--only tiled | crops: time one of the two alone -- the process to run under `rocprofv3 --kernel-trace --stats`, whose per-kernel averages
would otherwise mix the two paths' launches of the same kernels."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["both", "tiled", "crops"], default="both")
    args = ap.parse_args()

    import torch
    from PIL import Image
    from yolo_tensorflow_amd import hip, darknet_io as IO
    if not torch.cuda.is_available():
        raise SystemExit("tiled_rate: no GPU: nothing is measured without one")

    S, tile, overlap, max_out = 416, 416, 64, 100
    img = np.ascontiguousarray(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "images", "kite.jpg")).convert("RGB")))
    wins = hip.tile_windows(img.shape[:2], tile, overlap)
    if img.shape[:2] != (900, 1352) or len(wins) != 12:
        raise SystemExit("tiled_rate: kite.jpg is %s and cuts into %d windows, 900 x 1352 and 12 expected" % (img.shape[:2], len(wins)))
    txt = IO.cfg_text("yolov3")
    eng = hip.Engine(txt, max_batch=len(wins), dtype=hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=0)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
    post = dict(score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)

    whole = hip.pack_images([img])
    crops = hip.pack_images([img[y0:y0 + h, x0:x0 + w] for y0, x0, h, w in wins])

    def call_tiled():
        return eng.detect_tiled(whole, tile=tile, overlap=overlap, fit=hip.FIT_STRETCH, relative=False, **post)

    def call_crops():
        return eng.detect_images(crops, fit=hip.FIT_STRETCH, units=hip.UNITS_SOURCE_PIXELS, **post)

    def timed(call):
        for _ in range(args.warmup):
            call()
        eng.synchronize()
        times = []
        t_end = time.perf_counter() + args.seconds
        while time.perf_counter() < t_end or len(times) < 10:
            t0 = time.perf_counter()
            call()                      # returns host records: the call has synchronised
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times)), len(times)

    ta, tb, calls = [], [], 0
    for _ in range(args.rounds):
        if args.only != "crops":
            m, n = timed(call_tiled); ta.append(m); calls += n
        if args.only != "tiled":
            m, n = timed(call_crops); tb.append(m); calls += n

    kept = None
    if args.only == "both":          # (a profiled run holds one path's launches only)
        kept = {"tiled_one_nms_per_image": int(len(call_tiled()[0])), "crops_nms_per_window_sum": int(sum(len(r) for r in call_crops())),
                "single_416_stretch": int(len(eng.detect_images([img], fit=hip.FIT_STRETCH, units=hip.UNITS_SOURCE_PIXELS, **post)[0])), "max_out": max_out,
                "note": "synthetic weights: a count of boxes, not an accuracy claim"}
    out = {
        "workload": "yolov3-416 bf16, kite.jpg 1352x900, tile 416 overlap 64 = 12 windows, max_batch 12 (one network step), host image in, host records out",
        "tiled_call_ms": float(np.median(ta)) if ta else None, "crops_call_ms": float(np.median(tb)) if tb else None,
        "tiled_rounds_ms": ta, "crops_rounds_ms": tb,
        "tiled_spread_ms": [min(ta), max(ta)] if ta else None, "crops_spread_ms": [min(tb), max(tb)] if tb else None,
        "tiled_minus_crops_ms": float(np.median(ta) - np.median(tb)) if ta and tb else None,
        "tiled_over_crops": float(np.median(ta) / np.median(tb)) if ta and tb else None,
        "bytes_copied_in": {"tiled": int(whole[0].size), "crops": int(crops[0].size)},
        "timed_calls": calls, "window_seconds": args.seconds, "rounds": args.rounds,
        "kept_boxes_synthetic_weights": kept,
    }
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
