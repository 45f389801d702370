"""Ten-crop classification rate: darknet's `classifier valid10` views formed on the device against what a user does today on the host.
darknet19 at 256 x 256, bf16, max_batch 32, the six tests/golden/images jpgs repeated to 32 images, ten views each = 320 slots = 10 network steps.

  (a) Engine.classify_views on the 32 packed images (VIEWS_TEN_CROP, shift 32, scale 1/10, top-5): one host-to-device copy of the source bytes, per step
      one fit launch over the view table, the network and a device copy of the step's rows, then ONE launch that adds, scales and selects; 32 x 5
      records come back;
  (b) the yardstick, today's way to the same answer: the 320 views made on the host (float32 -- a crop of a RESIZED image is no uint8 image, so
      classify_images cannot take it: Engine.classify over [32, 256, 256, 3] float32 batches), ten uploads of 32 views, ten 32 x 1000 probability
      matrices back, the sum of each image's ten rows and the top-5 in numpy.  The views are made ONCE, outside the timed window (from the reference's
      pixel rule restated in numpy, tools/make_views_golden.py); what making them costs per call is reported beside it (host_views_build_ms, one run).
Both take host buffers and return host records; they run in one process in alternating rounds, each a host-clock window of at least --seconds after
--warmup calls; the median call time of every round and the spread over the rounds are reported, with calib_tflops (hip.calibrate) of the box.

  python tools/views_rate.py [--seconds 1.0] [--rounds 5] [--warmup 3] [--out FILE] [--kernel-stats STATS_CSV]      prints one JSON line

--only views | crops: time one of the two alone -- the process to run under `rocprofv3 --kernel-trace --stats`; --kernel-stats: read that run's
kernel_stats.csv and add the two new launches' own times (k_fit_images over the view table, k_view_reduce) to the line."""
import argparse
import csv
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JPGS = ["dog.jpg", "eagle.jpg", "giraffe.jpg", "horses.jpg", "kite.jpg", "person.jpg"]


def launch_stats(path):
    """{kernel: (calls, average ns)} of the view fit and the reduction in a rocprofv3 kernel_stats.csv"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            key = "k_fit_images" if "k_fit_images" in name and "ViewDesc" in name else "k_view_reduce" if "k_view_reduce" in name else None
            if key:
                out[key] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", choices=["both", "views", "crops"], default="both")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()

    import torch
    from PIL import Image
    from yolo_tensorflow_amd import hip, darknet_io as IO
    if not torch.cuda.is_available():
        raise SystemExit("views_rate: no GPU: nothing is measured without one")
    spec = importlib.util.spec_from_file_location("make_views_golden", os.path.join(ROOT, "tools", "make_views_golden.py"))
    V = importlib.util.module_from_spec(spec); spec.loader.exec_module(V)

    N, B, K, S, shift, top = 32, 32, 10, 256, 32, 5
    jpgs = [np.ascontiguousarray(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "images", n)).convert("RGB"))) for n in JPGS]
    imgs = [jpgs[i % len(jpgs)] for i in range(N)]
    txt = IO.cfg_text("darknet19")
    eng = hip.Engine(txt, max_batch=B, dtype=hip.BF16, semantics=hip.SEM_DARKNET, device=0)
    if eng.input_hw != (S, S):
        raise SystemExit("views_rate: darknet19 reads %s, 256 x 256 expected" % (eng.input_hw,))
    eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
    packed = hip.pack_images(imgs)

    t0 = time.perf_counter()
    per_jpg = [V.ten_crop_numpy(j, shift, S, S) for j in jpgs]          # (the six distinct images; a user's folder has 32)
    build_ms = (time.perf_counter() - t0) * 1e3 * N / len(jpgs)
    crops = np.ascontiguousarray(np.stack([per_jpg[i % len(jpgs)] for i in range(N)]).reshape(N * K, S, S, 3))

    def call_views():
        return eng.classify_views(packed, hip.VIEWS_TEN_CROP, shift=shift, scale=1.0 / K, top_k=top)

    def call_crops():
        rows = np.concatenate([eng.classify(crops[lo:lo + B], top_k=0, scale=1.0) for lo in range(0, N * K, B)]).reshape(N, K, -1)
        s = np.zeros((N, rows.shape[2]), np.float32)
        for v in range(K):
            s = s + rows[:, v]
        s = s * np.float32(1.0 / K)
        cls = np.argsort(-s, axis=1, kind="stable")[:, :top]
        return cls.astype(np.int32), np.take_along_axis(s, cls, axis=1)

    def timed(call):
        for _ in range(args.warmup):
            call()
        eng.synchronize()
        times = []
        t_end = time.perf_counter() + args.seconds
        while time.perf_counter() < t_end or len(times) < 5:
            t0 = time.perf_counter()
            call()                      # returns host records: the call has synchronised
            times.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(times)), len(times)

    same = None
    if args.only == "both":
        a, b = call_views(), call_crops()
        same = {"classes_equal": bool(np.array_equal(a[0], b[0])), "means_bit_equal": bool(np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))}
    ta, tb, calls = [], [], 0
    for _ in range(args.rounds):
        if args.only != "crops":
            m, n = timed(call_views); ta.append(m); calls += n
        if args.only != "views":
            m, n = timed(call_crops); tb.append(m); calls += n
    tflops, clock = hip.calibrate()
    out = {
        "workload": "darknet19-256 bf16, six jpgs repeated to 32 images, ten-crop (shift 32) = 320 slots, max_batch 32 (10 network steps), host images in, host top-5 out",
        "views_call_ms": float(np.median(ta)) if ta else None, "crops_call_ms": float(np.median(tb)) if tb else None,
        "views_rounds_ms": ta, "crops_rounds_ms": tb,
        "views_spread_ms": [min(ta), max(ta)] if ta else None, "crops_spread_ms": [min(tb), max(tb)] if tb else None,
        "crops_over_views": float(np.median(tb) / np.median(ta)) if ta and tb else None,
        "host_views_build_ms": build_ms, "host_views_build_note": "numpy restatement of the pixel rule, made once outside the timed window; not part of crops_call_ms",
        "bytes_copied_in": {"views": int(packed[0].size), "crops": int(crops.nbytes)},
        "bytes_copied_out": {"views": N * top * 8, "crops": int(N * K * eng.num_classes * 4)},
        "same_answer": same,
        "timed_calls": calls, "window_seconds": args.seconds, "rounds": args.rounds,
        "calib_tflops": tflops, "calib_clock_ghz": clock,
        "launches": launch_stats(args.kernel_stats) if args.kernel_stats else None,
    }
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
