"""Classifier rate from files and frames: what the new entry points cost against today's way to the same answer.  darknet19 at 256 x 256, bf16, seeded
weights, max_batch 32, one process.

  files:  (a) classify_jpegs of 32 x dog.jpg (768 x 576, luma sampled 1 x 2), FIT_CENTER_CROP -- darknet's `classifier predict` preprocessing --, top-5:
              entropy stage on the host (min(n, 8) threads), one upload of the coefficients, one IDCT launch, fit + network + top-k
          (b) PIL decodes every file (ONE thread), classify_images over the decoded pictures
          split of (a): the entropy stage's wall time, the upload's bytes and device time, the IDCT launch's device time (Engine.jpeg_decode_times).
          PIL's decode (libjpeg) is not the reference's (stb_image): (a) and (b) do not see the same pixels; (a) equals classify_images over
          hip.jpeg_to_rgb, which the tool checks.
  frames: (c) classify_views_frames (VIEWS_TEN_CROP, shift 32, scale 1/10, top-5) over 32 host-resident 1920 x 1080 NV12 frames: 320 slots = 10 steps,
              1.5 bytes per pixel uploaded once
          (d) classify_views over the same pictures as host RGB (hip.frame_to_rgb of the frames: the same answer, which the tool checks): 3 bytes per pixel
Host clock around each call (each ends in the copy of the records to the host), median per round, median over rounds, rounds alternating.

          --entropy both | host | auto: (a) under each entropy mode, alternating within every round; "auto" decodes dog.jpg's 36 restart
          intervals per file on the device from the uploaded file bytes; its split adds Engine.jpeg_entropy_times.
  python tools/classify_files_rate.py [--host-steps 6] [--rounds 5] [--out JSON] [--only both | views] [--entropy both | host | auto] [--kernel-stats STATS_CSV]

--only views: run (c) and (d) alone (the process to run under `rocprofv3 --kernel-trace --stats`); --kernel-stats: read that run's kernel_stats.csv and add
the per-step view-fit launches' own average times (k_fit_frames over the view table, k_fit_images over the view table).  Prints one JSON line."""
import argparse
import csv
import importlib.util
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def view_fit_stats(path):
    """{kernel: calls, average us} of the two view fits in a rocprofv3 kernel_stats.csv: k_fit_images<.., ViewDesc, ..> and the FIT_TEN_CROP (5) view slot (2) of k_fit_frames"""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name = row["Name"]
            key = "k_fit_images" if "k_fit_images" in name and "ViewDesc" in name else "k_fit_frames" if "k_fit_frames" in name and ", 5, 2>" in name else None
            if key:
                out[key] = {"calls": int(row["Calls"]), "average_us": float(row["AverageNs"]) / 1e3, "name": name}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-steps", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["both", "views"], default="both")
    ap.add_argument("--entropy", choices=["both", "host", "auto"], default="both")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from PIL import Image
    from yolo_tensorflow_amd import hip, darknet_io as IO
    if not torch.cuda.is_available():
        raise SystemExit("classify_files_rate: no GPU: nothing is measured without one")
    spec = importlib.util.spec_from_file_location("frames_rate", os.path.join(ROOT, "tools", "frames_rate.py"))
    FR = importlib.util.module_from_spec(spec); spec.loader.exec_module(FR)

    B, S, K, shift, top = 32, 256, 10, 32, 5
    txt = IO.cfg_text("darknet19")
    eng = hip.Engine(txt, max_batch=B, dtype=hip.BF16, semantics=hip.SEM_DARKNET, device=0)
    if eng.input_hw != (S, S):
        raise SystemExit("classify_files_rate: darknet19 reads %s, 256 x 256 expected" % (eng.input_hw,))
    eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))

    def host_timed(call):
        for _ in range(2):
            call()
        ts = []
        for _ in range(args.host_steps):
            eng.synchronize()
            t0 = time.perf_counter()
            call()                                   # ends in the copy of the records to the host
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def same(a, b):
        return bool(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)))

    out = {"workload": "darknet19-256 bf16, max_batch 32: classify_jpegs vs PIL decode + classify_images (32 x dog.jpg, CENTER_CROP, top-5); "
                       "classify_views_frames vs classify_views (32 x 1920 x 1080 NV12 / the same pictures as RGB, ten-crop shift 32, top-5)"}

    if args.only == "both":
        with open(os.path.join(ROOT, "tests", "golden", "images", "dog.jpg"), "rb") as fh:
            data = fh.read()
        info = hip.jpeg_info(data)
        files = [data] * B
        twin = hip.jpeg_to_rgb(data)
        fit = hip.FIT_CENTER_CROP
        equal = same(eng.classify_jpegs(files, fit=fit, top_k=top), eng.classify_images([twin] * B, fit=fit, top_k=top))

        def pil_decode():
            return [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
        pictures = pil_decode()
        modes = ["host", "auto"] if args.entropy == "both" else [args.entropy]
        ta, tp, ti, split = [], [], [], []
        auto_ms, auto_split, auto_equal = [], [], None
        for _ in range(args.rounds):
            for m in modes:
                eng.set_jpeg_entropy(m)
                t = host_timed(lambda: eng.classify_jpegs(files, fit=fit, top_k=top))
                if m == modes[0]:
                    ta.append(t); split.append(eng.jpeg_decode_times())
                else:
                    auto_ms.append(t); auto_split.append(dict(eng.jpeg_decode_times(), **eng.jpeg_entropy_times()))
                    auto_equal = same(eng.classify_jpegs(files, fit=fit, top_k=top), eng.classify_images([twin] * B, fit=fit, top_k=top))
            eng.set_jpeg_entropy("host")
            tp.append(host_timed(pil_decode))
            ti.append(host_timed(lambda: eng.classify_images(pictures, fit=fit, top_k=top)))
        med = lambda k: float(np.median([s[k] for s in split]))
        out["files"] = {
            "picture": "dog.jpg", "h": info["h"], "w": info["w"], "format": info["format"], "file_bytes": len(data), "rgb_bytes": int(twin.size),
            "records_equal_host_twin": equal, "threads_note": "the entropy stage runs on min(n, 8) threads, PIL on one",
            "classify_jpegs_call_ms": float(np.median(ta)), "classify_jpegs_rounds_ms": ta,
            "pil_decode_ms": float(np.median(tp)), "pil_decode_rounds_ms": tp,
            "classify_images_call_ms": float(np.median(ti)), "classify_images_rounds_ms": ti,
            "pil_plus_classify_images_ms": float(np.median(tp) + np.median(ti)),
            "jpegs_over_pil_path": float(np.median(ta) / (np.median(tp) + np.median(ti))),
            "split": {"entropy_ms": med("entropy_ms"), "upload_ms": med("upload_ms"), "upload_bytes": int(split[-1]["upload_bytes"]), "idct_ms": med("idct_ms")},
            "entropy_mode": modes[0],
        }
        if auto_ms:
            amed = lambda k: float(np.median([s[k] for s in auto_split]))
            out["files"]["auto"] = {
                "classify_jpegs_call_ms": float(np.median(auto_ms)), "classify_jpegs_rounds_ms": auto_ms, "records_equal_host_twin": auto_equal,
                "auto_over_host": float(np.median(auto_ms) / np.median(ta)),
                "split": {"entropy_ms": amed("entropy_ms"), "upload_ms": amed("upload_ms"), "upload_bytes": int(auto_split[-1]["upload_bytes"]), "idct_ms": amed("idct_ms"),
                          "scan_ms": amed("scan_ms"), "device_entropy_ms": amed("device_ms"), "stream_bytes": int(auto_split[-1]["stream_bytes"]),
                          "device_files": auto_split[-1]["device_files"], "intervals": auto_split[-1]["intervals"]},
            }

    distinct = FR.nv12_pictures(hip, 4)
    rgb_distinct = [hip.frame_to_rgb(f) for f in distinct]
    fpacked = hip.pack_frames([distinct[i % 4] for i in range(B)])
    ipacked = hip.pack_images([rgb_distinct[i % 4] for i in range(B)])
    views = dict(shift=shift, scale=1.0 / K, top_k=top)
    call_frames = lambda: eng.classify_views_frames(fpacked, hip.VIEWS_TEN_CROP, **views)
    call_images = lambda: eng.classify_views(ipacked, hip.VIEWS_TEN_CROP, **views)
    equal = same(call_frames(), call_images())
    tf, tr = [], []
    for _ in range(args.rounds):
        tf.append(host_timed(call_frames)); tr.append(host_timed(call_images))
    out["frames"] = {
        "frame": "%d x %d NV12 / BT709" % (FR.W, FR.H), "slots": B * K, "steps": B * K // B, "records_equal": equal,
        "source_bytes": {"nv12": int(fpacked[0].size), "rgb": int(ipacked[0].size)},
        "classify_views_frames_call_ms": float(np.median(tf)), "classify_views_frames_rounds_ms": tf,
        "classify_views_call_ms": float(np.median(tr)), "classify_views_rounds_ms": tr,
        "frames_over_rgb": float(np.median(tf) / np.median(tr)),
        "view_fit_launch": view_fit_stats(args.kernel_stats) if args.kernel_stats else None,
    }
    tflops, clock = hip.calibrate()
    out["calib_tflops"], out["calib_clock_ghz"], out["rounds"], out["host_steps"] = tflops, clock, args.rounds, args.host_steps
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
