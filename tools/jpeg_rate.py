"""JPEG-file rate: what feeding files costs, YOLOv3-416, bf16, seeded weights, batch 32 of one photograph -- kite.jpg (1352 x 900, 4:4:4) and
dog.jpg (768 x 576, luma sampled 1 x 2) of tests/golden/images --, one process.

  (a) detect_jpegs(files): entropy stage on the host (min(n, 8) threads), one upload of the coefficients, one IDCT launch, fit + network + NMS
      -- under each entropy mode of --entropy: "host", and "auto", which decodes the restart intervals of kite.jpg and dog.jpg on the
      device from the uploaded file bytes (giraffe.jpg has no restart interval: under "auto" it costs the host path plus the interval scan)
  (b) what a caller does without it: PIL decodes every file (one thread), detect_images over the decoded pictures
  host clock around each call (both end in the copy of the records to the host), median per round, median over rounds, rounds alternating.
  split of (a): the entropy stage's wall time, the upload's bytes and device time, the IDCT launch's device time (Engine.jpeg_decode_times); under "auto"
      also the interval scan's wall time, the device stage's time and the file bytes uploaded (Engine.jpeg_entropy_times).
  fit:  detect_frames_graph over the decoded table  vs  detect_frames_graph over RGB24 frames of the same pictures (the host twin's decodes),
        device-resident, events on the engine's stream: the two steps differ in the fit launch alone.

  python tools/jpeg_rate.py [--steps 30] [--host-steps 6] [--warmup 5] [--rounds 5] [--entropy both|host|auto] [--pictures kite dog giraffe] [--decode-only] [--out JSON]

Note that PIL's decode (libjpeg) is not the reference's (stb_image): (a) and (b) do not see the same pixels; (a) equals detect_images over
hip.jpeg_to_rgb, which the tool checks.  Prints one JSON line (and writes it to --out)."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--host-steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--entropy", choices=["both", "host", "auto"], default="both", help="the entropy modes to measure, alternating within every round")
    ap.add_argument("--pictures", nargs="+", default=["kite", "dog", "giraffe"])
    ap.add_argument("--decode-only", action="store_true", help="(a) alone: no PIL path, no fit comparison")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from PIL import Image
    from yolo_tensorflow_amd import hip, darknet_io as IO

    B, S, max_out = args.batch, 416, 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    txt = IO.cfg_text("yolov3")
    eng = hip.Engine(txt, max_batch=B, dtype=hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=0, stream=stream.cuda_stream)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
    plan_path = os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b%d_bf16.json" % (S, B))
    plan_loaded = False
    if os.path.exists(plan_path):
        plan = json.load(open(plan_path))
        if plan.get("num_cfgs") == hip.op_conv_num_cfgs() and len(plan["cfgs"]) == eng.num_layers:
            eng.set_tile_configs(plan["cfgs"]); plan_loaded = True
    modes = ["host", "auto"] if args.entropy == "both" else [args.entropy]
    if not hasattr(eng, "set_jpeg_entropy"):          # (a library from before the device stage: its one path, so that the same tool measures it)
        modes = ["host"]
    post = dict(score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)

    def host_timed(call):
        for _ in range(2):
            call()
        ts = []
        for _ in range(args.host_steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def timed(step):
        for _ in range(args.warmup):
            step()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        torch.cuda.synchronize(dev)
        ev[0].record(stream)
        for i in range(args.steps):
            step()
            ev[i + 1].record(stream)
        torch.cuda.synchronize(dev)
        return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)]))

    out = {"workload": "yolov3-416 bf16 batch %d of one JPEG photograph: detect_jpegs vs PIL decode + detect_images, STRETCH fit" % B,
           "tile_plan": os.path.basename(plan_path) if plan_loaded else "built-in", "pictures": {}}
    out["entropy_modes"] = modes
    for name in args.pictures:
        with open(os.path.join(ROOT, "tests", "golden", "images", name + ".jpg"), "rb") as fh:
            data = fh.read()
        info = hip.jpeg_info(data)
        files = [data] * B
        twin = hip.jpeg_to_rgb(data)
        ra = eng.detect_jpegs(files, fit=hip.FIT_STRETCH, **post); rb = eng.detect_images([twin] * B, fit=hip.FIT_STRETCH, **post)
        same = all(len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ra, rb))

        def pil_decode():
            return [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
        pictures = pil_decode() if not args.decode_only else None
        tp, ti = [], []
        ta, split, esplit, mode_same = {m: [] for m in modes}, {m: [] for m in modes}, {m: [] for m in modes}, {}
        for _ in range(args.rounds):
            for m in modes:
                if hasattr(eng, "set_jpeg_entropy"):
                    eng.set_jpeg_entropy(m)
                ta[m].append(host_timed(lambda: eng.detect_jpegs(files, fit=hip.FIT_STRETCH, **post)))
                split[m].append(eng.jpeg_decode_times())
                if hasattr(eng, "jpeg_entropy_times"):
                    esplit[m].append(eng.jpeg_entropy_times())
                rm = eng.detect_jpegs(files, fit=hip.FIT_STRETCH, **post)
                mode_same[m] = all(len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(rm, rb))
            if not args.decode_only:
                tp.append(host_timed(pil_decode))
                ti.append(host_timed(lambda: eng.detect_images(pictures, fit=hip.FIT_STRETCH, **post)))
        if hasattr(eng, "set_jpeg_entropy"):
            eng.set_jpeg_entropy("host")
        med = lambda rows, k: float(np.median([s[k] for s in rows]))
        by_mode = {}
        for m in modes:
            sp = split[m]
            by_mode[m] = {"detect_jpegs_call_ms": float(np.median(ta[m])), "detect_jpegs_rounds_ms": ta[m], "records_equal_host_twin": bool(mode_same[m]),
                          "split": {"entropy_ms": med(sp, "entropy_ms"), "upload_ms": med(sp, "upload_ms"), "upload_bytes": int(sp[-1]["upload_bytes"]), "idct_ms": med(sp, "idct_ms")}}
            if esplit[m]:
                es = esplit[m]
                by_mode[m]["split"].update({"device_files": es[-1]["device_files"], "host_files": es[-1]["host_files"], "intervals": es[-1]["intervals"],
                                            "scan_ms": med(es, "scan_ms"), "device_entropy_ms": med(es, "device_ms"), "stream_bytes": int(es[-1]["stream_bytes"])})
        entry = {"h": info["h"], "w": info["w"], "format": info["format"], "restart_interval": info["restart_interval"], "file_bytes": len(data), "rgb_bytes": int(twin.size),
                 "records_equal": {"host_twin": bool(same)}, "modes": by_mode}
        if len(modes) == 2:
            entry["auto_over_host"] = by_mode["auto"]["detect_jpegs_call_ms"] / by_mode["host"]["detect_jpegs_call_ms"]
        out["pictures"][name] = entry
        if args.decode_only:
            continue
        ta, split = ta[modes[0]], split[modes[0]]

        # the fit launch: the decoded table against RGB24 frames of the same pictures, both device-resident, through the captured frames step
        handle = eng.decode_jpegs(files)
        rbuf, rdescs = hip.pack_frames([hip.Frame(twin, twin.shape[0], twin.shape[1], hip.PIX_RGB24)] * B)
        rpix = torch.from_numpy(rbuf).to(dev)
        boxes_j = torch.zeros(B * max_out * 6, dtype=torch.int32, device=dev); counts_j = torch.zeros(B, dtype=torch.int32, device=dev)
        boxes_r = torch.zeros_like(boxes_j); counts_r = torch.zeros_like(counts_j)

        def step_j():
            eng.detect_frames_graph(handle.pixels, handle.descs, boxes_j, counts_j, nbytes=handle.nbytes, fit=hip.FIT_STRETCH, **post)

        def step_r():
            eng.detect_frames_graph(rpix, rdescs, boxes_r, counts_r, fit=hip.FIT_STRETCH, **post)
        tj, tr = [], []
        for _ in range(args.rounds):
            tj.append(timed(step_j)); tr.append(timed(step_r))
        graph_same = bool(torch.equal(boxes_j, boxes_r) and torch.equal(counts_j, counts_r))
        med = lambda k: float(np.median([s[k] for s in split]))
        entry["records_equal"]["graph_rgb24"] = graph_same
        entry.update({
            "detect_jpegs_call_ms": float(np.median(ta)), "detect_jpegs_rounds_ms": ta,
            "pil_decode_ms": float(np.median(tp)), "detect_images_call_ms": float(np.median(ti)), "pil_plus_detect_images_ms": float(np.median(tp) + np.median(ti)),
            "pil_decode_rounds_ms": tp, "detect_images_rounds_ms": ti,
            "jpegs_over_pil_path": float(np.median(ta) / (np.median(tp) + np.median(ti))),
            "split": {"entropy_ms": med("entropy_ms"), "upload_ms": med("upload_ms"), "upload_bytes": int(split[-1]["upload_bytes"]), "idct_ms": med("idct_ms"),
                      "upload_gb_per_s": split[-1]["upload_bytes"] / med("upload_ms") / 1e6},
            "graph_jpeg_table_step_ms": float(np.median(tj)), "graph_rgb24_step_ms": float(np.median(tr)),
            "graph_jpeg_rounds_ms": tj, "graph_rgb24_rounds_ms": tr, "fit_difference_us": float((np.median(tj) - np.median(tr)) * 1e3),
        })
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
