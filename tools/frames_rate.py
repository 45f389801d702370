"""Decoded-frame rate: what handing over a decoder's NV12 surfaces costs against packed RGB, YOLOv3-416, bf16, batch 32 of 1920 x 1080
frames, one process.

  host:   (a) detect_images on host-resident packed RGB  vs  (b) detect_frames on host-resident NV12 of the SAME pictures (the RGB is
          yolo_frame_to_rgb_host of the NV12, so both calls fit the same bytes and return the same records): host clock around the call,
          which ends in the copy of the records to the host; 3 bytes per pixel uploaded against 1.5.
  device: (c) detect_images_graph  vs  (d) detect_frames_graph on device-resident buffers: events on the engine's stream.
(a) / (b) and (c) / (d) run in alternating rounds (median step per round, median over rounds).

  python tools/frames_rate.py [--steps 30] [--host-steps 8] [--warmup 5] [--rounds 5] [--kernel-stats STATS_CSV] [--out JSON]

--only graph: time (c) and (d) alone (the process to run under `rocprofv3 --kernel-trace --stats`); --kernel-stats: read that run's
kernel_stats.csv and add the fit launches' own average durations (k_fit_images, k_fit_frames), their ratio and their bandwidths to the
line.  Bytes of a fit: the source bytes (each counted once) plus the network input written (32 x 416 x 416 x 8 bf16); GB/s against
8 TB/s, the MI355X's HBM peak.  Prints one JSON line (and writes it to --out)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
H, W = 1080, 1920


def fit_stats(path):
    """{kernel: (calls, average ns)} of the two fit kernels in a rocprofv3 kernel_stats.csv (every instantiation of a kernel added up)"""
    acc = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            for k in ("k_fit_images", "k_fit_frames"):
                if k in row["Name"]:
                    c, ns = acc.get(k, (0, 0.0))
                    acc[k] = (c + int(row["Calls"]), ns + float(row["Calls"]) * float(row["AverageNs"]))
    return {k: (c, ns / c) for k, (c, ns) in acc.items() if c}


def nv12_pictures(hip, count, seed=1):
    """`count` NV12 frames of smooth content with noise on it (Y: gradients, U / V: slower ones), as hip.Frame at the row's own pitch"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    out = []
    for k in range(count):
        Y = ((x * (k + 1) // 7 + y * 3 // (k + 2)) % 220 + 16 + rng.integers(0, 8, (H, W))).astype(np.uint8)
        U = ((cx // (3 + k) + 64) % 224 + 16).astype(np.uint8); V = ((cy // (2 + k) + 96) % 224 + 16).astype(np.uint8)
        out.append(hip.Frame(np.concatenate([Y.reshape(-1), np.stack([U, V], -1).reshape(-1)]), H, W, hip.PIX_NV12, matrix=hip.MATRIX_BT709))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--host-steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--only", choices=["both", "graph"], default="both")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
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

    distinct = nv12_pictures(hip, 4)
    rgb_distinct = [hip.frame_to_rgb(f) for f in distinct]
    fbuf, fdescs = hip.pack_frames([distinct[i % 4] for i in range(B)])
    ibuf, idescs = hip.pack_images([rgb_distinct[i % 4] for i in range(B)])
    post = dict(score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)

    # the two forms see the same pictures: the same records, bit for bit
    ra = eng.detect_images((ibuf, idescs), fit=hip.FIT_STRETCH, **post); rb = eng.detect_frames((fbuf, fdescs), fit=hip.FIT_STRETCH, **post)
    same = all(len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ra, rb))

    def host_timed(call):
        for _ in range(2):
            call()
        ts = []
        for _ in range(args.host_steps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            call()                                   # ends in the copy of the records to the host
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    ha, hb = [], []
    if args.only == "both":
        for _ in range(args.rounds):
            ha.append(host_timed(lambda: eng.detect_images((ibuf, idescs), fit=hip.FIT_STRETCH, **post)))
            hb.append(host_timed(lambda: eng.detect_frames((fbuf, fdescs), fit=hip.FIT_STRETCH, **post)))

    ipix = torch.from_numpy(ibuf).to(dev); fpix = torch.from_numpy(fbuf).to(dev)
    boxes_c = torch.zeros(B * max_out * 6, dtype=torch.int32, device=dev); counts_c = torch.zeros(B, dtype=torch.int32, device=dev)
    boxes_d = torch.zeros_like(boxes_c); counts_d = torch.zeros_like(counts_c)

    def step_c():
        eng.detect_images_graph(ipix, idescs, boxes_c, counts_c, fit=hip.FIT_STRETCH, **post)

    def step_d():
        eng.detect_frames_graph(fpix, fdescs, boxes_d, counts_d, fit=hip.FIT_STRETCH, **post)

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

    tc, td = [], []
    for _ in range(args.rounds):
        tc.append(timed(step_c)); td.append(timed(step_d))
    graph_same = bool(torch.equal(boxes_c, boxes_d) and torch.equal(counts_c, counts_d))

    dst_bytes = B * S * S * 8 * 2
    out = {
        "workload": "yolov3-416 bf16 batch %d of %d x %d frames: packed RGB (detect_images*) vs NV12 / BT709 (detect_frames*) of the same pictures, STRETCH fit" % (B, W, H),
        "tile_plan": os.path.basename(plan_path) if plan_loaded else "built-in",
        "records_equal": {"host": bool(same), "graph": graph_same},
        "source_bytes": {"rgb": int(ibuf.size), "nv12": int(fbuf.size)},
        "host_rgb_call_ms": float(np.median(ha)) if ha else None, "host_nv12_call_ms": float(np.median(hb)) if hb else None,
        "host_rgb_rounds_ms": ha, "host_nv12_rounds_ms": hb,
        "host_nv12_over_rgb": float(np.median(hb) / np.median(ha)) if ha else None,
        "graph_rgb_step_ms": float(np.median(tc)), "graph_nv12_step_ms": float(np.median(td)),
        "graph_rgb_rounds_ms": tc, "graph_nv12_rounds_ms": td,
        "graph_nv12_over_rgb": float(np.median(td) / np.median(tc)),
    }
    if args.kernel_stats:
        st = fit_stats(args.kernel_stats)
        fit = {}
        for k, src in (("k_fit_images", int(ibuf.size)), ("k_fit_frames", int(fbuf.size))):
            if k in st:
                calls, ns = st[k]
                gbs = (src + dst_bytes) / ns
                fit[k] = {"calls": calls, "avg_us": ns / 1e3, "gb_per_s": gbs, "frac_of_8tbs": gbs / HBM_PEAK_GBS}
        if len(fit) == 2:
            fit["frames_over_images"] = fit["k_fit_frames"]["avg_us"] / fit["k_fit_images"]["avg_us"]
        out["fit_launch"] = fit
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
