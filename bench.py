#!/usr/bin/env python3
"""Headline benchmark: YOLOv3 416x416, batch 32 per GPU, bf16, detect path (conv stack + decode + threshold + NMS
[+ RCCL all-gather of the box records when N > 1]) -> whole-job images/s, one JSON line on rank 0.

  python bench.py --gpus 1 --steps 50 --warmup 10
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Inputs (uint8 NHWC images) are resident in HBM before the timed region; weights are the seeded synthetic
stream (no real .weights ships with the reference).  A plain run sets up, warms up, times --steps steps and
prints the headline line.  --full adds the legs that take runs of their own, after the timed region:
`roofline` prices the dominant kernel (the fused implicit-GEMM conv) with HIP events recorded by the library
on its own stream, plus the batch-1 latency, the calibration yardsticks, `parity` against the fp32 oracle,
`tolerance_line` and `cpu_baseline` (the reference's own C code, oracle/_ref, on the host cores for a bounded
sample).  --dump-outputs DIR writes the box records of the last timed step as DIR/<name>.npy (float32).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md, chip-level parameters)
PEAK_FP8_TFLOPS = 5000.0       # dense e4m3 through v_mfma_*_f8f6f4 (same table)
PEAK_F32_TFLOPS = 157.3        # v_mfma_f32_16x16x4_f32: exact fp32 at the vector rate (same table, "Peak FP32 (matrix)")


def dump_outputs(out_dir, boxes, counts, max_out):
    """What a caller of the timed step receives, as float32 arrays in `out_dir`: the yolo_box records (x0, y0, x1, y1, score, cls)
    of every image, boxes [n, max_out, 4], scores / classes [n, max_out], and counts [n].  Slots past an image's count hold
    nothing the library promises: they are written as zeros (class -1), so that two builds compare record for record."""
    recs = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, max_out, 6)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(recs.shape[0])
    keep = np.arange(max_out)[None, :] < counts[:, None]
    f = recs.view(np.float32)
    arrays = {"boxes": np.where(keep[..., None], f[..., :4], np.float32(0)),
              "scores": np.where(keep, f[..., 4], np.float32(0)),
              "classes": np.where(keep, recs[..., 5], -1),
              "counts": counts}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float32))


def cpu_baseline(cfg_txt, flat, budget_s=25.0):
    """The reference's CPU path on this host: darknet `network_predict`, batch 1, all cores (its own `speed`
    method, D2T/examples/darknet.c:116-134).  Falls back to the numpy restatement when oracle/_ref is absent."""
    cores = os.cpu_count() or 1
    rng = np.random.default_rng(1)
    img = rng.random((416, 416, 3), dtype=np.float32)
    try:
        from oracle import darknet_ref as D
        if not D.available():
            raise RuntimeError("oracle/_ref not built")
        os.environ.setdefault("OMP_NUM_THREADS", str(cores))
        net = D.RefNet(cfg_txt, flat, 0, 2)
        net.predict(img)                     # warm-up
        times = []
        t_end = time.time() + budget_s
        while len(times) < 5 and (time.time() < t_end or len(times) < 2):
            t = time.time(); net.predict(img); times.append(time.time() - t)
        net.close()
        kind = "reference"
    except Exception as e:      # noqa: BLE001
        from oracle import yolo_ref as R
        secs = R.parse_cfg(cfg_txt); params = R.unflatten_weights(flat, secs)
        R.forward(secs, params, img[None])
        times = []
        for _ in range(2):
            t = time.time(); R.forward(secs, params, img[None]); times.append(time.time() - t)
        kind = "port"
    med = float(np.median(times))
    return {"value": round(1.0 / med, 4), "unit": "img/s", "cores": cores, "kind": kind,
            "sample": "%d x YOLOv3-416 batch-1 forward after 1 warm-up, median %.3f s/image" % (len(times), med)}


def oracle_boxes(cfg_txt, flat, imgs_u8, size, thr=0.5):
    """fp32 oracle (TF semantics) on the given images: per image (boxes, scores, rows) of every candidate above `thr`.  Host, outside the timed region."""
    from oracle import yolo_ref as R
    osecs = R.parse_cfg(cfg_txt); params = R.unflatten_weights(flat, osecs)
    refs = []
    for b in range(imgs_u8.shape[0]):
        heads, _ = R.forward(osecs, params, imgs_u8[b:b + 1].astype(np.float32) / np.float32(255))
        ref = R.yolo_v3_detections(heads, size, ratio=True)[0]
        rb, rs, rc, ridx = R.select_threshold(ref, thr)
        refs.append((rb, rs, ridx))
    return refs


def parity(eng, refs, imgs_u8, thr=0.5, margin=1e-2, t_oracle=0.0):
    """Boxes of the timed engine (its dtype, its tile plan) against the fp32 oracle (TF semantics) on the first images of the timed batch:
    over every oracle candidate whose score clears `thr` by more than `margin` (a candidate inside the band may legitimately flip),
    min IoU and max |dscore|.  The checker runs on the host outside the timed region; tests/test_gpu_tuned.py asserts the same measure
    over all 32 images."""
    t0 = time.time()
    det = eng.forward(imgs_u8)
    miou, mds, cnt, lost = 1.0, 0.0, 0, 0
    for b in range(imgs_u8.shape[0]):
        rb, rs, ridx = refs[b]
        ok = rs >= thr + margin
        if not ok.any():
            continue
        d = det[b][ridx[ok]]
        sc = (d[:, 4:5] * d[:, 5:]).max(-1)
        bx = np.stack([d[:, 0] - d[:, 2] / 2, d[:, 1] - d[:, 3] / 2, d[:, 0] + d[:, 2] / 2, d[:, 1] + d[:, 3] / 2], -1)
        a = rb[ok]
        ix = np.maximum(0, np.minimum(a[:, 2], bx[:, 2]) - np.maximum(a[:, 0], bx[:, 0])); iy = np.maximum(0, np.minimum(a[:, 3], bx[:, 3]) - np.maximum(a[:, 1], bx[:, 1]))
        inter = ix * iy
        iou = inter / ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) + (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1]) - inter + 1e-12)
        miou = min(miou, float(iou.min())); mds = max(mds, float(np.abs(rs[ok] - sc).max())); cnt += int(ok.sum()); lost += int((sc <= thr).sum())
    return {"min_iou": round(miou, 5), "max_dscore": round(mds, 5), "candidates": cnt, "lost": lost, "images": int(imgs_u8.shape[0]),
            "meets_north_star_iou_0p999": bool(miou >= 0.999 and lost == 0),
            "reference": "fp32 oracle (oracle/yolo_ref.py, TF semantics)", "weights": "seeded synthetic darknet stream (seed 0), benign batch-norm statistics",
            "threshold": thr, "margin": margin, "seconds": round(time.time() - t0 + t_oracle, 1)}


def tolerance_line(hip, IO, base_cfg_txt, flat, args, dev, stream, images, refs, imgs_par, kind):
    """The configuration that MEETS north_star's tolerance (decoded boxes within IoU >= 0.999 of the fp32 reference), timed in the same process
    on the same resident batch, after and outside the headline's timed region.  bf16 -- BASELINE's named type, the
    headline -- has an 8-bit significand and cannot hold 0.999 (1 - IoU falls 4-5 x per 2 bits, 0.999 needs 13-17); this
    leg is the fastest configuration of the library that does on every weight flavour of tests/test_gpu_fp16x2.py (benign, drawn and real
    trained-file statistics) and on all 32 images of this batch (tests/test_gpu_tuned.py): split-fp16 pairs
    (22 significant bits, W_hi x_hi + W_hi x_lo + W_lo x_hi on the fp16 MFMA = 3 MFMA products per algorithmic product, fp32 accumulation).
    Same step (uint8 batch resident in HBM -> conv stack -> decode -> threshold -> TF-NMS), same graph replay, same event timing."""
    import torch
    from yolo_tensorflow_amd import dist as ydist
    B = int(images.shape[0]); max_out = 20
    cfg_txt = base_cfg_txt; products = 3.0; what = "split fp16 pairs (hi + lo, interleaved per 32-channel group) on every tensor and filter; pair K loop: W_hi x_hi + W_lo x_hi + W_hi x_lo per K-step row pair"
    eng = hip.Engine(cfg_txt, max_batch=B, dtype=hip.FP16X2, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=dev.index, stream=stream.cuda_stream)
    try:
        eng.set_weights(flat)
        eng.forward(images, want_detections=False)
        tuned = os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b%d_%s.json" % (args.size, B, kind))
        loaded = False
        if os.path.exists(tuned):
            plan = json.load(open(tuned))
            if plan.get("num_cfgs") == hip.op_conv_num_cfgs() and len(plan["cfgs"]) == eng.num_layers:
                eng.set_tile_configs(plan["cfgs"]); loaded = True
        rec, boxes, counts = ydist.alloc_flat_records(B, max_out, dev)

        def step():
            eng.detect_graph(images, boxes, counts, score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)
        for _ in range(max(3, args.warmup)):
            step()
        steps = max(5, min(args.steps, 50))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize(dev)
        elapsed = time.perf_counter() - t0
        total_ms, conv_ms = eng.time_forward(B, 5, conv=True)
        flops = eng.conv_flops() * B
        achieved = flops / (conv_ms * 1e-3) / 1e12
        out = {"dtype": kind, "what": what, "value": round(B * steps / elapsed, 2), "unit": "img/s", "ms_per_step": round(elapsed / steps * 1e3, 4), "steps": steps,
               "tile_plan": os.path.basename(tuned) if loaded else "built-in",
               "roofline": {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                            "mfma_products": products, "mfma_tflops": round(achieved * products, 2), "mfma_frac": round(achieved * products / PEAK_BF16_TFLOPS, 4),
                            "kernel_ms_per_forward": round(conv_ms, 4), "forward_ms": round(total_ms, 4),
                            "note": "achieved / frac count the ALGORITHMIC FLOPs (the reference's formula); mfma_* the products the matrix pipe executes"},
               "tolerance": "north_star: decoded boxes within IoU >= 0.999 of the fp32 reference on identical inputs"}
        if not args.no_calibration:      # the fp16 MFMA's own yardstick on this box (the pair K loop runs v_mfma_f32_16x16x32_f16)
            ct, cg = hip.calibrate(0.3, f16=True, device=dev.index, stream=stream.cuda_stream)
            out["roofline"].update({"calib_tflops": round(ct, 1), "clock_ghz": round(cg, 3), "mfma_frac_of_calib": round(achieved * products / ct, 4) if ct > 0 else None})
        if refs is not None:
            out["parity"] = parity(eng, refs, imgs_par)
        return out
    finally:
        eng.close()


def latency_b1(hip, cfg_txt, flat, args, dev, stream, fp8, fp32, fp16, x2, eng1=None, iters=200):
    """BASELINE.json's metric also names 'p50 ms/image': `p50_ms_per_image` of the main line is the throughput reciprocal (a batch-32 step / 32).
    This leg is the LATENCY of one image: a context of its own with max_batch 1 (built-in tile plan, or tuned/yolov3_<size>_b1_<dtype>.json
    when one is committed), the same detect step replayed from its HIP graph, the host synchronised after every image.  Wall clock per
    call (submission + device + completion) and device time between events, p50 over `iters` calls; outside the timed region."""
    import torch
    from yolo_tensorflow_amd import dist as ydist
    eng = eng1 or hip.Engine(cfg_txt, max_batch=1, dtype=hip.FP8 if fp8 else hip.FP32 if fp32 else hip.FP16 if fp16 else hip.FP16X2 if x2 else hip.BF16,
                             semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=dev.index, stream=stream.cuda_stream)
    if eng1 is None:
        eng.set_weights(flat)
        tuned = os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b1_%s.json" % (args.size, "bf16" if fp16 else args.dtype))
        if os.path.exists(tuned):
            plan = json.load(open(tuned))
            if plan.get("num_cfgs") == hip.op_conv_num_cfgs() and len(plan["cfgs"]) == eng.num_layers:
                eng.set_tile_configs(plan["cfgs"])
    img = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (1, args.size, args.size, 3), dtype=np.uint8)).to(dev)
    rec, boxes, counts = ydist.alloc_flat_records(1, 20, dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wall, devms = [], []
    for it in range(iters + 10):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        e0.record(stream)
        eng.detect_graph(img, boxes, counts, score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)
        e1.record(stream)
        torch.cuda.synchronize(dev)
        if it >= 10:
            wall.append((time.perf_counter() - t0) * 1e3); devms.append(e0.elapsed_time(e1))
    if eng1 is None:
        eng.close()
    return {"latency_b1_ms": round(float(np.median(wall)), 4), "latency_b1_device_ms": round(float(np.median(devms)), 4),
            "latency_b1_p99_ms": round(float(np.percentile(wall, 99)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="images per GPU per step (weak scaling: the global batch grows with --gpus)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="STRONG scaling: a fixed global batch split contiguously over the ranks (earlier ranks take the remainder); "
                         "0 = off (weak scaling, --batch images per GPU).  BASELINE.json's 'batch=32, 1/2/4/8x' read as one batch of 32 is "
                         "--global-batch 32: 32 / 16 / 8 / 4 images per GPU")
    ap.add_argument("--config4", action="store_true", help="BASELINE.json config 4: 608x608, global batch 64 sharded over the ranks (= --size 608 --global-batch 64)")
    ap.add_argument("--parity-images", type=int, default=2, help="images of the timed batch whose boxes are compared with the fp32 oracle for the `parity` field (rank 0, N = 1; 0 = skip)")
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-latency", action="store_true", help="skip the batch-1 latency leg (`latency_b1_ms`: one image per call, graph replay, synchronised per image; rank 0, N = 1, outside the timed region)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a HIP graph")
    ap.add_argument("--retune", action="store_true", help="ignore the persisted tile plan and autotune")
    ap.add_argument("--no-tune", action="store_true", help="no committed tile plan for this (size, batch, dtype): run the library's built-in plan instead of autotuning (functional runs)")
    ap.add_argument("--dtype", choices=("bf16", "fp8", "fp32", "fp16", "mixed", "fp16x2", "mixed16"), default="bf16",
                    help="bf16 is BASELINE.json's headline configuration; fp8 is its config 5; fp32 is the exact-fp32 MFMA path, the one "
                         "that meets north_star's IoU >= 0.999; fp16 is the bf16 configuration with IEEE fp16 storage (same kernels, plans and "
                         "MFMA rate, 11-bit significand); mixed is config 5 with the layers named in tuned/yolov3_*_mixed.json kept in bf16 "
                         "(the plan that brings the e4m3 configuration's boxes back to IoU >= 0.97); fp16x2 is split-fp16 storage (pairs of fp16 numbers, "
                         "three MFMA products per algorithmic one): the 16-bit-MFMA configuration that meets IoU >= 0.999 on trained-file statistics "
                         "; mixed16 is the split-fp16 network with pairs only on the first layers (tuned/yolov3_*_mixed16.json: where rounding noise is amplified most), "
                         "plain fp16 and the fp16 configuration's fused kernels after them "
                         "(each reported as a separate line)")
    ap.add_argument("--tolerance", choices=("fp16x2", "none"), default="fp16x2",
                    help="after the headline leg, time the configuration that meets north_star's IoU >= 0.999 in the same process and print it inside the "
                         "same JSON line as `tolerance_line` (rank 0, N = 1, default workload only; outside the headline's timed region)")
    ap.add_argument("--no-calibration", action="store_true", help="skip roofline.calib_tflops / clock_ghz (the register-resident MFMA yardstick, 0.4 s)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the legs that take runs of their own: `roofline` (library events per forward), the batch-1 "
                         "latency, the calibration yardsticks, `parity`, `tolerance_line`, `cpu_baseline` and the functional exchange check of "
                         "BENCH_BACKEND=gloo (each still subject to its --no-* / --parity-images / --tolerance option); off: the headline line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the box records of the last timed step (rank 0: the global batch when N > 1) as DIR/{boxes,scores,classes,counts}.npy, float32")
    args = ap.parse_args()
    if args.config4:
        args.size, args.global_batch = 608, args.global_batch or 64

    import torch
    import torch.distributed as dist
    from yolo_tensorflow_amd import hip, darknet_io as IO, dist as ydist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    force_dist = os.environ.get("BENCH_FORCE_DIST") == "1"      # exercise the RCCL path at world size 1 (testing only)
    # BENCH_BACKEND=gloo: a FUNCTIONAL multi-rank run on whatever GPUs there are -- ranks beyond the device count share GPUs (two ranks on the one
    # GPU of a test box), the box records are exchanged through pinned host buffers by gloo instead of RCCL (dist.HostStagedGather).  It runs
    # every line of the N > 1 path (shard bounds, per-rank seeds, ragged splits, the pipelined exchange, the MAX-reduce, the rank-0 print) on a
    # real device; it says nothing about scaling, and the line says so.  (device_count() does not initialise the GPU on this image.)
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    if backend == "gloo":
        local_rank = local_rank % max(1, torch.cuda.device_count())
    if world > 1 or force_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29533")
        if backend == "gloo":
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    cfg_txt = IO.cfg_text("yolov3") if args.size == 416 else IO.with_input_size(IO.cfg_text("yolov3"), args.size)
    secs = IO.parse_cfg(cfg_txt)
    flat = IO.synth_weights(secs, seed=0)
    G = world
    strong = args.global_batch > 0
    if strong:      # fixed global batch: this rank's share (ragged when G does not divide it); B = the largest share = every rank's buffer size
        GB = args.global_batch
        if GB < G:
            raise SystemExit("--global-batch %d < %d ranks" % (GB, G))
        lo, hi = ydist.shard_bounds(GB, G, rank)
        B = -(-GB // G)
    else:
        B = args.batch; GB = B * G; lo, hi = ydist.shard_bounds(GB, G, rank)
    n_local = hi - lo
    max_out = 20
    # A stream of our own, made torch's current one (events, RCCL and the library all enqueue on it): a created stream can be captured, so
    # the step replays as one HIP graph.  (torch's default stream is the legacy NULL stream, handle 0: hip.Engine passes it on as
    # hipStreamLegacy -- stream-ordered too, but not capturable, the step is then launched eagerly, BENCH_NULL_STREAM=1.  Until that
    # mapping existed, handle 0 read as "no stream given" at the boundary and the wrapper's host-side wait for torch's stream, which on
    # the NULL stream also waits for the engine's own previous replay, put the whole submission latency between consecutive steps:
    # 2.67 ms of host time per step against 21 us, same-box 2.720 -> 2.665 ms per step.)
    stream = torch.cuda.current_stream(dev) if os.environ.get("BENCH_NULL_STREAM") else torch.cuda.Stream(dev)      # (the variable: for the A/B only)
    torch.cuda.set_stream(stream)
    mixed = args.dtype == "mixed"
    fp8 = args.dtype == "fp8" or mixed
    fp32 = args.dtype == "fp32"
    if mixed:      # an fp8 network whose cfg text keeps the named layers in bf16 (darknet_io.with_layer_store)
        mplan = json.load(open(os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b%d_mixed.json" % (args.size, B))))
        cfg_txt = IO.with_layer_store(cfg_txt, mplan["store_bf16"])
    peak = PEAK_FP8_TFLOPS if fp8 else PEAK_F32_TFLOPS if fp32 else PEAK_BF16_TFLOPS
    if mixed:      # the time both matrix pipes would need at their peaks: the bf16 share of the FLOPs at 2.5 PFLOP/s, the rest at 5
        share = IO.bf16_flop_share(IO.parse_cfg(cfg_txt))
        peak = round(1.0 / (share / PEAK_BF16_TFLOPS + (1.0 - share) / PEAK_FP8_TFLOPS), 1)
    fp16 = args.dtype == "fp16"
    m16 = args.dtype == "mixed16"
    x2 = args.dtype == "fp16x2" or m16
    if m16:        # a split-fp16 network whose cfg text says which tensors are pairs (darknet_io.with_layer_pairs): the first layers, per the plan file
        m16plan = json.load(open(os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b%d_mixed16.json" % (args.size, B))))
        m16pair = IO.pair_closure(IO.parse_cfg(cfg_txt), set(range(-1, int(m16plan["pairs_upto"]) + 1)))
        m16share = IO.pair_flop_share(IO.parse_cfg(cfg_txt), m16pair)
        cfg_txt = IO.with_layer_pairs(cfg_txt, m16pair)
    eng = hip.Engine(cfg_txt, max_batch=B, dtype=hip.FP8 if fp8 else hip.FP32 if fp32 else hip.FP16 if fp16 else hip.FP16X2 if x2 else hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO,
                     device=local_rank, stream=stream.cuda_stream)
    eng.set_weights(flat)
    # this rank's shard of the global batch (weak scaling: B images per GPU; strong: n_local of GB), resident in HBM
    rng = np.random.default_rng(1 + rank)
    images = torch.from_numpy(rng.integers(0, 256, (hi - lo, args.size, args.size, 3), dtype=np.uint8)).to(dev)
    # one flat record buffer per rank: [B * max_out] box records (6 x int32 each) followed by [B] counts, written in place by
    # the library, so the exchange is ONE all_gather_into_tensor straight from the library's output (equal shards: every
    # rank ends up with the global batch in rank order)
    rec, boxes, counts = ydist.alloc_flat_records(B, max_out, dev)
    # the exchange of step n runs under the compute of step n+1 (dist.PipelinedGather); the last one is waited for inside the timed region
    gather = (ydist.HostStagedGather(rec) if backend == "gloo" else ydist.PipelinedGather(rec)) if (world > 1 or force_dist) else None
    eng.forward(images, want_detections=False)
    # per-layer tile choices: reuse a persisted plan for this (workload, batch) if one is committed, else autotune
    # (fp16 runs the bf16 configuration's kernels shape for shape: it shares that plan)
    tuned = os.path.join(ROOT, "yolo_tensorflow_amd", "tuned", "yolov3_%d_b%d_%s.json" % (args.size, B, "bf16" if fp16 else args.dtype))
    tuned = os.environ.get("BENCH_PLAN") or tuned                  # (probes: another plan file for the same workload)
    loaded = False
    if os.path.exists(tuned) and not args.retune:
        try:
            plan = json.load(open(tuned))
            if plan.get("num_cfgs") == hip.op_conv_num_cfgs() and len(plan["cfgs"]) == eng.num_layers:
                eng.set_tile_configs(plan["cfgs"]); loaded = True
        except Exception:      # noqa: BLE001
            loaded = False
    if not loaded and args.no_tune:
        pass                      # the library's built-in plan (functional runs at batch sizes without a committed plan)
    elif not loaded:
        eng.autotune(B, int(os.environ.get("BENCH_TUNE_ITERS", "5")))
        if rank == 0:
            out_dir = os.path.join(ROOT, "gpurun_out"); os.makedirs(out_dir, exist_ok=True)
            json.dump({"num_cfgs": hip.op_conv_num_cfgs(), "cfgs": [int(v) for v in eng.get_tile_configs()]},
                      open(os.path.join(out_dir, os.path.basename(tuned)), "w"))

    def step():
        if args.no_graph:
            eng.forward(images, want_detections=False)
            eng.postprocess(n_local, score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT,
                            boxes_out=boxes, counts_out=counts)
        else:   # same launches, replayed from a HIP graph captured on the second call
            eng.detect_graph(images, boxes, counts, score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF,
                             select_mode=hip.SELECT_GT)
        if gather is not None:
            gather.submit(rec)
        return None

    for _ in range(args.warmup):
        step()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    if G > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    ev[0].record(stream)
    for i in range(args.steps):
        step()
        ev[i + 1].record(stream)
    gathered = None
    if gather is not None:
        gathered = gather.result()              # the last step's exchange completes inside the timed region
    torch.cuda.synchronize(dev)
    if G > 1:
        dist.barrier()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    if G > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if backend == "gloo" else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    step_ms = np.array([ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps)])
    if args.dump_outputs and rank == 0:
        # the last timed step's records, before anything else runs on the engine: this rank's buffers, or the gathered global batch
        if gathered is not None:
            out_boxes, out_counts = ydist.split_flat_records_ragged(gathered, GB, max_out)
        else:
            out_boxes, out_counts = boxes[:n_local], counts[:n_local]
        dump_outputs(args.dump_outputs, out_boxes.cpu().numpy(), out_counts.cpu().numpy(), max_out)
    exchange_ok = None
    if args.full and gather is not None and backend == "gloo":
        # functional check of the exchange: one more step, gathered; this rank's slot must hold its own records, and the counts of all ranks
        # must be those of n_local real images followed by the zero padding of a short rank
        step(); allrec = gather.result()
        mine = rec.cpu()
        ok = bool(torch.equal(allrec[rank], mine))
        for r in range(G):
            rlo, rhi = ydist.shard_bounds(GB, G, r)
            cnt = allrec[r][B * max_out * ydist.RECORD_FLOATS:]
            ok = ok and bool((cnt[rhi - rlo:] == 0).all()) and bool((cnt[:rhi - rlo] >= 0).all()) and bool((cnt[:rhi - rlo] <= max_out).all())
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
        if G > 1:
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        exchange_ok = bool(flag.item())

    if rank == 0:
        out = {
            "metric": "images_per_sec", "value": round(GB * args.steps / elapsed, 2), "unit": "img/s",
            "n_gpus": G, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True, "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "YOLOv3 %dx%d %s, %s: conv stack + head decode + threshold + TF-NMS%s"
                                   % (args.size, args.size, ("global batch=%d split over %d GPU(s), %d image(s) on rank 0" % (GB, G, n_local)) if strong else "batch=%d per GPU" % B, "e4m3 backbone to 26x26 + bf16 13x13 stage and FPN (tuned/yolov3_%d_b%d_mixed.json), fp32 heads" % (args.size, B) if mixed else "e4m3 filters and activations (scales 1), fp32 heads" if fp8 else "exact fp32 (f32 MFMA)" if fp32 else "fp16 storage, fp32 accumulation" if fp16 else ("split fp16 pairs (hi + lo) on cfg layers 0..%d and the image -- %.0f %% of the conv FLOPs at 3 MFMA products per algorithmic one --, plain fp16 storage and the fp16 configuration's fused kernels after them (tuned/yolov3_%d_b%d_mixed16.json), fp32 accumulation" % (int(m16plan["pairs_upto"]), 100 * m16share, args.size, B)) if m16 else "split fp16 pairs (hi + lo), W_hi x_hi + W_hi x_lo + W_lo x_hi on the fp16 MFMA = 3 MFMA products per algorithmic product (roofline.achieved counts the ALGORITHMIC FLOPs against the 2.5 PFLOP/s peak: at most 1/3 of it), fp32 accumulation, shortcuts folded into the conv epilogues, no stem / block / 1x1-tail fusions" if x2 else "bf16",
                                      " + RCCL all-gather of box records" if G > 1 else ""),
                       "global_batch": GB, "input": "uint8 NHWC resident in HBM", "weights": "seeded synthetic darknet stream (seed 0)",
                       "parallelism": "dp%d" % G if G == 1 else
                                      "dp%d; the box-record all-gather of step n runs under the compute of step n+1 (dist.PipelinedGather): "
                                      "p50_ms_* are per-step compute on rank 0 and EXCLUDE the exchange, value / ms_per_step include every "
                                      "exchange (the last one is waited for inside the timed region)" % G},
            "p50_ms_per_image": round(float(np.median(step_ms)) / n_local, 5),
            "p50_ms_per_batch": round(float(np.median(step_ms)), 4),
        }
        if backend == "gloo" and (G > 1 or force_dist):
            out["backend"] = ("gloo: FUNCTIONAL multi-rank run -- %d ranks on %d GPU(s), box records exchanged through pinned host buffers; exercises the N > 1 "
                              "code path, not a scaling measurement" % (G, max(1, torch.cuda.device_count())))
            if args.full:
                out["exchange_check"] = exchange_ok
        if hip.LIB_OVERRIDE:
            out["lib_override"] = hip.LIB_OVERRIDE          # measured through YOLO_HIP_LIB (an A/B probe build), not the in-tree library
        if strong:
            out["config"]["per_rank"] = {"images_on_rank0": n_local}
        if args.full:      # the legs after the timed region that take runs of their own
            total_ms, conv_ms = eng.time_forward(n_local, 10, conv=True)
            # HBM bytes per forward of the conv launches: PMC counters cannot be read in-process, so this is the committed
            # rocprofv3 measurement (tools/profile_round.sh) -- printed only when it was taken on exactly this code and tile plan
            # (source hash), null otherwise: a stale number is never reported
            traffic = None
            from yolo_tensorflow_amd import buildinfo
            for tpath in sorted(__import__("glob").glob(os.path.join(ROOT, "profiles", "r*_hbm_traffic.json")), reverse=True):
                try:
                    tj = json.load(open(tpath))
                    if loaded and tj.get("source_hash") == buildinfo.source_hash(args.size, B, args.dtype):
                        traffic = tj["conv_hbm_bytes_per_forward"]; break
                except Exception:      # noqa: BLE001
                    pass
            flops = eng.conv_flops() * n_local
            achieved = flops / (conv_ms * 1e-3) / 1e12
            out["roofline"] = {"bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
                               "frac": round(achieved / peak, 4), "traffic": traffic,
                               "kernel": "conv_igemm_f32 (every conv launch of one forward)" if fp32 else "conv_igemm + conv_stem (every conv launch of one forward)", "flops_per_forward": flops,
                               "kernel_ms_per_forward": round(conv_ms, 4), "forward_ms": round(total_ms, 4)}
            if strong:      # a fixed global batch leaves each rank a small share: say which regime that share runs in, so a poor strong curve reads correctly
                out["config"]["per_rank"].update({"conv_frac_of_peak_on_rank0": round(achieved / peak, 4),
                                                  "regime": "launch-bound (per-launch fixed cost dominates: DESIGN.md section 6)" if achieved / peak < 0.25 else "matrix-pipe / fixed-cost mix"})
            if G == 1 and not args.no_latency:
                out.update(latency_b1(hip, cfg_txt, flat, args, dev, stream, fp8, fp32, fp16, x2, eng if B == 1 else None))
            if not args.no_calibration and not fp32:
                # the box's own yardstick, outside the timed region and AFTER the timed work (the chip is warm): what a register-resident MFMA loop
                # sustains here and at which clock -- `frac_of_calib` is what compares between boxes (the same binary reads 9 % apart by box)
                ct, cg = hip.calibrate(0.4, f16=fp16 or x2, device=local_rank, stream=stream.cuda_stream)
                mult = 2.0 if fp8 and not mixed else 1.0          # (the e4m3 MFMA runs at twice the 16-bit rate the loop measures)
                try:
                    cc = hip.calibrate_copy(0.2, device=local_rank, stream=stream.cuda_stream)
                except Exception:      # noqa: BLE001
                    cc = None
                out["roofline"].update({"calib_tflops": round(ct, 1), "clock_ghz": round(cg, 3), "calib_copy_gbs": round(cc, 0) if cc else None,
                                        "frac_of_calib": round(achieved / (ct * mult), 4) if ct > 0 and not mixed else None,
                                        "calib": "yolo_calibrate: register-resident v_mfma_f32_16x16x32 loop, 8 waves per CU, random operands, 0.4 s; clock = s_memtime / s_memrealtime; yolo_calibrate_copy: streaming 1 GiB -> 1 GiB device copy, GB/s read + written"})
            refs, imgs_par, t_or = None, None, 0.0
            if G == 1 and args.parity_images > 0:
                imgs_par = images[:min(args.parity_images, n_local)].cpu().numpy()
                t_or = time.time()
                refs = oracle_boxes(cfg_txt.replace("yolo_store=bf16\n", "").replace("yolo_store=fp8\n", "").replace("yolo_pair=0\n", "").replace("yolo_pair=1\n", "").replace("yolo_pair_input=0\n", ""), flat, imgs_par, args.size)
                t_or = time.time() - t_or
                out["parity"] = parity(eng, refs, imgs_par, t_oracle=t_or)
            if G == 1 and args.tolerance != "none" and args.dtype == "bf16" and not strong and not args.no_graph:
                base_txt = IO.cfg_text("yolov3") if args.size == 416 else IO.with_input_size(IO.cfg_text("yolov3"), args.size)
                try:
                    out["tolerance_line"] = tolerance_line(hip, IO, base_txt, flat, args, dev, stream, images, refs, imgs_par, args.tolerance)
                except Exception as e:      # noqa: BLE001 -- the headline line must not depend on the extra leg
                    out["tolerance_line"] = {"dtype": args.tolerance, "error": "%s: %s" % (type(e).__name__, e)}
            if G == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(cfg_txt, flat)
        print(json.dumps(out), flush=True)
    eng.close()
    if G > 1 or force_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
