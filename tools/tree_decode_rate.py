#!/usr/bin/env python3
"""Rate of the two decode forms of a softmax-tree head on the generated YOLO9000 shape: 17 x 17 x 3 boxes, 9418 classes.

The descent form (YOLO_TREE_DESCENT=1: one wave per kept box walks the tree over the raw logits) against the full form
(YOLO_TREE_FULL=1: the decoded tensor with every absolute probability, then the walk over it).  Each form runs in a process of its
own (the switch is read when the context is created): warm-up, then the median of `--steps` timed yolo_detect_graph steps on
device-resident images, stream-synchronised.  Prints one JSON line.

  python tools/tree_decode_rate.py [--batch 8] [--steps 30] [--warmup 5] [--thresh 0.5]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child(a):
    import numpy as np
    import torch
    torch.cuda.init()
    import make_cfgs as M
    from yolo_tensorflow_amd import hip, darknet_io as IO
    os.chdir(a.dir)
    txt = M.yolo9000()
    eng = hip.Engine(txt, max_batch=a.batch, dtype=hip.BF16, semantics=hip.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0, obj_bias=0.0))
    img = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (a.batch, 544, 544, 3), dtype=np.uint8)).cuda()
    boxes = torch.zeros(a.batch * 20 * 24, dtype=torch.uint8, device="cuda"); counts = torch.zeros(a.batch, dtype=torch.int32, device="cuda")
    kw = dict(score_thr=a.thresh, iou_thr=0.45, max_out=20, nms_mode=hip.NMS_DARKNET, hier_thresh=0.5)
    for _ in range(a.warmup + 2):
        eng.detect_graph(img, boxes, counts, **kw)
    eng.synchronize()
    ts = []
    for _ in range(a.steps):
        t = time.perf_counter(); eng.detect_graph(img, boxes, counts, **kw); eng.synchronize(); ts.append(time.perf_counter() - t)
    recs = boxes.cpu().numpy().view(hip.BOX_DTYPE).reshape(a.batch, 20); cn = counts.cpu().numpy()
    kept = None
    if a.count:
        det = eng.forward(img.cpu().numpy())
        kept = int((det[:, :, 4] >= a.thresh).sum())
    ms = sorted(ts)[len(ts) // 2] * 1e3
    print(json.dumps({"step_ms_median": round(ms, 4), "step_ms_min": round(min(ts) * 1e3, 4), "kept_boxes": kept, "records": int(cn.sum()),
                      "labels": [int(v) for b in range(a.batch) for v in recs[b, :cn[b]]["cls"]]}))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8); ap.add_argument("--steps", type=int, default=30); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--thresh", type=float, default=0.5); ap.add_argument("--dir"); ap.add_argument("--count", type=int, default=0)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    import make_cfgs as M
    d = tempfile.mkdtemp(prefix="yolo9000_")
    with open(os.path.join(d, "9k.tree"), "w") as f:
        f.write(M.synthetic_tree())
    out = {}
    for form, full in (("descent", False), ("full", True)):
        env = dict(os.environ)
        env.pop("YOLO_TREE_FULL", None); env.pop("YOLO_TREE_DESCENT", None)
        env["YOLO_TREE_FULL" if full else "YOLO_TREE_DESCENT"] = "1"
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--dir", d, "--batch", str(a.batch), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--thresh", str(a.thresh), "--count", "1" if full else "0"]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stderr); raise SystemExit("%s form failed (%d)" % (form, r.returncode))
        out[form] = json.loads(r.stdout.strip().splitlines()[-1])
    same = out["descent"].pop("labels") == out["full"].pop("labels")
    print(json.dumps({"shape": "yolo9000 17x17x3 boxes, 9418 classes, batch %d, bf16, synthetic weights" % a.batch, "score_thr": a.thresh,
                      "descent": out["descent"], "full": out["full"], "kept_boxes": out["full"]["kept_boxes"], "same_labels": same}))


if __name__ == "__main__":
    main()
