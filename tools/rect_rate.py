"""What a 16:9 network input costs against the square one: the detect step of YOLOv3, bf16, batch 32, at 608 x 608 and at 352 high x 608
wide, on one build, one process.

Both contexts run the library's default tile plan: there is no tuned plan for either shape at batch 32 (yolo_tensorflow_amd/tuned/ holds
608 at batch 8 only), and a plan tuned for a square size says nothing about the rectangular one.  The step is bench.py's headline form: a
device-resident uint8 batch, yolo_detect_graph (forward + lean decode + threshold + NMS replayed from one graph).  The two shapes run
in alternating rounds on one created stream, timed with events (median step per round, median over rounds).

  python tools/rect_rate.py [--steps 50] [--warmup 10] [--rounds 5] [--batch 32]

Prints one JSON line.  352 x 608 has 352 / 608 = 57.9 % of the pixels, and so of the conv work, of 608 x 608; nothing fixes the time ratio in
advance."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((608, 608), (352, 608))          # height, width


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()

    import torch
    from yolo_tensorflow_amd import hip, darknet_io as IO

    B, max_out = args.batch, 20
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    post = dict(score_thr=0.5, iou_thr=0.5, max_out=max_out, nms_mode=hip.NMS_TF, select_mode=hip.SELECT_GT)
    rng = np.random.default_rng(1)
    steps, flops, rows = [], [], []
    for hw in SHAPES:
        txt = IO.with_input_size(IO.cfg_text("yolov3"), hw)
        eng = hip.Engine(txt, max_batch=B, dtype=hip.BF16, semantics=hip.SEM_TF, decode=hip.DECODE_RATIO, device=0, stream=stream.cuda_stream)
        eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
        assert eng.input_hw == hw
        img = torch.from_numpy(rng.integers(0, 256, (B, hw[0], hw[1], 3), dtype=np.uint8)).to(dev)
        boxes = torch.zeros(B * max_out * 6, dtype=torch.int32, device=dev); counts = torch.zeros(B, dtype=torch.int32, device=dev)
        steps.append((eng, lambda e=eng, i=img, b=boxes, c=counts: e.detect_graph(i, b, c, **post)))
        flops.append(eng.conv_flops()); rows.append(eng.rows)

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

    times = [[], []]
    for _ in range(args.rounds):
        for k in range(2):
            times[k].append(timed(steps[k][1]))
    med = [float(np.median(t)) for t in times]
    out = {
        "workload": "yolov3 bf16 batch %d detect graph step, library-default tile plan: 608 x 608 against 352 high x 608 wide" % B,
        "tile_plan": "built-in (both shapes)",
        "square_step_ms": med[0], "rect_step_ms": med[1],
        "square_rounds_ms": times[0], "rect_rounds_ms": times[1],
        "rect_over_square_time": med[1] / med[0],
        "rect_over_square_conv_flops": flops[1] / flops[0],
        "square_img_per_s": B / (med[0] / 1e3), "rect_img_per_s": B / (med[1] / 1e3),
        "rows_per_image": {"square": rows[0], "rect": rows[1]},
    }
    for eng, _ in steps:
        eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
