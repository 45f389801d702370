"""bench.py's plain line and --dump-outputs on the device: a plain run prints the headline fields without the legs of --full, and
the records it dumps for the last timed step are what the engine's own detect returns on the same seeded inputs.  The benchmark
runs in a child process started before it touches the GPU, so this process's current stream is left as it was."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_line_and_dump_outputs(hiplib, tmp_path):
    # 416 x 416 at batch 2 has no committed tile plan: --no-tune runs the library's built-in plan, the one a fresh Engine uses
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "2", "--no-tune",
           "--dump-outputs", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["metric"] == "images_per_sec" and out["unit"] == "img/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) / out["value"] < 0.01
    assert not {"roofline", "parity", "tolerance_line", "cpu_baseline", "latency_b1_ms"} & set(out)
    got = {n: np.load(str(tmp_path / "out" / (n + ".npy"))) for n in ("boxes", "scores", "classes", "counts")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["boxes"].shape == (2, 20, 4) and got["scores"].shape == got["classes"].shape == (2, 20) and got["counts"].shape == (2,)

    txt = IO.cfg_text("yolov3")
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=0)
    img = np.random.default_rng(1).integers(0, 256, (2, 416, 416, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.BF16, semantics=hiplib.SEM_TF, decode=hiplib.DECODE_RATIO)
    eng.set_weights(flat)
    want = eng.detect(img, score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=hiplib.NMS_TF, select_mode=hiplib.SELECT_GT)
    eng.close()
    assert [int(c) for c in got["counts"]] == [len(w) for w in want] and sum(len(w) for w in want) > 0
    for b, w in enumerate(want):
        n = len(w)
        assert np.array_equal(got["boxes"][b, :n], np.stack([w["x0"], w["y0"], w["x1"], w["y1"]], -1))
        assert np.array_equal(got["scores"][b, :n], w["score"]) and np.array_equal(got["classes"][b, :n], w["cls"].astype(np.float32))
        assert not got["boxes"][b, n:].any() and not got["scores"][b, n:].any() and (got["classes"][b, n:] == -1).all()
