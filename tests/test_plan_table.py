"""The planner's output, pinned: yolo_plan_table (no device) against tests/golden/plan_tables.json, which was recorded from the commit
BEFORE the per-layer (kernel, fused, launcher) fields replaced the eleven fusion booleans -- by a throw-away patch that printed the same
table from the booleans -- and is never regenerated from the code under test.

Per combination the fixture holds the planner's status and message when it refuses, else: the rows of the conv layers that are not
"tiled, own launch, no 1x1 tail"; around every fused group the rows whose `def` / `last` the group can move (the layer in front of its first
member and the members' folded shortcut sources); the final line; and the SHA-256 of the whole table, so every other row is pinned too.
Row lists that several combinations share (bf16 and fp16 plan alike, batch 1 and 32 differ in the byte total only) are stored once.
"""
import hashlib
import importlib.util
import json
import os

import pytest

from yolo_tensorflow_amd import hip, darknet_io as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_tables.json")
DTYPES = {"bf16": hip.BF16, "fp16": hip.FP16, "fp8": hip.FP8, "fp16x2": hip.FP16X2, "fp32": hip.FP32}
KNOBS = ("YOLO_NO_RESBLOCK", "YOLO_NO_HALO", "YOLO_NO_S2", "YOLO_NO_C3S2", "YOLO_NO_PAIR_STEM")


def cfg_texts(tmp_dir):
    """name -> text of every cfg the package ships, and of every cfg tools/make_cfgs.py generates (those, and yolo9000 with its seeded tree)."""
    spec = importlib.util.spec_from_file_location("make_cfgs", os.path.join(ROOT, "tools", "make_cfgs.py"))
    M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
    texts = {f[:-4]: IO.cfg_text(f[:-4]) for f in sorted(os.listdir(IO.CFG_DIR)) if f.endswith(".cfg")}
    tree = os.path.join(str(tmp_dir), "9k.tree")
    with open(tree, "w") as f:
        f.write(M.synthetic_tree())
    texts["yolo9000"] = M.yolo9000(tree=tree)
    return texts


def combinations(texts):
    """(key, cfg text, dtype, max_batch, keep_layers, environment knob or None)"""
    for name in sorted(texts):
        for dt in DTYPES:
            for keep in (0, 1):
                for mb in (1, 32):
                    yield "%s/%s/keep%d/b%d" % (name, dt, keep, mb), texts[name], DTYPES[dt], mb, keep, None
    for knob in KNOBS:
        yield "yolov3/bf16/keep0/b32/%s" % knob, texts["yolov3"], hip.BF16, 32, 0, knob
    # (the pair stem exists in split-fp16 networks only: its knob once more where it changes the plan)
    yield "yolov3/fp16x2/keep0/b32/YOLO_NO_PAIR_STEM", texts["yolov3"], hip.FP16X2, 32, 0, "YOLO_NO_PAIR_STEM"


def digest(rc, text):
    """What the fixture keeps of one call's (status, table or message)."""
    if rc != 0:
        return {"rc": rc, "err": text}
    lines = text.splitlines()
    rows, final = [ln.split() for ln in lines[:-1]], lines[-1]
    field = lambda row, k: next(v.split("=", 1)[1] for v in row if v.startswith(k + "="))
    keep = set()
    for i, row in enumerate(rows):
        if field(row, "kernel") == "-":          # not a conv
            continue
        if (field(row, "kernel"), field(row, "fused"), field(row, "tail_layer")) != ("tiled", "none", "-1"):
            keep.add(i)
        if field(row, "fused") != "none":
            first = min(j for j, r in enumerate(rows) if field(r, "fused") == field(row, "fused") and field(r, "launcher") == field(row, "launcher"))
            keep.update(j for j in (first - 1, int(field(row, "residual_from"))) if j >= 0)
    return {"rc": 0, "rows": [lines[i] for i in sorted(keep)], "final": final, "sha256": hashlib.sha256(text.encode()).hexdigest()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        fx = json.load(f)
    return {k: dict(v, rows=fx["rows"][v["rows"]]) if v["rc"] == 0 else v for k, v in fx["combos"].items()}


def test_fixture_covers_every_combination(recorded, tmp_path):
    assert sorted(recorded) == sorted(k for k, *_ in combinations(cfg_texts(tmp_path)))
    assert any(v["rc"] == 0 and any("fused=c3s2" in r for r in v["rows"]) for v in recorded.values())
    assert any(v["rc"] == 0 and any("fused=pair-stem" in r for r in v["rows"]) for v in recorded.values())
    assert recorded["yolov3/fp16x2/keep0/b32/YOLO_NO_PAIR_STEM"]["sha256"] != recorded["yolov3/fp16x2/keep0/b32"]["sha256"]


def test_plan_tables_equal_the_recorded_parent(recorded, tmp_path, monkeypatch):
    for knob in KNOBS:
        monkeypatch.delenv(knob, raising=False)
    bad = []
    for key, text, dtype, mb, keep, knob in combinations(cfg_texts(tmp_path)):
        if knob:
            monkeypatch.setenv(knob, "1")
        got = digest(*hip.plan_table(text, dtype, mb, keep))
        if knob:
            monkeypatch.delenv(knob)
        if got != recorded[key]:
            bad.append((key, got, recorded[key]))
    assert not bad, "%d plans differ from the recorded ones; first: %r" % (len(bad), bad[0])


def test_table_shape_and_small_buffer():
    rc, text = hip.plan_table(IO.cfg_text("yolov3"), hip.BF16, 32, False)
    assert rc == 0
    lines = text.splitlines()
    assert len(lines) == 107 + 1 and lines[-1].startswith("buffers ")
    assert lines[1].split()[:5] == ["1", "convolutional", "kernel=tiled", "fused=stem", "launcher=1"]
    import ctypes as C
    out, err = C.create_string_buffer(64), C.create_string_buffer(256)
    rc = hip.load_library().yolo_plan_table(IO.cfg_text("yolov3").encode(), hip.BF16, 32, 0, out, 64, err, 256)
    assert rc != 0 and out.value == b"" and ("needs %d bytes" % (len(text) + 1)) in err.value.decode()
    assert hip.plan_table(IO.cfg_text("yolov3"), hip.BF16, 0, False)[1] == "max_batch < 1"
