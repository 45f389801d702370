"""Everything the planner writes, pinned: yolo_plan_dump (no device) against tests/golden/plan_dumps.json, which tools/plan_dump.py --record
wrote from the commit BEFORE build_plan was taken apart into passes, with only the dump entry point added to it, and which is never
regenerated from the code under test.  Per combination the fixture holds the planner's status and message when it refuses, else the SHA-256
of the dump: every layer's fields, every storage's, the context's (tests/test_plan_table.py pins the eleven fields of its table).

The combinations (tools/plan_dump.py): those of test_plan_table.py, cfg/zoo/, the cfg of every tests/golden/*.npz that has one, and
YOLO_NO_POOL_FUSE on darknet19 (whose plan it changes) and darknet53.
"""
import importlib.util
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("plan_dump", os.path.join(ROOT, "tools", "plan_dump.py"))
P = importlib.util.module_from_spec(spec); spec.loader.exec_module(P)

# what at least one pinned plan must exercise: a pattern of the dump's text (LType 12: [deconvolutional], 15: grouped [convolutional])
FEATURES = {"pool_fused": r" pool_fused=1 ", "inplace": r" inplace=1 ", "copy_inputs": r" copy_inputs=\[\d", "general": r" general=1 ",
            "L_DECONV": r" deconvolutional type=12 ", "L_GCONV": r" convolutional type=15 "}


@pytest.fixture(scope="module")
def recorded():
    with open(P.FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """key -> (status, dump or message) of every combination, planned once"""
    return {key: P.dump(*rest) for key, *rest in P.combinations(tmp_path_factory.mktemp("trees"))}


def test_fixture_covers_every_combination(recorded, planned):
    assert sorted(recorded) == sorted(planned)
    assert all(v["rc"] in P.PLANNER_RC for v in recorded.values())
    assert all(set(v) == ({"rc", "err"} if v["rc"] else {"rc", "sha256"}) for v in recorded.values())
    assert any(v["rc"] != 0 for v in recorded.values())
    # (darknet53's [avgpool] is followed by a [connected] layer, not by the [softmax]: nothing for the knob to change there)
    assert recorded["darknet19/bf16/keep0/b1/YOLO_NO_POOL_FUSE"] != recorded["darknet19/bf16/keep0/b1"]
    assert recorded["darknet53/bf16/keep0/b1/YOLO_NO_POOL_FUSE"] == recorded["darknet53/bf16/keep0/b1"]


def test_plan_dumps_equal_the_recorded_parent(recorded, planned):
    bad = [(key, P.digest(*got), recorded[key]) for key, got in planned.items() if P.digest(*got) != recorded[key]]
    assert not bad, "%d plans differ from the recorded ones (tools/plan_dump.py --show KEY prints one); first: %r" % (len(bad), bad[0])


@pytest.mark.parametrize("feature", sorted(FEATURES))
def test_a_pinned_plan_exercises(feature, recorded, planned):
    """... among the plans whose dump IS the recorded one"""
    pinned = (text for key, (rc, text) in planned.items() if rc == 0 and P.digest(rc, text) == recorded[key])
    assert any(re.search(FEATURES[feature], text) for text in pinned)


def test_dump_shape_and_small_buffer():
    from yolo_tensorflow_amd import hip, darknet_io as IO
    rc, text = hip.plan_dump(IO.cfg_text("yolov3"), hip.BF16, 32, False)
    assert rc == 0
    lines = text.splitlines()
    assert sum(ln.startswith("layer ") for ln in lines) == 107 and lines[-1].startswith("context in_h=416 in_w=416 ")
    assert sum(ln.startswith("storage ") for ln in lines) == len(lines) - 108
    import ctypes as C
    out, err = C.create_string_buffer(64), C.create_string_buffer(256)
    rc = hip.load_library().yolo_plan_dump(IO.cfg_text("yolov3").encode(), hip.BF16, 32, 0, out, 64, err, 256)
    assert rc != 0 and out.value == b"" and ("needs %d bytes" % (len(text) + 1)) in err.value.decode()
    assert hip.plan_dump(IO.cfg_text("yolov3"), hip.BF16, 0, False)[1] == "max_batch < 1"
