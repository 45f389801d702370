"""yolo_plan_dump (every field the planner writes, no device) of one combination, or the fixture tests/test_plan_dump.py compares against.

    python tools/plan_dump.py --show yolov3/bf16/keep0/b32      # one combination's dump (or its refusal)
    python tools/plan_dump.py --list                            # the keys
    python tools/plan_dump.py --record                          # write tests/golden/plan_dumps.json

The fixture is recorded from the commit BEFORE a change to the planner, with the library built there, never from the code under test.
"""
import argparse
import glob
import hashlib
import importlib.util
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yolo_tensorflow_amd import hip, darknet_io as IO  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_dumps.json")
# cfgs added after the fixture was recorded whose plans the recording commit could not form (it refused dense convs of a size other than 1 and
# 3): nothing recorded there could pin them, tests/test_wide_host.py pins their geometry instead
# ... and [rnn] / [gru] / [lstm] / [crnn] sections, which it refused too: tests/test_recurrent_host.py pins what their plans hold
# ... and [crop] / [normalization] sections, likewise: tests/test_lrn_crop_host.py
# ... and a vector-input network ([net] yolo_input=vector), which it refused for its missing image size: tests/test_char_rnn_host.py
# ... and image networks of a channel count other than three ([net] yolo_input=planes), which it refused for their channels=: tests/test_planes_host.py
# ... and [convolutional] sections with xnor=1, a key it read nowhere (it planned them as dense convs): tests/test_xnor_host.py pins their L_XCONV rows and refusals
UNPINNED = ("zoo/alexnet", "golden/mini_wide", "golden/mini_seq", "golden/mini_crnn", "zoo/alexnet-lrn", "golden/mini_lrn", "golden/mini_char_rnn",
            "golden/mini_planes_grey", "golden/mini_planes_rgbd", "golden/mini_planes_nine", "golden/mini_planes_17", "golden/mini_xnor", "golden/xnor_layer_cases")
PLANNER_RC = (0, -1, -6)          # YOLO_OK, YOLO_ERR_INVALID, YOLO_ERR_UNSUPPORTED: all build_plan returns for a cfg whose tree file opens


def _table_module():
    spec = importlib.util.spec_from_file_location("test_plan_table", os.path.join(ROOT, "tests", "test_plan_table.py"))
    T = importlib.util.module_from_spec(spec); spec.loader.exec_module(T)
    return T


def combinations(tmp_dir):
    """(key, cfg text, dtype, max_batch, keep_layers, environment knob or None): what tests/test_plan_table.py enumerates, then cfg/zoo/
    the same way, the cfg of every tests/golden/*.npz that has one at batch 1, and YOLO_NO_POOL_FUSE on darknet19 (whose plan it changes) and darknet53."""
    T = _table_module()
    texts = T.cfg_texts(tmp_dir)
    yield from T.combinations(texts)
    zoo = {"zoo/" + os.path.basename(p)[:-4]: open(p).read() for p in sorted(glob.glob(os.path.join(IO.CFG_DIR, "zoo", "*.cfg")))}
    for name in sorted(zoo):
        if name in UNPINNED:
            continue
        for dt in T.DTYPES:
            for keep in (0, 1):
                for mb in (1, 32):
                    yield "%s/%s/keep%d/b%d" % (name, dt, keep, mb), zoo[name], T.DTYPES[dt], mb, keep, None
    for p in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz"))):
        with np.load(p, allow_pickle=False) as z:
            if "cfg" not in z.files:
                continue
            text = str(z["cfg"])
        if "golden/" + os.path.basename(p)[:-4] in UNPINNED:
            continue
        for dt in T.DTYPES:
            for keep in (0, 1):
                yield "golden/%s/%s/keep%d/b1" % (os.path.basename(p)[:-4], dt, keep), text, T.DTYPES[dt], 1, keep, None
    for name in ("darknet19", "darknet53"):
        yield "%s/bf16/keep0/b1/YOLO_NO_POOL_FUSE" % name, texts[name], hip.BF16, 1, 0, "YOLO_NO_POOL_FUSE"


def dump(text, dtype, mb, keep, knob):
    """(status, dump or message) of one combination, with `knob` (and no other planner knob) in the environment."""
    T = _table_module()
    saved = {k: os.environ.pop(k, None) for k in T.KNOBS + ("YOLO_NO_POOL_FUSE",)}
    try:
        if knob:
            os.environ[knob] = "1"
        return hip.plan_dump(text, dtype, mb, keep)
    finally:
        os.environ.pop(knob or "", None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})


def digest(rc, text):
    return {"rc": rc, "err": text} if rc else {"rc": 0, "sha256": hashlib.sha256(text.encode()).hexdigest()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--show", metavar="KEY"); g.add_argument("--list", action="store_true"); g.add_argument("--record", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        combos = list(combinations(tmp))
        if a.list:
            print("\n".join(k for k, *_ in combos))
        elif a.show:
            found = [c for c in combos if c[0] == a.show]
            if not found:
                sys.exit("no combination %r (see --list)" % a.show)
            rc, text = dump(*found[0][1:])
            print(text if rc == 0 else "refused (%d): %s" % (rc, text))
        else:
            fx = {key: digest(*dump(*rest)) for key, *rest in combos}
            assert len(fx) == len(combos), "two combinations share a key"
            strange = {k: v["rc"] for k, v in fx.items() if v["rc"] not in PLANNER_RC}
            assert not strange, "statuses the planner does not return: %r" % strange
            with open(FIXTURE, "w") as f:
                json.dump(fx, f, indent=0, sort_keys=True)
                f.write("\n")
            print("%d combinations (%d refusals) -> %s" % (len(fx), sum(v["rc"] != 0 for v in fx.values()), os.path.relpath(FIXTURE, ROOT)))


if __name__ == "__main__":
    main()
