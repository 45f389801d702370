"""Softmax trees without a GPU: the two tree readers against the reference's read_tree, the refusals, and the planner.

The first part of this file is shared with tests/test_gpu_tree.py: the seeded synthetic trees, and the reference's own tree code
(oracle/_ref: `read_tree`, `softmax_cpu`, `hierarchy_predictions`, `hierarchy_top_prediction`) bound through a ctypes mirror of its
`tree` struct (include/darknet.h:42-53)."""
import ctypes as C
import os
import re
import sys
import numpy as np
import pytest
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import darknet_io as IO, hip


class TREE(C.Structure):
    _fields_ = [("leaf", C.POINTER(C.c_int)), ("n", C.c_int), ("parent", C.POINTER(C.c_int)), ("child", C.POINTER(C.c_int)),
                ("group", C.POINTER(C.c_int)), ("name", C.POINTER(C.c_char_p)), ("groups", C.c_int),
                ("group_size", C.POINTER(C.c_int)), ("group_offset", C.POINTER(C.c_int))]


def tree_text(nodes, root, special, seed):
    """A seeded tree file of exactly `nodes` nodes: a root group of `root`, then runs of children appended breadth-first.  `special`:
    group sizes that must occur (each is hung under the LAST node of the group in front of it, so a parent that ends its own group
    is covered); the rest are small random runs.  Depth >= 4 by construction: every special run hangs one level below the one
    before it."""
    rng = np.random.default_rng(seed)
    parent = [-1] * root
    tip = root - 1                                     # last node of the newest group
    for k in special:
        parent += [tip] * k
        tip = len(parent) - 1
    free = [i for i in range(len(parent)) if i not in set(parent)]      # nodes without children yet, ascending
    while len(parent) < nodes:
        p = free.pop(int(rng.integers(0, min(len(free), 6))))
        k = int(min(nodes - len(parent), rng.integers(1, 9)))
        free += list(range(len(parent), len(parent) + k))
        parent += [p] * k
    return "".join("n%04d %d\n" % (i, q) for i, q in enumerate(parent))


def tree_a(path):
    """240 nodes: root group of 6, depth >= 4, one group of 1, one of 70 (past one wave), one of 3 whose parent is the last node of
    its own group."""
    open(path, "w").write(tree_text(240, 6, (3, 1, 70, 3), seed=11))
    return str(path)


def tree_b(path):
    """1200 nodes with one group of 700 (past one 256-thread pass, past ten waves)."""
    open(path, "w").write(tree_text(1200, 5, (4, 700, 2), seed=12))
    return str(path)


def ref_lib():
    l = DR.lib()
    l.read_tree.argtypes = [C.c_char_p]; l.read_tree.restype = C.POINTER(TREE)
    FP = C.POINTER(C.c_float)
    l.softmax_cpu.argtypes = [FP, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, FP]; l.softmax_cpu.restype = None
    l.hierarchy_predictions.argtypes = [FP, C.c_int, C.POINTER(TREE), C.c_int, C.c_int]; l.hierarchy_predictions.restype = None
    l.hierarchy_top_prediction.argtypes = [FP, C.POINTER(TREE), C.c_float, C.c_int]; l.hierarchy_top_prediction.restype = C.c_int
    return l


class RefTree:
    def __init__(self, path):
        self.l = ref_lib()
        self.t = self.l.read_tree(str(path).encode())
        t = self.t.contents
        self.n, self.groups = t.n, t.groups
        arr = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).astype(np.int32).copy()
        self.parent, self.child, self.leaf = arr(t.parent, t.n), arr(t.child, t.n), arr(t.leaf, t.n)
        self.group_offset, self.group_size = arr(t.group_offset, t.groups), arr(t.group_size, t.groups)

    def conditional(self, x, temp):
        """softmax_cpu per group (as DN/softmax_layer.c:41-48 / DN/region_layer.c:177-181 call it) over rows x [n, nodes]."""
        x = np.ascontiguousarray(x, dtype=np.float32); out = np.zeros_like(x)
        FP = C.POINTER(C.c_float)
        for r in range(x.shape[0]):
            for off, sz in zip(self.group_offset, self.group_size):
                self.l.softmax_cpu(x[r, off:].ctypes.data_as(FP), int(sz), 1, 0, 1, 0, 1, C.c_float(temp), out[r, off:].ctypes.data_as(FP))
        return out

    def absolute(self, cond, only_leaves=0):
        a = np.ascontiguousarray(cond, dtype=np.float32).copy()
        for r in range(a.shape[0]):
            self.l.hierarchy_predictions(a[r].ctypes.data_as(C.POINTER(C.c_float)), self.n, self.t, only_leaves, 1)
        return a

    def top(self, absolute, thresh):
        a = np.ascontiguousarray(absolute, dtype=np.float32)
        return np.array([self.l.hierarchy_top_prediction(a[r].ctypes.data_as(C.POINTER(C.c_float)), self.t, C.c_float(thresh), 1)
                         for r in range(a.shape[0])], dtype=np.int32)

    def abs64(self, x):
        """float64 absolute probabilities of rows x [n, nodes] of raw logits (temperature 1)"""
        x = np.asarray(x, dtype=np.float64)
        a = np.zeros_like(x)
        for off, sz in zip(self.group_offset, self.group_size):
            e = np.exp(x[:, off:off + sz] - x[:, off:off + sz].max(axis=1, keepdims=True)); a[:, off:off + sz] = e / e.sum(axis=1, keepdims=True)
        for j in range(self.n):
            if self.parent[j] >= 0:
                a[:, j] *= a[:, self.parent[j]]
        return a

    def walk64(self, a, thresh, eps=1e-5, trace=False):
        """hierarchy_top_prediction in float64 over one row of abs64 -> (label, ambiguous): ambiguous when, on the path, the two
        best values of a group lie within `eps` relative of each other or p * max within `eps` of the threshold -- the rows the
        tests may leave out.  trace: -> (label, ambiguous, exit, groups) with exit one of "root" (the test failed at group 0),
        "deeper" (it failed below: the parent of the group's first node) or "leaf", and the groups visited."""
        p, group, amb, seen = 1.0, 0, False, []
        while True:
            seen.append(group)
            off, sz = int(self.group_offset[group]), int(self.group_size[group])
            v = a[off:off + sz]
            i = int(np.argmax(v)); mx = float(v[i]) if v[i] > 0 else 0.0
            mi = off + i if v[i] > 0 else 0
            if sz > 1:
                second = float(np.partition(v, -2)[-2])
                amb |= abs(mx - second) <= eps * max(abs(mx), 1e-300)
            amb |= abs(p * mx - thresh) <= eps
            if p * mx > thresh:
                p *= mx; group = int(self.child[mi])
                if group < 0:
                    return (mi, amb, "leaf", seen) if trace else (mi, amb)
            elif group == 0:
                return (mi, amb, "root", seen) if trace else (mi, amb)
            else:
                j = int(self.parent[off])
                return (j, amb, "deeper", seen) if trace else (j, amb)


TF = sys.modules[__name__]

ARRAYS = ("parent", "child", "group_offset", "group_size", "leaf")

CLS_CFG = """[net]
batch=1
height=32
width=32
channels=3

[convolutional]
batch_normalize=1
filters=8
size=3
stride=2
pad=1
activation=leaky

[convolutional]
filters=240
size=1
stride=1
pad=1
activation=linear

[avgpool]

[softmax]
groups=1
"""


@pytest.mark.parametrize("make", [TF.tree_a, TF.tree_b])
def test_readers_equal_the_reference(tmp_path, make):
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    path = make(tmp_path / "t.tree")
    ref = TF.RefTree(path)
    py, lib = IO.read_tree(path), hip.tree_read(path)
    assert ref.n == py["n"] == lib["n"] and ref.groups == py["groups"] == lib["groups"]
    for k in ARRAYS:
        assert np.array_equal(getattr(ref, k), py[k]), k
        assert np.array_equal(getattr(ref, k), lib[k]), k


def test_trees_have_the_shapes_the_kernels_must_survive(tmp_path):
    a, b = IO.read_tree(TF.tree_a(tmp_path / "a.tree")), IO.read_tree(TF.tree_b(tmp_path / "b.tree"))
    assert a["n"] == 240 and a["group_size"][0] == 6 and 1 in a["group_size"] and 70 in a["group_size"]
    g3 = [g for g in range(1, a["groups"]) if a["group_size"][g] == 3 and
          a["parent"][a["group_offset"][g]] == a["group_offset"][a["group"][a["parent"][a["group_offset"][g]]]] + a["group_size"][a["group"][a["parent"][a["group_offset"][g]]]] - 1]
    assert g3, "a group of 3 whose parent ends its own group"
    depth = np.zeros(a["n"], int)
    for j in range(a["n"]):
        depth[j] = 0 if a["parent"][j] < 0 else depth[a["parent"][j]] + 1
    assert depth.max() >= 4
    assert b["n"] == 1200 and 700 in b["group_size"]


BAD = [
    ("a 0\nb -1\n", "line 1.*root"),
    ("a -1\nb -1\nc 2\n", "line 3.*below"),
    ("a -1\nb -1\nc 0\nd 1\ne 0\n", "line 5.*contiguous"),
    ("a -1\nb 0\nc -1\n", "line 3.*contiguous"),
]


@pytest.mark.parametrize("text,msg", BAD)
def test_malformed_trees_are_refused_with_the_line(tmp_path, text, msg):
    path = str(tmp_path / "bad.tree")
    open(path, "w").write(text)
    with pytest.raises(hip.YoloError, match=msg):
        hip.tree_read(path)
    with pytest.raises(ValueError, match=msg):
        IO.read_tree(path)
    rc, err = hip.plan_check(CLS_CFG.replace("groups=1", "tree=%s" % path))
    assert rc == -1 and re.search(msg, err), err


def test_missing_file_is_refused(tmp_path):
    path = str(tmp_path / "nope.tree")
    with pytest.raises(hip.YoloError, match="cannot be opened"):
        hip.tree_read(path)
    with pytest.raises(ValueError, match="cannot be opened"):
        IO.read_tree(path)
    rc, err = hip.plan_check(CLS_CFG.replace("groups=1", "tree=%s" % path))
    assert rc == -1 and "cannot be opened" in err


def _region_cfg(tree, classes=240, extra=""):
    return ("[net]\nbatch=1\nheight=96\nwidth=96\nchannels=3\n\n[convolutional]\nbatch_normalize=1\nfilters=16\nsize=3\nstride=2\npad=1\nactivation=leaky\n\n"
            "[convolutional]\nfilters=%d\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[region]\nanchors=1,1, 2,2\nclasses=%d\ncoords=4\nnum=2\nsoftmax=1\ntree=%s\n%s"
            % (2 * (5 + classes), classes, tree, extra))


def test_softmax_and_region_trees_plan(tmp_path):
    """`tree=` on [softmax] was refused as UNSUPPORTED before this feature; on [region] it was silently served as a flat softmax."""
    a = TF.tree_a(tmp_path / "a.tree")
    rc, err = hip.plan_check(CLS_CFG.replace("groups=1", "tree=%s\ntemperature=2" % a))
    assert rc == 0, err
    rc, err = hip.plan_check(_region_cfg(a))
    assert rc == 0, err
    secs = IO.parse_cfg(_region_cfg(a))
    assert secs[-1]["tree"] == a


def test_size_and_option_refusals(tmp_path):
    a = TF.tree_a(tmp_path / "a.tree")
    rc, err = hip.plan_check(CLS_CFG.replace("filters=240", "filters=200").replace("groups=1", "tree=%s" % a))
    assert rc == -1 and "240 nodes" in err and "200 inputs" in err
    rc, err = hip.plan_check(_region_cfg(a, classes=100))
    assert rc == -1 and "240 nodes" in err and "100 classes" in err
    for extra, word in (("background=1\n", "background"), ("map=coco9k.map\n", "map")):
        rc, err = hip.plan_check(_region_cfg(a, extra=extra))
        assert rc == -6 and word in err, (rc, err)
    rc, err = hip.plan_check(_region_cfg(a).replace("coords=4", "coords=6"))
    assert rc == -6 and "coords" in err, (rc, err)
    rc, err = hip.plan_check(CLS_CFG.replace("groups=1", "tree=%s\nspatial=1" % a))
    assert rc == -6 and "spatial" in err
    rc, err = hip.plan_check(CLS_CFG.replace("groups=1", "tree=%s" % a), dtype=hip.FP8)
    assert rc == -6 and "fp8" in err
    for dt in (hip.BF16, hip.FP16, hip.FP16X2, hip.FP32):
        assert hip.plan_check(_region_cfg(a), dtype=dt)[0] == 0


def test_generated_yolo9000_plans(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_cfgs", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "make_cfgs.py"))
    M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
    tree = str(tmp_path / "9k.tree")
    open(tree, "w").write(M.synthetic_tree())
    t = IO.read_tree(tree)
    assert t["n"] == 9418 and t["group_size"].max() > 64
    assert M.synthetic_tree() == open(tree).read()          # seeded
    rc, err = hip.plan_check(M.yolo9000(tree=tree))
    assert rc == 0, err
