"""Multi-view classification, host side: yolo_view_table against the literal tables, the fixture tests/golden/views_cases.npz against a float32 numpy
restatement of the view pixel rule (include/yolo_hip.h) and -- where oracle/_ref is built -- against a fresh ctypes composition of the compiled
reference's own functions in validate_classifier_10's order, and the argument checks that need no device."""
import ctypes
import importlib.util
import os
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def views_module():
    """tools/make_views_golden.py: the cfgs, the case list, the numpy restatement and the ctypes composition the fixture was written with"""
    spec = importlib.util.spec_from_file_location("make_views_golden", os.path.join(ROOT, "tools", "make_views_golden.py"))
    M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
    return M


V = views_module()
CASES = [c[0] for c in V.CASES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_view_table_states_the_literal_tables():
    flip = hip.view_table(hip.VIEWS_FLIP)
    assert [tuple(int(x) for x in v) for v in flip] == [(0, 0, 0, 0), (0, 0, 1, 0)]
    for s in (32, 5, 0, 1):
        ten = hip.view_table(hip.VIEWS_TEN_CROP, s)
        # (dy, dx, flip, pad): the reference's (dx, dy) list (-s,-s), (s,-s), (0,0), (-s,s), (s,s), then the same on the mirrored image
        want = [(-s, -s, 0, 0), (-s, s, 0, 0), (0, 0, 0, 0), (s, -s, 0, 0), (s, s, 0, 0)]
        want = want + [(dy, dx, 1, 0) for dy, dx, _, _ in want]
        assert [tuple(int(x) for x in v) for v in ten] == want, s
    assert hip.VIEW_DTYPE.itemsize == 16


def test_view_table_count_cap_and_refusals():
    lib = hip.load_library()
    n = ctypes.c_int(-5)
    assert lib.yolo_view_table(hip.VIEWS_TEN_CROP, 32, None, 0, ctypes.byref(n)) == 0 and n.value == 10
    out = np.full(3, 77, dtype=hip.VIEW_DTYPE)
    assert lib.yolo_view_table(hip.VIEWS_TEN_CROP, 4, out.ctypes.data, 2, ctypes.byref(n)) == 0 and n.value == 10
    assert tuple(out[1]) == (-4, 4, 0, 0) and tuple(out[2]) == (77, 77, 77, 77)          # cap is respected
    for views, shift in ((0, 32), (3, 32), (-1, 0), (hip.VIEWS_TEN_CROP, -1), (hip.VIEWS_FLIP, -1)):
        n.value = 9
        assert lib.yolo_view_table(views, shift, out.ctypes.data, 3, ctypes.byref(n)) == INVALID and n.value == 0, (views, shift)
    assert lib.yolo_view_table(hip.VIEWS_FLIP, 0, out.ctypes.data, 3, None) == INVALID
    assert lib.yolo_view_table(hip.VIEWS_FLIP, 0, None, 3, ctypes.byref(n)) == INVALID and n.value == 0
    with pytest.raises(hip.YoloError, match="yolo_view_table"):
        hip.view_table(7)


def test_the_new_entry_points_are_bound():
    lib = hip.load_library()
    for name in ("yolo_view_table", "yolo_classify_views_u8", "yolo_op_view_reduce"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert (hip.VIEWS_FLIP, hip.VIEWS_TEN_CROP) == (1, 2)
    assert callable(hip.Engine.classify_views) and callable(hip.op_view_reduce)


def test_fixture_lists_the_cases_the_generator_states():
    g = golden("views_cases.npz")
    assert [tuple(r) for r in g["cases"]] == [(c[0], c[1], str(c[2]), str(c[3])) for c in V.CASES]
    assert tuple(g["net_hw"]) == (V.NET_H, V.NET_W)
    # the sizes the views must survive: W' x H' = (24 + shift) x (20 + shift)
    shapes = {c[0]: (c[3], c[4], c[5]) for c in V.CASES}
    assert shapes["s5_exact"] == (5, V.NET_H + 5, V.NET_W + 5) and shapes["s0_exact"] == (0, V.NET_H, V.NET_W) and shapes["s32_1x1"] == (32, 1, 1)
    assert shapes["s5_axis"][2] == V.NET_W + 5 and shapes["s5_axis"][1] != V.NET_H + 5
    for name, cfg, _, _, _ in V.NETS:
        assert str(g[name + "_cfg"]) == cfg


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_equals_the_fixture_views(case):
    g = golden("views_cases.npz")
    _, _, mode, shift, h, w = next(c for c in V.CASES if c[0] == case)
    img, views = g[case + "_image_u8"], g[case + "_views"]
    assert img.shape[:2] == (h, w)
    if mode == V.TEN_CROP:
        assert views.shape[0] == 10
        assert np.array_equal(bits(views), bits(V.ten_crop_numpy(img, shift)))
        if shift == 0:
            assert all(np.array_equal(bits(views[v]), bits(views[0])) for v in range(5))          # the five crops coincide
        if shift >= V.NET_W:
            assert len(np.unique(bits(views[0]).reshape(-1, views.shape[-1]), axis=0)) == 1          # (-s, -s): nothing but the corner pixel
    else:
        assert views.shape[0] == 2
        assert np.array_equal(bits(views[0]), bits(V.stretch_numpy(img)))
        assert np.array_equal(bits(views[1]), bits(views[0][:, ::-1]))


@pytest.mark.parametrize("case", CASES)
def test_fixture_sum_is_the_sequential_fp32_sum_and_its_topk(case):
    """axpy_cpu's order, restated: ((0 + p_0) + p_1) + ...; top_k's order: value descending, the earlier class first among equals"""
    g = golden("views_cases.npz")
    rows = g[case + "_rows"]
    s = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        s = s + r
    assert np.array_equal(bits(s), bits(g[case + "_sum"]))
    assert np.array_equal(np.argsort(-s, kind="stable")[:int(g["top"])].astype(np.int32), g[case + "_topk"])
    # the gap the fp32 top-k test needs, as the generator asserted it
    bound = V.sum_bound(rows, s, g[case + "_max_logit"], 2e-4)
    order = np.argsort(-s, kind="stable")
    for j in range(int(g["top"])):
        assert float(s[order[j]]) - float(s[order[j + 1]]) > 2 * max(bound[order[j]], bound[order[j + 1]])


@pytest.mark.parametrize("case", CASES)
def test_fresh_reference_composition_equals_the_fixture(case, tmp_path, monkeypatch):
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    g = golden("views_cases.npz")
    _, netname, mode, shift, _, _ = next(c for c in V.CASES if c[0] == case)
    R = V.RefViews()
    img = g[case + "_image_u8"]
    views = R.ten_views(img, shift) if mode == V.TEN_CROP else R.flip_views(V.stretch_numpy(img))
    assert np.array_equal(bits(views), bits(g[case + "_views"]))
    if case not in ("s5_odd", "tree_s5", "flip_grey", "rgbd_s32"):
        return          # the networks: one case per cfg
    (tmp_path / V.TREE_FILE).write_text(str(g["tree_text"]))
    monkeypatch.chdir(tmp_path)
    cfg = str(g[netname + "_cfg"])
    net = DR.RefNet(cfg, g[netname + "_weights"], 0, 2)
    tree = R.l.read_tree(V.TREE_FILE.encode()) if "tree=" in cfg else None
    logit_layer = max(i for i, s in enumerate(V_parse(cfg)) if s == "convolutional")
    rows, total, topk, max_logit = R.reduce(net, views, logit_layer, tree)
    net.close()
    assert np.array_equal(bits(rows), bits(g[case + "_rows"])) and np.array_equal(bits(total), bits(g[case + "_sum"]))
    assert np.array_equal(topk, g[case + "_topk"]) and np.array_equal(bits(max_logit), bits(g[case + "_max_logit"]))


def V_parse(cfg):
    from yolo_tensorflow_amd import darknet_io as IO
    return [s["type"] for s in IO.parse_cfg(cfg)[1:]]


def test_python_argument_checks():
    with pytest.raises(hip.YoloError, match="rows"):
        hip.op_view_reduce(np.zeros((5, 4), np.float32), 2)          # 5 rows are no whole number of 2-view images
    with pytest.raises(hip.YoloError, match="rows"):
        hip.op_view_reduce(np.zeros((4,), np.float32), 2)
    with pytest.raises(hip.YoloError, match="views"):
        hip.op_view_reduce(np.zeros((4, 4), np.float32), 0)
    # refused by the library in front of any device call
    lib = hip.load_library()
    x = np.zeros((33, 4), np.float32); out = np.zeros((1, 4), np.float32)
    cls = np.zeros((1, 8), np.int32); top = np.zeros((1, 8), np.float32)
    assert lib.yolo_op_view_reduce(x.ctypes.data, 1, 33, 4, 1.0, 0, out.ctypes.data, None, None, 0) == INVALID          # views 1..32
    assert lib.yolo_op_view_reduce(x.ctypes.data, 1, 2, 4, 1.0, 5, out.ctypes.data, cls.ctypes.data, top.ctypes.data, 0) == INVALID      # top_k > len
    assert lib.yolo_op_view_reduce(x.ctypes.data, 1, 2, 4, 1.0, 2, out.ctypes.data, None, top.ctypes.data, 0) == INVALID
    assert lib.yolo_op_view_reduce(None, 1, 2, 4, 1.0, 0, out.ctypes.data, None, None, 0) == INVALID
    assert lib.yolo_classify_views_u8(None, None, 0, None, 1, hip.VIEWS_FLIP, 0, 0, hip.HOST, 1.0, 0, None, None, hip.HOST) == INVALID
    from yolo_tensorflow_amd.classifier import Classifier
    assert Classifier.VIEWS == {"flip": hip.VIEWS_FLIP, "ten_crop": hip.VIEWS_TEN_CROP}
