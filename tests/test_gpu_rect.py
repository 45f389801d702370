"""Networks whose input is not square (width != height) on the device: parity with the compiled reference at 64 x 96 and 96 x 64, fused plans
against layer-by-layer plans bit for bit, the decode operator against a numpy restatement, the decode forms against each other, ingest
(stretch, letterbox, cv2; single images and ragged batches), box geometry in source coordinates, the C ABI and the darknet veneer.

YOLOv3's topology closes only where both sides are multiples of 32 (tests/test_rect_host.py pins the refusal of 208 x 416): the full-size
shapes here are 192 x 416 and 416 x 192, where every fusion of the headline plan fires."""
import ctypes as C
import importlib.util
import os
import re
import numpy as np
import pytest
from conftest import golden
from oracle import yolo_ref as R, darknet_ref as DR, postprocess_ref as P
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ((37, 80), (50, 37), (32, 48))          # the letterbox fixture's source images, height x width


def _relmax(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _recs_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _probs_close(got, ref, thresh):
    """prob = objectness * class, zero unless above thresh: entries within 1e-3 of the threshold may flip and are left out"""
    near = (np.abs(got - thresh) < 1e-3) | (np.abs(ref - thresh) < 1e-3)
    np.testing.assert_allclose(np.where(near, 0, got), np.where(near, 0, ref), rtol=2e-3, atol=2e-4)
    assert near.mean() < 0.02


def _v3(hw):
    txt = IO.with_input_size(IO.cfg_text("yolov3"), hw)
    return txt, IO.synth_weights(IO.parse_cfg(txt), seed=11)


# ---- reference parity -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mini_v3_rect.npz", "mini_v2_rect.npz"])
@pytest.mark.parametrize("dtype_name,tol", [("FP32", 5e-4), ("BF16", 3e-2)])
def test_mini_network_matches_compiled_reference(hiplib, name, dtype_name, tol):
    g = golden(name)
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=getattr(hiplib, dtype_name), semantics=hiplib.SEM_DARKNET, keep_layers=True)
    assert eng.input_hw == g["image_u8"].shape[:2] and eng.size == g["image_u8"].shape[0]
    eng.set_weights(g["weights"])
    eng.forward(g["image_u8"][None], scale=1.0 / 255.0)
    for i, s in enumerate(IO.parse_cfg(str(g["cfg"]))[1:]):
        if s["type"] in ("yolo", "region"):
            continue
        got, ref = eng.layer_output(i, 1), g["layer_%02d" % i]
        assert got.shape == ref.shape
        print("%s %s layer %d (%s): %.3e" % (name, dtype_name, i, s["type"], _relmax(got, ref)))
        assert _relmax(got, ref) < tol, "layer %d (%s)" % (i, s["type"])
    eng.close()


def test_mini_v3_rect_boxes_match_darknet(hiplib):
    g = golden("mini_v3_rect.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(g["weights"])
    det = eng.forward(g["image_u8"][None])[0]
    keep = det[:, 4] > float(g["thresh"])
    assert keep.sum() == len(g["boxes_raw"])
    np.testing.assert_allclose(det[keep, :4], g["boxes_raw"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(det[keep, 4], g["obj_raw"], rtol=2e-3, atol=2e-4)
    eng.close()


def test_mini_v2_rect_boxes_match_darknet(hiplib):
    """get_region_detections returns every box, anchor-major (index = n * w * h + i); the decoded tensor is cell-major, anchor inner"""
    g = golden("mini_v2_rect.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(g["weights"])
    det = eng.forward(g["image_u8"][None])[0]
    geo = eng.head_geometry(0)
    assert (geo["grid_h"], geo["grid_w"]) == (12, 8) and geo["kind"] == 1          # 96 high x 64 wide, stride 8
    cells, na = geo["grid_h"] * geo["grid_w"], geo["anchors"]
    assert len(g["boxes_raw"]) == cells * na == det.shape[0]
    mine = det.reshape(cells, na, -1).transpose(1, 0, 2).reshape(cells * na, -1)
    np.testing.assert_allclose(mine[:, :4], g["boxes_raw"], rtol=2e-3, atol=2e-4)
    thresh = float(g["thresh"])
    np.testing.assert_allclose(np.where(mine[:, 4] > thresh, mine[:, 4], 0), g["obj_raw"], rtol=2e-3, atol=2e-4)
    eng.close()


def test_mini_cls_rect_matches_compiled_reference(hiplib):
    """The classifier test's bound: relmax < 5e-4 (fp32) on the layers, and on the probabilities tol * (1 + 2 max|logit|) * p + a floor"""
    g = golden("mini_cls_rect.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    eng.set_weights(g["weights"])
    p = eng.classify(g["image_u8"][None], top_k=0)
    assert p.shape == (1, 24) and eng.input_hw == (64, 96)
    for i, s in enumerate(IO.parse_cfg(str(g["cfg"]))[1:]):
        if s["type"] == "softmax":
            continue
        assert _relmax(eng.layer_output(i, 1).reshape(-1), np.asarray(g["layer_%02d" % i]).reshape(-1)) < 5e-4, "layer %d" % i
    # a relative logit error e moves a probability by at most 2 e max|logit| relative (numerator and denominator)
    bound = 5e-4 * 2.0 * float(g["max_abs_logit"]) * g["output"].astype(np.float64) + 1e-7
    assert (np.abs(p[0].astype(np.float64) - g["output"]) <= bound).all()
    eng.close()


# ---- fused plans equal layer-by-layer plans, bit for bit -----------------------------------------------
KNOBS = ("YOLO_NO_RESBLOCK", "YOLO_NO_HALO", "YOLO_NO_S2", "YOLO_NO_C3S2", "YOLO_NO_PAIR_STEM")


def _plans_agree(hiplib, monkeypatch, hw, dtype, knobs, want_in_plan):
    txt, flat = _v3(hw)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    rc, table = hiplib.plan_table(txt, dtype=dtype, max_batch=3)
    assert rc == 0, table
    for w in want_in_plan:
        assert (re.search(w, table) if w.startswith("tail_layer") else w in table), "the plan at %s lacks %s" % (hw, w)
    img = np.random.default_rng(hw[0] * 1000 + hw[1]).integers(0, 256, (3, hw[0], hw[1], 3), dtype=np.uint8)
    dets = []
    for keep, knob in [(False, None), (True, None)] + [(False, k) for k in knobs]:
        if knob:
            monkeypatch.setenv(knob, "1")
        eng = hiplib.Engine(txt, max_batch=3, dtype=dtype, keep_layers=keep)
        if knob:
            monkeypatch.delenv(knob)
        eng.set_weights(flat)
        dets.append(eng.forward(img))
        eng.close()
    assert np.abs(dets[0]).max() > 0 and np.isfinite(dets[0]).all()
    for d, what in zip(dets[1:], ["keep_layers"] + list(knobs)):
        assert np.array_equal(dets[0], d), "%s: fused plan differs from %s" % (hw, what)


@pytest.mark.parametrize("dtype_name", ["BF16", "FP16"])
@pytest.mark.parametrize("hw", [(64, 96), (96, 32), (192, 416), (416, 192)])
def test_fused_plans_equal_layer_by_layer_plans(hiplib, monkeypatch, hw, dtype_name):
    """(64, 96), (96, 32): one to three c3s2 tile columns, every tile on a border, an odd tile walk over three images.  (192, 416), (416, 192):
    48 x 104 at the 128-channel stage -- the resblock launch, 13 x 13 halo blocks on ragged 12 x 26 / 6 x 13 grids, the 1x1 tails and the head
    tail as on the headline plan."""
    big = max(hw) > 100
    want = ["fused=stem", "fused=c3s2", "kernel=halo", "kernel=s2"] + (["fused=resblock", r"tail_layer=\d"] if big else [])
    _plans_agree(hiplib, monkeypatch, hw, getattr(hiplib, dtype_name), (("YOLO_NO_RESBLOCK",) if big else ()) + ("YOLO_NO_HALO", "YOLO_NO_S2", "YOLO_NO_C3S2"), want)


@pytest.mark.parametrize("dtype_name,hw", [("FP16X2", (64, 96)), ("FP16X2", (192, 416)), ("FP8", (64, 96))])
def test_fused_plans_of_the_other_storage_forms(hiplib, monkeypatch, dtype_name, hw):
    """bit for bit against that storage form's own unfused plan"""
    want = ["fused=pair-stem"] if dtype_name == "FP16X2" else []
    _plans_agree(hiplib, monkeypatch, hw, getattr(hiplib, dtype_name), ("YOLO_NO_PAIR_STEM", "YOLO_NO_HALO") if dtype_name == "FP16X2" else ("YOLO_NO_HALO",), want)


# ---- decode operator ------------------------------------------------------------------------------------
def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _decode_numpy(raw, anchors, classes, img_hw, mode):
    """The semantics, literally, in float64.  raw [n, gh, gw, na * (5 + C)].  mode 'pixel' / 'ratio' (V3 detection_layer with per-axis
    strides sx = img_w / gw, sy = img_h / gh), 'region' (get_region_box + softmax).  With darknet's [yolo] form x = (col + s) / gw,
    w = e^tw aw / netw, which is the ratio mode's ((col + s) sx) / img_w and (e^tw (aw / sx)) sx / img_w where img_w = gw sx."""
    n, gh, gw, _ = raw.shape
    na = len(anchors)
    r = raw.reshape(n, gh, gw, na, 5 + classes).astype(np.float64)
    col = np.arange(gw).reshape(1, 1, gw, 1); row = np.arange(gh).reshape(1, gh, 1, 1)
    aw = np.array([a[0] for a in anchors], np.float64).reshape(1, 1, 1, na); ah = np.array([a[1] for a in anchors], np.float64).reshape(1, 1, 1, na)
    out = np.zeros_like(r)
    if mode == "region":
        out[..., 0] = (col + _sig(r[..., 0])) / gw; out[..., 1] = (row + _sig(r[..., 1])) / gh
        out[..., 2] = np.exp(r[..., 2]) * aw / gw; out[..., 3] = np.exp(r[..., 3]) * ah / gh
        out[..., 4] = _sig(r[..., 4])
        e = np.exp(r[..., 5:] - r[..., 5:].max(-1, keepdims=True)); out[..., 5:] = e / e.sum(-1, keepdims=True)
    else:
        sx, sy = img_hw[1] // gw, img_hw[0] // gh
        out[..., 0] = (_sig(r[..., 0]) + col) * sx; out[..., 1] = (_sig(r[..., 1]) + row) * sy
        out[..., 2] = np.exp(r[..., 2]) * (aw / sx) * sx; out[..., 3] = np.exp(r[..., 3]) * (ah / sy) * sy
        if mode == "ratio":
            out[..., 0] /= img_hw[1]; out[..., 2] /= img_hw[1]; out[..., 1] /= img_hw[0]; out[..., 3] /= img_hw[0]
        out[..., 4:] = _sig(r[..., 4:])
    return out.reshape(n, gh * gw * na, 5 + classes)


@pytest.mark.parametrize("classes", [1, 80])
@pytest.mark.parametrize("grid", [(2, 3), (3, 2), (1, 5), (5, 1), (13, 7)])
def test_op_decode_hw(hiplib, grid, classes):
    gh, gw = grid
    rng = np.random.default_rng(gh * 100 + gw * 10 + classes)
    anchors = [(10, 13), (16, 30), (33, 23)]
    raw = (rng.standard_normal((2, gh, gw, 3 * (5 + classes))) * 2).astype(np.float32)
    img_hw = (16 * gh, 32 * gw)          # distinct strides along the two axes as well
    for mode, dec in (("pixel", hiplib.DECODE_PIXEL), ("ratio", hiplib.DECODE_RATIO)):
        got = hiplib.op_decode_hw(raw, anchors, classes, img_hw, dec)
        # tests/test_gpu_ops.py's bound for op_decode: expf / sigmoid differ from numpy's by a few ulp
        np.testing.assert_allclose(got, _decode_numpy(raw, anchors, classes, img_hw, mode), rtol=3e-6, atol=1e-7, err_msg=mode)
    # darknet's [yolo] form, stated on its own: x / gw, y / gh, e^tw aw / netw, e^th ah / neth
    r = raw.reshape(2, gh, gw, 3, 5 + classes).astype(np.float64)
    got = hiplib.op_decode_hw(raw, anchors, classes, img_hw, hiplib.DECODE_RATIO).reshape(2, gh, gw, 3, 5 + classes)
    np.testing.assert_allclose(got[..., 0], (np.arange(gw).reshape(1, 1, gw, 1) + _sig(r[..., 0])) / gw, rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(got[..., 1], (np.arange(gh).reshape(1, gh, 1, 1) + _sig(r[..., 1])) / gh, rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(got[..., 2], np.exp(r[..., 2]) * np.array([10, 16, 33.0]) / img_hw[1], rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(got[..., 3], np.exp(r[..., 3]) * np.array([13, 30, 23.0]) / img_hw[0], rtol=3e-6, atol=1e-7)
    ranchors = [(0.57273, 0.677385), (1.87446, 2.06253), (3.33843, 5.47434)]
    got = hiplib.op_decode_hw(raw, ranchors, classes, img_hw, region=True)
    want = _decode_numpy(raw, ranchors, classes, img_hw, "region")
    # tests/test_gpu_ops.py's bounds for the region decode
    np.testing.assert_allclose(got[..., :4], want[..., :4], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(got[..., 4], want[..., 4], rtol=3e-6)
    np.testing.assert_allclose(got[..., 5:], want[..., 5:], rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("g,classes", [(3, 1), (13, 80)])
def test_op_decode_hw_of_a_square_grid_is_op_decode(hiplib, g, classes):
    rng = np.random.default_rng(g)
    raw = (rng.standard_normal((2, g, g, 3 * (5 + classes))) * 2).astype(np.float32)
    anchors = [(10, 13), (16, 30), (33, 23)]
    for dec in (hiplib.DECODE_PIXEL, hiplib.DECODE_RATIO):
        assert np.array_equal(hiplib.op_decode_hw(raw, anchors, classes, (32 * g, 32 * g), dec), hiplib.op_decode(raw, anchors, classes, 32 * g, dec))
    assert np.array_equal(hiplib.op_decode_hw(raw, anchors, classes, (32 * g, 32 * g), region=True), hiplib.op_decode(raw, anchors, classes, 32 * g, region=True))


# ---- decode forms agree ---------------------------------------------------------------------------------
@pytest.mark.parametrize("decode", ["DECODE_RATIO", "DECODE_PIXEL"])
def test_lean_detect_equals_forward_and_postprocess(hiplib, decode):
    hw = (64, 96)
    txt = IO.with_input_size(IO.cfg_text("yolov3"), hw)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=5, obj_bias=-0.75)
    eng = hiplib.Engine(txt, max_batch=3, dtype=hiplib.BF16, decode=getattr(hiplib, decode))
    eng.set_weights(flat)
    img = np.random.default_rng(3).integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)
    det = eng.forward(img)
    sc = (det[..., 4:5] * det[..., 5:]).max(-1)
    thr = float(np.quantile(sc, 0.97))
    kept = 0
    for mode, select, max_out in ((hiplib.NMS_TF, hiplib.SELECT_GT, 20), (hiplib.NMS_DARKNET, hiplib.SELECT_GT, 60), (hiplib.NMS_TF_V1, hiplib.SELECT_GE, 20),
                                  (hiplib.NMS_PER_CLASS, hiplib.SELECT_GT, 60)):
        kw = dict(score_thr=thr, iou_thr=0.45, max_out=max_out, nms_mode=mode, select_mode=select)
        lean = eng.detect_fused(img, **kw)
        with pytest.raises(hiplib.YoloError, match="without materialising"):          # the decoded tensor was skipped: the lean decode ran
            eng.postprocess(3, score_thr=1.0, nms_mode=hiplib.NMS_NUMPY_V3)
        eng.forward(img, want_detections=False)
        full = eng.postprocess(3, **kw)
        for b in range(3):
            assert _recs_equal(lean[b], full[b]), "mode %d image %d" % (mode, b)
            if decode == "DECODE_RATIO" or mode != hiplib.NMS_PER_CLASS:
                want, _ = P.postprocess_records(det[b], thr, 0.45, max_out, mode, select, image_hw=hw if mode == hiplib.NMS_PER_CLASS else None)
                for k in ("x0", "y0", "x1", "y1", "score", "cls"):
                    assert np.array_equal(want[k], full[b][k]), "mode %d image %d field %s against the record oracle" % (mode, b, k)
            kept += len(full[b])
    assert kept > 0
    eng.close()


def test_tree_head_forms_agree_on_a_rectangular_grid(hiplib, monkeypatch, tmp_path):
    """A YOLO9000-shaped mini at 64 x 96 (2 x 3 grid): the descent form equals the full form, and the full form's decoded tensor equals
    get_region_box on a gh x gw grid + the tree's absolute probabilities (the restatement of tests/test_gpu_tree.py with gh != gw)."""
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    from tests import test_tree_host as TF
    spec = importlib.util.spec_from_file_location("make_cfgs", os.path.join(ROOT, "tools", "make_cfgs.py"))
    M = importlib.util.module_from_spec(spec); spec.loader.exec_module(M)
    path = TF.tree_a(tmp_path / "a.tree"); ref = TF.RefTree(path)
    txt = IO.with_input_size(M.yolo9000(size=64, classes=ref.n, tree=str(path)), (64, 96))
    secs = IO.parse_cfg(txt)
    flat = IO.synth_weights(secs, 31, obj_bias=0.0).copy()
    last = IO.conv_specs(secs)[-1]
    flat[-last["filters"] * (1 + last["cin"] * last["size"] ** 2):] *= np.float32(6.0)
    imgs = np.random.default_rng(8).integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)
    kw = dict(score_thr=0.3, iou_thr=0.45, max_out=18, nms_mode=hiplib.NMS_DARKNET)
    recs = {}
    for full in (False, True):
        monkeypatch.delenv("YOLO_TREE_FULL", raising=False); monkeypatch.delenv("YOLO_TREE_DESCENT", raising=False)
        monkeypatch.setenv("YOLO_TREE_FULL" if full else "YOLO_TREE_DESCENT", "1")
        eng = hiplib.Engine(txt, max_batch=3, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
        eng.set_weights(flat)
        recs[full] = eng.detect_fused(imgs, hier_thresh=0.5, **kw)
        if full:
            det = eng.forward(imgs); raw = eng.head_raw(0, 3); geo = eng.head_geometry(0)
        eng.close()
    assert sum(len(r) for r in recs[True]) > 0
    for b in range(3):
        assert np.array_equal(recs[False][b], recs[True][b]), "image %d: descent form vs full form" % b
    gh, gw, na = geo["grid_h"], geo["grid_w"], geo["anchors"]
    assert (gh, gw) == (2, 3) and raw.shape == (3, 2, 3, na * (5 + ref.n))
    anchors = [tuple(float(v) for v in a) for a in M.YOLO9000_ANCHORS]
    r = raw.reshape(3, gh * gw, na, 5 + ref.n).astype(np.float64)
    d = det.reshape(3, gh * gw, na, 5 + ref.n)
    for i in range(gh * gw):
        for n in range(na):
            want = np.stack([(i % gw + _sig(r[:, i, n, 0])) / gw, (i // gw + _sig(r[:, i, n, 1])) / gh,
                             np.exp(r[:, i, n, 2]) * anchors[n][0] / gw, np.exp(r[:, i, n, 3]) * anchors[n][1] / gh, _sig(r[:, i, n, 4])], -1)
            np.testing.assert_allclose(d[:, i, n, :5], want, rtol=1e-5, atol=1e-6)
    logits = raw.reshape(-1, 5 + ref.n)[:, 5:]
    np.testing.assert_allclose(det.reshape(-1, 5 + ref.n)[:, 5:], ref.absolute(ref.conditional(np.ascontiguousarray(logits), 1.0), 0), rtol=1e-4, atol=1e-9)


# ---- ingest ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_hw", [(64, 96), (96, 64)])
@pytest.mark.parametrize("src_hw", [(50, 37), (37, 80)])
def test_op_resize_u8_hw(hiplib, src_hw, out_hw):
    img = np.random.default_rng(src_hw[0]).integers(0, 256, src_hw + (3,), dtype=np.uint8)
    got = hiplib.op_resize_u8_hw(img, out_hw)
    want = R.resize_bilinear_legacy(img.astype(np.float32) / np.float32(255), out_hw[0], out_hw[1])
    assert got.shape == want.shape == out_hw + (3,)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
    assert np.array_equal(hiplib.op_resize_u8_hw(img, (64, 64)), hiplib.op_resize_u8(img, 64))


def test_letterbox_inputs_match_the_reference(hiplib):
    """darknet's letterbox_image into 96 wide x 64 high, at the tolerance of the square helper test (tests/test_gpu_darknet_veneer.py)"""
    g = golden("mini_v3_rect_letterbox.npz")
    for k, (ih, iw) in enumerate(SOURCES):
        got = hiplib.op_letterbox(g["src_%d" % k], 96, 64)
        assert got.shape == (3, 64, 96)
        np.testing.assert_allclose(got, g["input_%d" % k], rtol=0, atol=2e-6, err_msg="source %d x %d" % (ih, iw))


@pytest.fixture(scope="module")
def rect_engine(hiplib):
    g = golden("mini_v3_rect.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=3, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    eng.set_weights(g["weights"])
    yield eng, g
    eng.close()


def _u8_sources(seed=4):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in SOURCES]


def test_letterboxed_forward_matches_recorded_boxes(hiplib, rect_engine):
    """yolo_forward_letterbox_chw + yolo_darknet_boxes at each source image's (w, h), relative = 1, against the reference's
    get_network_boxes; the first conv's tensor equals the one the recorded letterboxed input gives"""
    eng, g = rect_engine
    lb = golden("mini_v3_rect_letterbox.npz")
    thresh = float(lb["thresh"])
    for k, (ih, iw) in enumerate(SOURCES):
        src = np.ascontiguousarray(lb["src_%d" % k])
        assert eng.lib.yolo_forward_letterbox_chw(eng.ctx, src.ctypes.data, iw, ih, hiplib.HOST, None, hiplib.HOST) == 0
        first = eng.layer_output(0, 1)
        rec = eng.darknet_boxes(0, iw, ih, thresh=thresh, relative=1)
        assert len(rec) == len(lb["boxes_%d" % k])
        np.testing.assert_allclose(rec[:, :4], lb["boxes_%d" % k], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(rec[:, 4], lb["obj_%d" % k], rtol=2e-3, atol=2e-4)
        _probs_close(rec[:, 5:], lb["prob_%d" % k], thresh)
        eng.forward(np.ascontiguousarray(lb["input_%d" % k].transpose(1, 2, 0))[None], scale=1.0)
        assert _relmax(first, eng.layer_output(0, 1)) < 1e-4          # (inputs within 2e-6 of each other, values up to 1)


@pytest.mark.parametrize("fit", ["FIT_STRETCH", "FIT_LETTERBOX", "FIT_CV2"])
def test_ragged_batch_equals_single_images(hiplib, rect_engine, fit):
    eng, g = rect_engine
    imgs = _u8_sources()
    f = getattr(hiplib, fit)
    det = eng.forward_images(imgs, fit=f)
    first = eng.layer_output(0, 3)
    kw = dict(score_thr=0.3, iou_thr=0.45, max_out=40, nms_mode=hiplib.NMS_DARKNET)
    got = eng.detect_images(imgs, fit=f, units=hiplib.UNITS_NETWORK, **kw)
    assert sum(len(r) for r in got) > 0
    for i, im in enumerate(imgs):
        d1 = eng.forward_images([im], fit=f)
        assert np.array_equal(eng.layer_output(0, 1)[0], first[i]), "image %d: the layer that reads the fitted input" % i
        assert np.array_equal(d1[0], det[i])
        assert _recs_equal(eng.detect_images([im], fit=f, units=hiplib.UNITS_NETWORK, **kw)[0], got[i])
        if fit == "FIT_STRETCH":          # ... and the single-image entry point
            assert np.array_equal(eng.forward_image(im)[0], det[i])
        if fit == "FIT_LETTERBOX":
            chw = np.ascontiguousarray((im.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))
            assert eng.lib.yolo_forward_letterbox_chw(eng.ctx, chw.ctypes.data, im.shape[1], im.shape[0], hiplib.HOST, None, hiplib.HOST) == 0
            assert np.array_equal(eng.layer_output(0, 1)[0], first[i])


@pytest.mark.parametrize("units", ["UNITS_NETWORK", "UNITS_SOURCE_PIXELS"])
def test_letterbox_records_are_darknets_boxes(hiplib, rect_engine, units):
    """LETTERBOX: every kept record of YOLO_NMS_DARKNET is one of get_network_boxes' boxes of that image -- relative (UNITS_NETWORK) or in
    source pixels -- which test_letterboxed_forward_matches_recorded_boxes pins to the reference's"""
    eng, g = rect_engine
    imgs = _u8_sources()
    got = eng.detect_images(imgs, fit=hiplib.FIT_LETTERBOX, units=getattr(hiplib, units), score_thr=0.3, iou_thr=0.45, max_out=50, nms_mode=hiplib.NMS_DARKNET)
    eng.forward_images(imgs, fit=hiplib.FIT_LETTERBOX)
    kept = 0
    for i, im in enumerate(imgs):
        rec = eng.darknet_boxes(i, im.shape[1], im.shape[0], thresh=0.0, relative=1 if units == "UNITS_NETWORK" else 0)
        boxes = {tuple(r[:4].tolist()) for r in rec}
        for r in got[i]:
            assert (float(r["x0"]), float(r["y0"]), float(r["x1"]), float(r["y1"])) in boxes
        kept += len(got[i])
    assert kept > 0


@pytest.mark.parametrize("decode", ["DECODE_RATIO", "DECODE_PIXEL"])
def test_stretch_records_in_source_pixels(hiplib, decode):
    """normalised boxes * (w, h); network-pixel boxes * (w / netw, h / neth): distinct factors along the two axes, float64, rounded once"""
    g = golden("mini_v3_rect.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=3, dtype=hiplib.FP32, decode=getattr(hiplib, decode))
    eng.set_weights(g["weights"])
    imgs = _u8_sources()
    kw = dict(score_thr=0.3, iou_thr=0.45, max_out=40)
    got = eng.detect_images(imgs, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, **kw)
    net = eng.detect_images(imgs, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_NETWORK, **kw)
    kept = 0
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        ratio = np.array([w, h], np.float64) if decode == "DECODE_RATIO" else np.array([w / 96.0, h / 64.0])
        box = (np.stack([net[i]["x0"], net[i]["y0"], net[i]["x1"], net[i]["y1"]], -1).reshape(-1, 2, 2).astype(np.float64) * ratio).reshape(-1, 4).astype(np.float32)
        gb = np.stack([got[i]["x0"], got[i]["y0"], got[i]["x1"], got[i]["y1"]], -1).reshape(-1, 4)
        assert gb.shape == box.shape
        np.testing.assert_array_max_ulp(gb, box, maxulp=1)
        assert np.array_equal(got[i]["score"], net[i]["score"]) and np.array_equal(got[i]["cls"], net[i]["cls"])
        kept += len(gb)
    assert kept > 0
    eng.close()


def test_image_that_letterboxes_to_nothing_is_refused_before_any_launch(hiplib, rect_engine):
    eng, g = rect_engine
    img = np.zeros((1, 200, 3), np.uint8)
    buf, descs = hiplib.pack_images([img])
    rc = eng.lib.yolo_forward_images_u8(eng.ctx, buf.ctypes.data, buf.nbytes, descs.ctypes.data, 1, hiplib.FIT_LETTERBOX, hiplib.HOST, None, hiplib.HOST)
    assert rc == -1 and "less than one pixel" in eng.lib.yolo_last_error(eng.ctx).decode()          # YOLO_ERR_INVALID


# ---- C ABI ----------------------------------------------------------------------------------------------
def test_head_geometry_and_raw_views(hiplib, rect_engine):
    eng, g = rect_engine
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    heads = [i for i, s in enumerate(secs) if s["type"] == "yolo"]
    det = eng.forward(g["image_u8"][None])
    off = 0
    for k, li in enumerate(heads):
        geo = eng.head_geometry(k)
        ref = g["layer_%02d" % (li - 1)]
        assert (geo["kind"], geo["grid_h"], geo["grid_w"], geo["anchors"], geo["row_offset"]) == (0, ref.shape[1], ref.shape[2], 3, off)
        assert geo["grid_h"] != geo["grid_w"]
        off += ref.shape[1] * ref.shape[2] * 3
        kind, grid, na, ro = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        rc = eng.lib.yolo_head_geometry(eng.ctx, k, C.byref(kind), C.byref(grid), C.byref(na), C.byref(ro))
        assert rc == -6 and "yolo_head_geometry_hw" in eng.lib.yolo_last_error(eng.ctx).decode()          # YOLO_ERR_UNSUPPORTED
        raw = eng.head_raw(k, 1)
        assert raw.shape == ref.shape and np.array_equal(raw, eng.layer_output(li - 1, 1))
    assert off == eng.rows == det.shape[1]
    # the last layer in darknet's own layout: planar [na * (5 + C)][gh * gw], the logistic on x, y, objectness and the classes
    last = eng.last_layer_output(1)[0]
    raw = eng.layer_output(heads[-1] - 1, 1)[0]
    gh, gw = raw.shape[:2]
    want = raw.reshape(gh * gw, 3, 9).astype(np.float64)
    want = np.where(np.isin(np.arange(9), (2, 3)), want, _sig(want)).transpose(1, 2, 0).reshape(-1)
    assert last.shape == want.shape
    np.testing.assert_allclose(last, want, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(last.reshape(27, gh, gw).transpose(1, 2, 0)[None], g["layer_%02d" % heads[-1]], rtol=2e-3, atol=2e-4)


def test_export_round_trip_and_graphs(hiplib, tmp_path):
    import torch
    hw = (64, 96)
    txt = IO.with_input_size(IO.cfg_text("yolov3"), hw)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=5, obj_bias=-0.75)
    eng = hiplib.Engine(txt, max_batch=3, dtype=hiplib.BF16)
    eng.set_weights(flat)
    img = np.random.default_rng(3).integers(0, 256, (3, 64, 96, 3), dtype=np.uint8)
    det = eng.forward(img)
    thr = float(np.quantile((det[..., 4:5] * det[..., 5:]).max(-1), 0.97))
    kw = dict(score_thr=thr, iou_thr=0.45, max_out=20)
    want = eng.detect_fused(img, **kw)
    assert sum(len(r) for r in want) > 0
    path = str(tmp_path / "rect.yolohip")
    eng.export(path)
    e2 = hiplib.Engine.from_file(path, max_batch=3)
    assert e2.input_hw == hw and e2.rows == eng.rows
    assert np.array_equal(e2.forward(img), det)
    for a, b in zip(e2.detect_fused(img, **kw), want):
        assert _recs_equal(a, b)
    e2.close()
    # captured detect steps: eager, capture, two replays
    d_img = torch.from_numpy(img).cuda(); boxes = torch.zeros(3 * 20 * 24, dtype=torch.uint8, device="cuda"); counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    for it in range(4):
        boxes.zero_(); counts.zero_()
        eng.detect_graph(d_img, boxes, counts, **kw)
        eng.synchronize()
        cn = counts.cpu().numpy(); bx = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(3, 20)
        for b in range(3):
            assert _recs_equal(bx[b, :cn[b]], want[b]), "detect_graph call %d image %d" % (it, b)
    imgs = _u8_sources()
    want_i = eng.detect_images(imgs, fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, **kw)
    buf, descs = hiplib.pack_images(imgs)
    d_pix = torch.from_numpy(buf).cuda()
    for it in range(4):
        boxes.zero_(); counts.zero_()
        eng.detect_images_graph(d_pix, descs, boxes, counts, fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, **kw)
        eng.synchronize()
        cn = counts.cpu().numpy(); bx = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(3, 20)
        for b in range(3):
            assert _recs_equal(bx[b, :cn[b]], want_i[b]), "detect_images_graph call %d image %d" % (it, b)
    eng.close()


class IMAGE(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


def test_veneer_on_a_rectangular_cfg(hiplib, tmp_path, monkeypatch):
    """load_network, network_width / network_height, network_predict_image (letterbox into 96 x 64), get_network_boxes at the image's
    (w, h) and do_nms_sort against the vectors recorded from the reference library"""
    monkeypatch.setenv("DARKNET_HIP_DTYPE", "fp32")
    g, lb = golden("mini_v3_rect.npz"), golden("mini_v3_rect_letterbox.npz")
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(g["cfg"])); IO.write_weights_file(wf, g["weights"], int(g["header"][0]), int(g["header"][1]))
    ven = C.CDLL(os.path.join(ROOT, "yolo_tensorflow_amd", "libdarknet_hip.so"))
    ven.load_network.argtypes = [C.c_char_p, C.c_char_p, C.c_int]; ven.load_network.restype = C.c_void_p
    ven.free_network.argtypes = [C.c_void_p]
    ven.network_width.argtypes = [C.c_void_p]; ven.network_height.argtypes = [C.c_void_p]
    ven.network_predict_image.argtypes = [C.c_void_p, IMAGE]; ven.network_predict_image.restype = C.POINTER(C.c_float)
    ven.get_network_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    ven.get_network_boxes.restype = C.POINTER(DR.DETECTION)
    ven.free_detections.argtypes = [C.POINTER(DR.DETECTION), C.c_int]
    ven.do_nms_sort.argtypes = [C.POINTER(DR.DETECTION), C.c_int, C.c_int, C.c_float]
    net = ven.load_network(cfg.encode(), wf.encode(), 0)
    assert net and ven.network_width(net) == 96 and ven.network_height(net) == 64
    classes, thresh, nms = 4, float(lb["thresh"]), float(lb["nms"])
    for k, (ih, iw) in enumerate(SOURCES):
        src = np.ascontiguousarray(lb["src_%d" % k])
        out = ven.network_predict_image(net, IMAGE(iw, ih, 3, src.ctypes.data_as(C.POINTER(C.c_float))))
        assert bool(out)
        num = C.c_int(0)
        dets = ven.get_network_boxes(net, iw, ih, thresh, .5, None, 1, C.byref(num))
        n = num.value
        assert n == len(lb["boxes_%d" % k])
        bb = np.array([(dets[i].bbox.x, dets[i].bbox.y, dets[i].bbox.w, dets[i].bbox.h) for i in range(n)], np.float32)
        pr = np.array([np.ctypeslib.as_array(dets[i].prob, shape=(classes,)).copy() for i in range(n)], np.float32)
        np.testing.assert_allclose(bb, lb["boxes_%d" % k], rtol=2e-3, atol=2e-4)
        _probs_close(pr, lb["prob_%d" % k], thresh)
        # NMS on identical inputs: the reference's own detections go through the veneer's do_nms_sort (the reference sorts the array, the
        # veneer suppresses in place: compared as multisets of (box, probability row))
        for i in range(n):
            dets[i].bbox.x, dets[i].bbox.y, dets[i].bbox.w, dets[i].bbox.h = (float(v) for v in lb["boxes_%d" % k][i])
            dets[i].objectness = float(lb["obj_%d" % k][i])
            row = np.ascontiguousarray(lb["prob_%d" % k][i])
            C.memmove(dets[i].prob, row.ctypes.data, classes * 4)
        ven.do_nms_sort(dets, n, classes, nms)
        prn = np.array([np.ctypeslib.as_array(dets[i].prob, shape=(classes,)).copy() for i in range(n)], np.float32)
        key = lambda b, p: sorted(map(tuple, np.concatenate([b, p], axis=1).round(6).tolist()))
        assert key(lb["boxes_%d" % k], prn) == key(lb["boxes_nms_%d" % k], lb["prob_nms_%d" % k])
        assert 0 < (prn > 0).sum() < (lb["prob_%d" % k] > 0).sum()
        ven.free_detections(dets, n)
    ven.free_network(net)
