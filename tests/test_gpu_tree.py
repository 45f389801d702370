"""Softmax trees on the device against the reference's own tree code (bound in tests/test_tree_host.py): the segmented softmax, the descent
walk, a [region] tree head through the veneer and through yolo_detect*, a [softmax] tree classifier, and a wide tree in 16-bit
storage.

Which rows a label comparison may leave out: those where, on the path the float64 walk takes, the two best values of a group lie
within 1e-5 relative of each other, or p * max lies within 1e-5 of the threshold -- at most 2 % of the rows."""
import ctypes as C
import os
import numpy as np
import pytest
from oracle import darknet_ref as DR, postprocess_ref as PR
from yolo_tensorflow_amd import darknet_io as IO
from tests import test_tree_host as TF

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRESHOLDS = (0.0, 0.3, 0.5, 0.9)


class IMAGE(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


def _bind(lib):
    """the veneer's entry points this file calls, declared as the reference's binding declares them (D2T/darknet.py:20-115)"""
    lib.load_network.argtypes = [C.c_char_p, C.c_char_p, C.c_int]; lib.load_network.restype = C.c_void_p
    lib.free_network.argtypes = [C.c_void_p]
    lib.network_predict_image.argtypes = [C.c_void_p, IMAGE]; lib.network_predict_image.restype = C.POINTER(C.c_float)
    lib.get_network_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    lib.get_network_boxes.restype = C.POINTER(DR.DETECTION)
    lib.free_detections.argtypes = [C.POINTER(DR.DETECTION), C.c_int]
    return lib


def _collect(dets, n, classes):
    bb = np.zeros((n, 4), np.float32); obj = np.zeros(n, np.float32); pr = np.zeros((n, classes), np.float32)
    for i in range(n):
        d = dets[i]
        bb[i] = (d.bbox.x, d.bbox.y, d.bbox.w, d.bbox.h); obj[i] = d.objectness
        pr[i] = np.ctypeslib.as_array(d.prob, shape=(classes,))
    return bb, obj, pr


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    d = tmp_path_factory.mktemp("trees")
    a, b = TF.tree_a(d / "a.tree"), TF.tree_b(d / "b.tree")
    return {"A": (a, TF.RefTree(a)), "B": (b, TF.RefTree(b)), "dir": d}


def _logits(n, nodes, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, nodes)) * scale).astype(np.float32)
    return x, rng


@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("temp", [1.0, 2.5])
def test_op_tree_softmax(hiplib, trees, which, temp):
    """Against softmax_cpu per group + hierarchy_predictions of the compiled reference.  Tolerance of the flat yolo_op_softmax test
    (tests/test_gpu_classifier.py::test_op_softmax): every conditional probability within 2^-21 max|x| / temp + 2e-6 relative; an
    absolute value is a product along a path of at most `depth` such factors (+ one rounding each)."""
    path, ref = trees[which]
    x, rng = _logits(3, ref.n, 5 + ref.n)
    x[0, rng.choice(ref.n, 12, replace=False)] = np.float32(30.0); x[1, rng.choice(ref.n, 12, replace=False)] = np.float32(-30.0)
    cond_ref = ref.conditional(x, temp)
    bound = 2.0 ** -21 * float(np.abs(x).max()) / temp + 2e-6
    depth = np.zeros(ref.n, int)
    for j in range(ref.n):
        depth[j] = 0 if ref.parent[j] < 0 else depth[ref.parent[j]] + 1
    for mode, want in ((0, cond_ref), (1, ref.absolute(cond_ref, 0)), (2, ref.absolute(cond_ref, 1))):
        got = hiplib.op_tree_softmax(x, path, temperature=temp, mode=mode)
        nz = want > 1e-30                      # (below: products that leave the normal range; only their smallness is checked)
        assert (got[~nz] <= 2e-30).all()
        assert np.array_equal(got == 0, want == 0) or mode < 2, "leaves mask"
        rel = np.abs(got.astype(np.float64) - want)[nz] / want[nz]
        lim = (bound * (1 if mode == 0 else (depth[None, :] + 1)) * np.ones_like(want, dtype=np.float64))[nz]
        print("tree %s temp %g mode %d: max rel err / bound %.3f" % (which, temp, mode, float((rel / lim).max())))
        assert (rel <= lim).all()
        if mode == 2:
            assert (got[:, ref.leaf == 0] == 0).all() and (got[:, ref.leaf == 1] > 0).any()
    sums = np.add.reduceat(hiplib.op_tree_softmax(x, path, temperature=temp).astype(np.float64), ref.group_offset, axis=1)
    assert np.abs(sums - 1.0).max() <= 1e-5


def _hand_rows(ref, rng):
    """20 rows aimed at each return branch of hierarchy_top_prediction: fail at the root (flat root group), fail deeper (one sharp
    root node above a flat group of >= 3 children), reach a leaf (a sharp path down to it), and a sharp path through the group of 1."""
    x = np.zeros((20, ref.n), np.float32)
    one = int(np.flatnonzero(ref.group_size == 1)[0]); node1 = int(ref.group_offset[one])
    roots = [j for j in range(ref.group_size[0]) if ref.child[j] >= 0 and ref.group_size[ref.child[j]] >= 3]
    leaves = np.flatnonzero(ref.leaf == 1)
    for r in range(20):
        kind = r % 4
        x[r] = rng.standard_normal(ref.n).astype(np.float32) * 0.01                      # flat: p * max ~ 1 / 6 at the root
        if kind == 1:
            x[r, roots[(r // 4) % len(roots)]] = 12.0
        elif kind >= 2:
            j = node1 if kind == 3 else int(leaves[rng.integers(0, len(leaves))])
            while j >= 0:
                x[r, j] = 20.0; j = int(ref.parent[j])
    return x


def _compare_labels(ref, x, got, want, thr, what):
    bad = np.flatnonzero(got != want)
    a64 = ref.abs64(x[bad]) if len(bad) else np.zeros((0, ref.n))
    skipped = [r for k, r in enumerate(bad) if ref.walk64(a64[k], thr)[1]]
    print("%s thresh %g: %d of %d rows differ, %d of them ambiguous" % (what, thr, len(bad), len(x), len(skipped)))
    assert len(skipped) == len(bad), "%s: rows %s differ from hierarchy_top_prediction" % (what, [int(r) for r in bad if r not in skipped][:8])
    assert len(skipped) <= 0.02 * len(x)


@pytest.mark.parametrize("which", ["A", "B"])
def test_op_tree_top(hiplib, trees, which):
    path, ref = trees[which]
    x, rng = _logits(2000, ref.n, 77 + ref.n, scale=4.0)
    x[:20] = _hand_rows(ref, rng)
    absolute = ref.absolute(ref.conditional(x, 1.0), 0)
    a64 = ref.abs64(x)
    for thr in THRESHOLDS:
        want = ref.top(absolute, thr)
        # the seeds keep the reference itself stable: its float32 labels against the float64 walk
        amb = sum(1 for r in range(len(x)) if ref.walk64(a64[r], thr)[0] != want[r])
        assert amb <= 0.02 * len(x)
        got = hiplib.op_tree_top(x, path, hier_thresh=thr)
        _compare_labels(ref, x, got, want, thr, "tree %s" % which)
    # the hand-made rows take the branch each was made for (float64 walk at hier_thresh 0.5), none of them near a tie
    one = int(np.flatnonzero(ref.group_size == 1)[0])
    for r in range(20):
        label, amb, how, groups = ref.walk64(a64[r], 0.5, trace=True)
        assert not amb, "hand-made row %d is ambiguous" % r
        assert how == ("root", "deeper", "leaf")[r % 4] if r % 4 < 3 else one in groups, "row %d: exit %s through groups %s" % (r, how, groups)
        if r % 4 == 1:
            assert label == ref.parent[ref.group_offset[groups[-1]]] and len(groups) >= 2


def _region_cfg(tree, classes, size, grid_convs, na=2):
    convs = ""
    filters = 8
    for _ in range(grid_convs):
        convs += "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n[maxpool]\nsize=2\nstride=2\n\n" % filters
        filters *= 2
    anchors = ",  ".join("%g,%g" % (0.8 + k, 1.1 + 0.7 * k) for k in range(na))
    return ("[net]\nbatch=1\nsubdivisions=1\nwidth=%d\nheight=%d\nchannels=3\n\n%s[convolutional]\nfilters=%d\nsize=1\nstride=1\npad=1\nactivation=linear\n\n"
            "[region]\nanchors=%s\nbias_match=1\nclasses=%d\ncoords=4\nnum=%d\nsoftmax=1\ntree=%s\n" % (size, size, convs, na * (5 + classes), anchors, classes, na, tree))


def _sharpen(secs, flat, classes, na, gain):
    """scale the head conv's class filters so the class logits spread over several units (else every group is near uniform)"""
    last = IO.conv_specs(secs)[-1]
    tail = last["filters"] * (1 + last["cin"] * last["size"] ** 2)
    flat = flat.copy(); flat[-tail:] *= np.float32(gain)
    return flat


@pytest.fixture(scope="module")
def region_net(trees, hiplib):
    """tiny-voc style trunk at 96 x 96 -> 3 x 3 grid, 2 anchors, tree A, fp32: the cfg, its weights, the oracle's view of one image"""
    path, ref = trees["A"]
    txt = _region_cfg(path, ref.n, 96, 5)
    secs = IO.parse_cfg(txt)
    flat = _sharpen(secs, IO.synth_weights(secs, 31, obj_bias=0.0), ref.n, 2, 6.0)
    d = trees["dir"]
    cfg = str(d / "region.cfg"); wf = str(d / "region.weights")
    open(cfg, "w").write(txt); IO.write_weights_file(wf, flat, 0, 1)
    return dict(txt=txt, flat=flat, cfg=cfg, wf=wf, ref=ref, path=path)


def _oracle_boxes(raw, ref, anchors, thresh, hier, map200=None):
    """get_region_detections with a tree (DN/region_layer.c:391-435) over OUR raw head tensor [g, g, na * (5 + C)], the class part
    through the reference's softmax_cpu (temperature 1, the GPU path's) / hierarchy_predictions / hierarchy_top_prediction.
    -> boxes [na * g * g, 4], objectness, prob, the absolute probabilities and logits per record (anchor-major, as darknet indexes)"""
    g = raw.shape[0]; na = len(anchors); A = 5 + ref.n
    r = raw.reshape(g * g, na, A).astype(np.float64)
    lg = lambda v: 1.0 / (1.0 + np.exp(-v))
    N = na * g * g
    bb = np.zeros((N, 4)); obj = np.zeros(N); prob = np.zeros((N, ref.n), np.float32); logits = np.zeros((N, ref.n), np.float32)
    for i in range(g * g):
        for n in range(na):
            k = n * g * g + i
            bb[k] = ((i % g + lg(r[i, n, 0])) / g, (i // g + lg(r[i, n, 1])) / g, np.exp(r[i, n, 2]) * anchors[n][0] / g, np.exp(r[i, n, 3]) * anchors[n][1] / g)
            obj[k] = lg(r[i, n, 4]); logits[k] = raw.reshape(g * g, na, A)[i, n, 5:]
    absolute = ref.absolute(ref.conditional(logits, 1.0), 0)
    scale = obj.astype(np.float32)
    if map200 is not None:
        p = scale[:, None] * absolute[:, map200]
        prob[:, :200] = np.where(p > thresh, p, 0)
        top = p
    else:
        top = ref.top(absolute, hier)
        prob[np.arange(N), top] = np.where(scale > thresh, scale, 0)
    return bb, obj, prob, top, logits, absolute


def test_region_tree_through_the_veneer(hiplib, region_net):
    os.environ["DARKNET_HIP_DTYPE"] = "fp32"
    R = region_net; ref = R["ref"]
    ven = _bind(C.CDLL(os.path.join(ROOT, "yolo_tensorflow_amd", "libdarknet_hip.so")))
    vnet = ven.load_network(R["cfg"].encode(), R["wf"].encode(), 0)
    assert vnet
    w = h = 96
    img = np.ascontiguousarray(np.random.default_rng(4).random((3, h, w), dtype=np.float32))
    im = IMAGE(w, h, 3, img.ctypes.data_as(C.POINTER(C.c_float)))
    assert bool(ven.network_predict_image(vnet, im))
    # the same forward on a context of our own: its raw head tensor feeds the oracle
    eng = hiplib.Engine(R["txt"], max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(R["flat"])
    eng._check(eng.lib.yolo_forward_letterbox_chw(eng.ctx, img.ctypes.data, w, h, hiplib.HOST, None, hiplib.HOST), "yolo_forward_letterbox_chw")
    raw = eng.head_raw(0, 1)[0]
    anchors = [(0.8, 1.1), (1.8, 1.8)]
    N = 3 * 3 * 2
    map200 = np.random.default_rng(9).integers(0, ref.n, 200).astype(np.int32)
    for thresh in (0.0, 0.3):
        bb, obj, prob, top, logits, _ = _oracle_boxes(raw, ref, anchors, thresh, 0.5)
        nv = C.c_int(0)
        dv = ven.get_network_boxes(vnet, w, h, thresh, 0.5, None, 1, C.byref(nv))
        assert nv.value == N
        bv, ov, pv = _collect(dv, N, ref.n)
        dv2 = ven.get_network_boxes(vnet, w, h, thresh, 0.5, None, 1, C.byref(nv))
        b2, o2, p2 = _collect(dv2, N, ref.n)
        assert np.array_equal(bv, b2) and np.array_equal(ov, o2) and np.array_equal(pv, p2), "get_network_boxes twice"
        ven.free_detections(dv, N); ven.free_detections(dv2, N)
        np.testing.assert_allclose(bv, bb, rtol=2e-3, atol=2e-3)
        clear = np.abs(obj - thresh) > 1e-3
        np.testing.assert_allclose(ov[clear], np.where(obj > thresh, obj, 0)[clear], rtol=2e-3, atol=2e-4)
        assert ((pv != 0).sum(axis=1) <= 1).all()
        gated = clear & (obj > thresh)
        assert ((pv != 0).sum(axis=1)[gated] == 1).all() and gated.sum() > 0
        got_top = pv.argmax(axis=1)
        _compare_labels(ref, logits[gated], got_top[gated], top[gated], 0.5, "veneer thresh %g" % thresh)
        same = gated & (got_top == top)
        np.testing.assert_allclose(pv[same, top[same]], obj[same], rtol=2e-3, atol=2e-4)
        # the map form: exactly 200 entries, objectness * absolute[map[j]] gated by thresh
        bb, obj, prob, praw, _, _ = _oracle_boxes(raw, ref, anchors, thresh, 0.5, map200)
        dm = ven.get_network_boxes(vnet, w, h, thresh, 0.5, map200.ctypes.data_as(C.POINTER(C.c_int)), 1, C.byref(nv))
        _, _, pm = _collect(dm, N, ref.n)
        ven.free_detections(dm, N)
        assert (pm[:, 200:] == 0).all() and (pm[:, :200] != 0).any()
        clear_p = np.abs(praw - thresh) > 1e-3 * max(thresh, 1e-3)
        np.testing.assert_allclose(pm[:, :200][clear_p], prob[:, :200][clear_p], rtol=2e-3, atol=2e-4)
    # the layer output: conditional probabilities, planar
    out = eng.last_layer_output(1)[0].reshape(2, 5 + ref.n, 9)
    cond = ref.conditional(raw.reshape(9, 2, 5 + ref.n)[:, :, 5:].reshape(18, ref.n), 1.0).reshape(9, 2, ref.n)
    np.testing.assert_allclose(out[:, 5:, :].transpose(2, 0, 1), cond, rtol=1e-4, atol=1e-7)
    eng.close(); ven.free_network(vnet)


def _detect_records(hiplib, R, imgs, full, graph, thr, monkeypatch):
    monkeypatch.delenv("YOLO_TREE_FULL", raising=False); monkeypatch.delenv("YOLO_TREE_DESCENT", raising=False)
    monkeypatch.setenv("YOLO_TREE_FULL" if full else "YOLO_TREE_DESCENT", "1")
    eng = hiplib.Engine(R["txt"], max_batch=3, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(R["flat"])
    kw = dict(score_thr=thr, iou_thr=0.45, max_out=18, nms_mode=hiplib.NMS_DARKNET)
    if graph:
        import torch
        d_img = torch.from_numpy(imgs).cuda(); boxes = torch.zeros(3 * 18 * 24, dtype=torch.uint8, device="cuda"); counts = torch.zeros(3, dtype=torch.int32, device="cuda")
        for _ in range(3):          # eager, capture, replay
            eng.detect_graph(d_img, boxes, counts, hier_thresh=0.5, **kw)
        eng.synchronize()
        cn = counts.cpu().numpy(); bx = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(3, 18)
        recs = [bx[i, :cn[i]].copy() for i in range(3)]
    else:
        recs = eng.detect_fused(imgs, hier_thresh=0.5, **kw)
    det = eng.forward(imgs)
    raw = eng.head_raw(0, 3)
    eng.close()
    return recs, det, raw


def test_region_tree_detect_forms_and_darknet_nms(hiplib, region_net, monkeypatch):
    """yolo_detect and yolo_detect_graph at batch 3: the descent form and the forced full form give identical records, and
    YOLO_NMS_DARKNET over them equals oracle/postprocess_ref.py fed with the tree scores (objectness) and labels."""
    R = region_net; ref = R["ref"]
    imgs = np.random.default_rng(8).integers(0, 256, (3, 96, 96, 3), dtype=np.uint8)
    thr = 0.3
    lean, det, raw = _detect_records(hiplib, R, imgs, False, False, thr, monkeypatch)
    full, det2, _ = _detect_records(hiplib, R, imgs, True, False, thr, monkeypatch)
    graph, _, _ = _detect_records(hiplib, R, imgs, False, True, thr, monkeypatch)
    assert np.array_equal(det, det2)
    assert sum(len(r) for r in lean) > 0
    compared = 0
    for b in range(3):
        assert np.array_equal(lean[b], full[b]), "image %d: descent form vs full form" % b
        assert np.array_equal(lean[b], graph[b]), "image %d: yolo_detect vs yolo_detect_graph" % b
        # oracle pipeline: a one-hot class column at the tree's top prediction makes row_scores give (objectness, label)
        logits = raw[b].reshape(9, 2, 5 + ref.n)[:, :, 5:].reshape(18, ref.n)
        top = ref.top(ref.absolute(ref.conditional(logits, 1.0), 0), 0.5)
        a64 = ref.abs64(logits)
        amb = [r for r in range(18) if ref.walk64(a64[r], 0.5)[1]]
        onehot = np.zeros((18, 5 + ref.n), np.float32); onehot[:, :5] = det[b][:, :5]; onehot[np.arange(18), 5 + top] = 1.0
        want, rows = PR.postprocess_records(onehot, thr, 0.45, 18, PR.NMS_DARKNET, 0)
        if not any(r in amb for r in rows):          # (an image with a kept row the oracle itself cannot label is left out: at most one of three)
            compared += 1
            assert len(want) == len(lean[b])
            for k in ("x0", "y0", "x1", "y1", "score", "cls"):
                assert np.array_equal(want[k], lean[b][k]), "image %d field %s" % (b, k)
    assert compared >= 2, "only %d of 3 images could be compared with the oracle pipeline" % compared
    # the absolute probabilities of the decoded tensor
    logits = raw.reshape(27, 2, 5 + ref.n)[:, :, 5:].reshape(54, ref.n)
    want_abs = ref.absolute(ref.conditional(logits, 1.0), 0)
    np.testing.assert_allclose(det.reshape(54, 5 + ref.n)[:, 5:], want_abs, rtol=1e-4, atol=1e-9)


CLS_TRUNK = ("[net]\nbatch=1\nsubdivisions=1\nheight=64\nwidth=64\nchannels=3\n\n"
             "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n[maxpool]\nsize=2\nstride=2\n\n"
             "[convolutional]\nbatch_normalize=1\nfilters=16\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n[maxpool]\nsize=2\nstride=2\n\n"
             "[convolutional]\nbatch_normalize=1\nfilters=32\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
             "[convolutional]\nfilters=240\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")


@pytest.mark.parametrize("temp", [1.0, 2.0])
def test_softmax_tree_classifier(hiplib, trees, temp):
    """The mini classifier trunk with tree A behind it: the whole network against the compiled reference's network_predict (the
    [softmax] path parses its temperature and is sound), then yolo_classify's top-5 in the three hierarchy modes."""
    path, ref = trees["A"]
    txt = CLS_TRUNK + "tree=%s\ntemperature=%g\n" % (path, temp)
    secs = IO.parse_cfg(txt)
    flat = _sharpen(secs, IO.synth_weights(secs, seed=23), 240, 1, 40.0)
    img = np.random.default_rng(24).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    net = DR.RefNet(txt, flat, 0, 2)
    net.predict(img.astype(np.float32) / np.float32(255.0))
    want = np.asarray(net.layer_output_nhwc(net.n - 1), dtype=np.float32).reshape(-1)
    logit = np.asarray(net.layer_output_nhwc(net.n - 2), dtype=np.float32).reshape(-1)
    net.close()
    assert float(np.abs(logit).max()) > 1.0
    eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(flat)
    x = np.stack([img, img[::-1].copy()])
    got = eng.classify(x, top_k=0)
    d = 2e-4 * float(np.abs(logit).max()) / temp
    bound = want.astype(np.float64) * np.expm1(2 * d) + 1e-7          # (tests/test_gpu_classifier.py::_prob_bound, fp32 tolerance)
    assert (np.abs(got[0].astype(np.float64) - want) <= bound).all()
    assert np.array_equal(eng.last_layer_output(2), got)
    geo = eng.tree_geometry()
    assert geo["n"] == ref.n and np.array_equal(geo["parent"], ref.parent) and np.array_equal(geo["group_size"], ref.group_size)
    cond = got
    for mode, name, form in ((0, None, cond), (1, "absolute", ref.absolute(cond, 0)), (2, "leaves", ref.absolute(cond, 1))):
        eng.set_hierarchy_mode(name)
        probs = eng.classify(x, top_k=0)
        np.testing.assert_allclose(probs, form, rtol=1e-5, atol=1e-12)
        cls, tkp = eng.classify(x, top_k=5)
        for b in range(2):
            order = np.argsort(-probs[b], kind="stable")[:5]
            assert np.array_equal(cls[b], order.astype(np.int32)), "mode %d image %d" % (mode, b)
            assert np.array_equal(tkp[b], probs[b][order])
        if mode == 2:
            assert all(ref.leaf[k] for k in cls.ravel())
    eng.close()


@pytest.mark.parametrize("dtype_name", ["BF16", "FP16X2"])
def test_wide_tree_head_in_16_bit_storage(hiplib, trees, dtype_name, monkeypatch):
    """Tree B (a group of 700) behind a 1x1 head on a 2 x 2 grid, one anchor: plans and runs in bf16 and in split-fp16 pairs (the
    head is fp32 in both); labels of both forms against the oracle walking the head's own raw logits."""
    monkeypatch.delenv("YOLO_TREE_FULL", raising=False); monkeypatch.setenv("YOLO_TREE_DESCENT", "1")
    path, ref = trees["B"]
    txt = _region_cfg(path, ref.n, 64, 5, na=1)
    secs = IO.parse_cfg(txt)
    flat = _sharpen(secs, IO.synth_weights(secs, 41, obj_bias=1.0), ref.n, 1, 6.0)
    eng = hiplib.Engine(txt, max_batch=2, dtype=getattr(hiplib, dtype_name), semantics=hiplib.SEM_DARKNET)
    eng.set_weights(flat)
    imgs = np.random.default_rng(3).integers(0, 256, (2, 64, 64, 3), dtype=np.uint8)
    recs = eng.detect_fused(imgs, score_thr=0.05, iou_thr=1.0, max_out=4, nms_mode=hiplib.NMS_DARKNET, hier_thresh=0.3)
    det = eng.forward(imgs)
    raw = eng.head_raw(0, 2).reshape(8, 5 + ref.n)
    full, rows = eng.postprocess(2, score_thr=0.05, iou_thr=1.0, max_out=4, nms_mode=hiplib.NMS_DARKNET, return_rows=True)
    eng.close()
    assert sum(len(r) for r in recs) > 0
    want = ref.top(ref.absolute(ref.conditional(raw[:, 5:], 1.0), 0), 0.3).reshape(2, 4)
    for b in range(2):
        assert np.array_equal(recs[b], full[b])
        r = rows[b]
        _compare_labels(ref, raw.reshape(2, 4, -1)[b][r][:, 5:], full[b]["cls"], want[b][r], 0.3, "%s image %d" % (dtype_name, b))


def test_export_embeds_the_tree_and_leaves_other_artifacts_alone(hiplib, region_net, tmp_path, monkeypatch):
    """The artifact of a tree network loads with the tree file gone; the artifact of a network without a tree has the bytes it
    always had: cfg text, scales, tile plan, parameters, checksum -- nothing between the tile plan and the first conv."""
    R = region_net
    eng = hiplib.Engine(R["txt"], max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(R["flat"])
    imgs = np.random.default_rng(8).integers(0, 256, (1, 96, 96, 3), dtype=np.uint8)
    want = eng.forward(imgs)
    art = str(tmp_path / "tree.yolohip")
    eng.export(art); eng.close()
    moved = R["path"] + ".moved"
    os.rename(R["path"], moved)
    try:
        e2 = hiplib.Engine.from_file(art, max_batch=1)
        assert np.array_equal(e2.forward(imgs), want)
        assert e2.tree_geometry()["n"] == R["ref"].n
        e2.close()
    finally:
        os.rename(moved, R["path"])
    txt = IO.with_input_size(IO.cfg_text("yolov3-tiny"), 96)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=0)
    e3 = hiplib.Engine(txt, max_batch=1, dtype=hiplib.FP32)
    e3.set_weights(flat)
    plain = str(tmp_path / "plain.yolohip")
    e3.export(plain)
    # the layout every artifact had before trees: header (magic, seven words, one reserved word = 0), cfg text, one scale and one tile
    # config per layer, then per conv three sizes and its filters + bias, then the checksum.  A tree-less artifact has exactly that
    # length and a zero reserved word: nothing was inserted anywhere
    blob = open(plain, "rb").read()
    n_layers = len(IO.parse_cfg(txt)) - 1
    up = lambda v, m: (v + m - 1) // m * m
    assert blob[:8] == b"YOLOHIP1" and int.from_bytes(blob[8:12], "little") == 3 and int.from_bytes(blob[36:40], "little") == 0
    want = 40 + len(txt.encode()) + 2 * 4 * n_layers + 8
    for cv in IO.conv_specs(IO.parse_cfg(txt)):
        cout_pad, kpad = up(cv["filters"], 256), up(cv["size"] ** 2 * up(cv["cin"], 8), 64)
        want += 3 * 8 + cout_pad * kpad * 4 + cout_pad * 4          # fp32 filters, fp32 bias, no fp8 scales
    assert len(blob) == want
    tree_blob = open(art, "rb").read()
    assert int.from_bytes(tree_blob[36:40], "little") == 1          # the flag that says tree blobs follow the tile plan
    e3.close()
