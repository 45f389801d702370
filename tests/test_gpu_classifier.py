"""Classifier networks on the device: [avgpool], [softmax] (+ top-k), [cost], the classifier context and its public surface
(yolo_classify*, Engine.classify*, Classifier, darknet_hip.classify), against float64 numpy for the operators and against the
reference's own C code (tests/golden/mini_cls19.npz / mini_cls53.npz, oracle/_ref) for whole networks."""
import ctypes as C
import os
import numpy as np
import pytest
from conftest import golden
from oracle import darknet_ref as DR
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_DIR = os.path.join(ROOT, "tests", "golden", "images")
JPGS = ["dog.jpg", "eagle.jpg", "giraffe.jpg", "horses.jpg", "kite.jpg", "person.jpg"]
U = 2.0 ** -24          # unit roundoff of fp32


def _relmax(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _bf16(x):
    """fp32 -> nearest bfloat16 (ties to even), as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _half_ulp(v, mant_bits, min_exp):
    """half a unit in the last place of |v| in a binary format with `mant_bits` explicit mantissa bits and minimum exponent `min_exp`"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** min_exp)))
    return 0.5 * 2.0 ** (e - mant_bits)


# ---- check 4: operators against float64 numpy, bounds from the arithmetic ----
@pytest.mark.parametrize("h,w,c", [(8, 8, 1024), (7, 7, 1000), (13, 13, 24), (5, 5, 21), (1, 1, 40)])
def test_op_avgpool(hiplib, h, w, c):
    """fp32: the sum of h * w terms in ANY order is off by at most (h w - 1) u sum|x|, the division adds u |mean|: together
    <= h w u mean|x| per channel.  16-bit storage: the reference is the mean of the values as stored, and the stored result adds
    half a unit in the last place of the storage type.  Split-fp16 pairs keep 22 bits: 2^-22 relative on the way in (per term, so
    2^-22 mean|x|) and on the way out."""
    rng = np.random.default_rng(h * 1000 + c)
    x = (rng.standard_normal((3, h, w, c)) * 3 + 0.5).astype(np.float32)
    for dtype in (hiplib.FP32, hiplib.BF16, hiplib.FP16, hiplib.FP16X2):
        xs = _bf16(x) if dtype == hiplib.BF16 else x.astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else x
        ref = xs.astype(np.float64).mean(axis=(1, 2))
        bound = h * w * U * np.abs(xs.astype(np.float64)).mean(axis=(1, 2))
        if dtype == hiplib.BF16:
            bound = bound + _half_ulp(ref, 7, -126)
        elif dtype == hiplib.FP16:
            bound = bound + _half_ulp(ref, 10, -14)
        elif dtype == hiplib.FP16X2:
            bound = bound + 2.0 ** -21 * np.abs(x.astype(np.float64)).mean(axis=(1, 2)) + 2.0 ** -24          # (+ the fp16 subnormal floor of a lo half)
        got = hiplib.op_avgpool(x, dtype=dtype)
        assert got.shape == (3, c) and got.dtype == np.float32
        err = np.abs(got.astype(np.float64) - ref)
        print("avgpool %dx%dx%d dtype %d: max err / bound %.3f" % (h, w, c, dtype, float((err / bound).max())))
        assert (err <= bound).all(), "dtype %d: %g over the bound" % (dtype, float((err - bound).max()))


def _softmax64(x, groups, temp):
    x = x.astype(np.float64).reshape(x.shape[0], groups, -1) / temp
    e = np.exp(x - x.max(axis=2, keepdims=True))
    return (e / e.sum(axis=2, keepdims=True)).reshape(x.shape[0], -1)


@pytest.mark.parametrize("length", [24, 1000, 8192])
@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("temp", [1.0, 2.0])
def test_op_softmax(hiplib, length, groups, temp):
    """relative error of every probability <= 2^-21 max|x| / temp + 2e-6: the two fp32 quotients x / t and max / t and their
    difference put at most 4 u max|x| / t into the exponent (a relative error of the result), expf, the sum and the divide the
    rest."""
    rng = np.random.default_rng(length + groups)
    x = rng.uniform(-30, 30, (3, length * groups)).astype(np.float32)
    x[1] = rng.standard_normal(length * groups).astype(np.float32) * 4
    p = hiplib.op_softmax(x, groups=groups, temperature=temp)
    ref = _softmax64(x, groups, temp)
    rel = np.abs(p.astype(np.float64) - ref) / ref
    bound = 2.0 ** -21 * float(np.abs(x).max()) / temp + 2e-6
    print("softmax len %d groups %d temp %g: max rel err %.3e (bound %.3e)" % (length, groups, temp, float(rel.max()), bound))
    assert (rel <= bound).all()
    sums = p.astype(np.float64).reshape(3, groups, -1).sum(axis=2)
    assert np.abs(sums - 1.0).max() <= 1e-5


# ---- check 5: the selection is exact ----
def _topk_inputs(length):
    rng = np.random.default_rng(length)
    x = rng.uniform(-8, 8, (4, length)).astype(np.float32)
    x[1] = np.float32(1.25)                                         # all logits equal
    x[2] = rng.uniform(-8, 0, length).astype(np.float32)
    x[2, rng.choice(length, min(100, length // 2), replace=False)] = np.float32(3.5)      # 100 equal maxima
    x[3] = np.round(rng.uniform(-3, 3, length)).astype(np.float32)  # many ties at every level
    return x


@pytest.mark.parametrize("length,ks", [(24, (1, 5, 24)), (1000, (1, 5, 32)), (8192, (1, 5, 32))])
def test_topk_is_exact(hiplib, length, ks):
    x = _topk_inputs(length)
    for k in ks:
        p, cls, tkp = hiplib.op_softmax(x, top_k=k)
        for b in range(x.shape[0]):
            want = np.argsort(-p[b], kind="stable")[:k]
            assert np.array_equal(cls[b], want.astype(np.int32)), "row %d k %d" % (b, k)
            assert np.array_equal(tkp[b].view(np.uint32), p[b][want].view(np.uint32)), "row %d k %d" % (b, k)
    # the probabilities do not depend on whether the launch also selects
    assert np.array_equal(hiplib.op_softmax(x), hiplib.op_softmax(x, top_k=5)[0])


def test_topk_beyond_the_row_is_marked_empty(hiplib):
    p, cls, tkp = hiplib.op_softmax(np.arange(6, dtype=np.float32)[None], top_k=8)
    assert list(cls[0]) == [5, 4, 3, 2, 1, 0, -1, -1] and tkp[0, 6] == 0 and tkp[0, 7] == 0


# ---- check 6: networks against the compiled reference ----
def _prob_bound(p_ref, tol, max_logit):
    """logits within d = tol * max|logit| of the reference's move every exponent by at most 2 d (its own and the maximum's), so
    every probability by the factor exp(+-2 d)"""
    d = tol * float(max_logit)
    return p_ref.astype(np.float64) * np.expm1(2 * d) + 1e-7


def _dtypes(hiplib):
    return ((hiplib.FP32, 2e-4), (hiplib.FP16, 4e-3), (hiplib.BF16, 3e-2), (hiplib.FP16X2, 2e-4))


@pytest.mark.parametrize("name", ["mini_cls19", "mini_cls53"])
def test_mini_classifiers_match_compiled_reference(hiplib, name, tmp_path):
    g = golden(name + ".npz")
    cfg = str(g["cfg"])
    secs = IO.parse_cfg(cfg)[1:]
    x = g["image_u8"][None]
    out = g["output"]
    for dtype, tol in _dtypes(hiplib):
        eng = hiplib.Engine(cfg, max_batch=3, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=True)
        eng.set_weights(g["weights"])
        assert eng.rows == 0 and eng.attrs == 0 and eng.num_classes == 24
        p = eng.classify(x, top_k=0)
        assert p.shape == (1, 24)
        for i, s in enumerate(secs):
            if s["type"] == "cost":
                continue          # darknet's cost layer holds no tensor at inference (forward returns without a truth); here it aliases its input
            got = eng.layer_output(i, 1).reshape(-1)
            ref = np.asarray(g["layer_%02d" % i]).reshape(-1)
            if s["type"] == "softmax":
                err = np.abs(got.astype(np.float64) - ref)
                print("%s dtype %d softmax: max err / bound %.3f" % (name, dtype, float((err / _prob_bound(ref, tol, g["max_abs_logit"])).max())))
                assert (err <= _prob_bound(ref, tol, g["max_abs_logit"])).all(), "softmax dtype %d" % dtype
                assert np.array_equal(got, p[0])
            else:
                print("%s dtype %d layer %d (%s): relmax %.3e" % (name, dtype, i, s["type"], _relmax(got, ref)))
                assert _relmax(got, ref) < tol, "layer %d (%s) dtype %d: %g" % (i, s["type"], dtype, _relmax(got, ref))
        if any(s["type"] == "cost" for s in secs):
            assert np.array_equal(eng.layer_output(len(secs) - 1, 1).reshape(-1), p[0])       # identity
        assert np.array_equal(eng.last_layer_output(1)[0], p[0])       # the last layer that is not [cost]
        eng.close()
        # the production plan (fusions on, tail launches as planned): same bound, the selection agrees with the matrix, batches, export
        eng = hiplib.Engine(cfg, max_batch=3, dtype=dtype, semantics=hiplib.SEM_DARKNET)
        eng.set_weights(g["weights"])
        q = eng.classify(x, top_k=0)
        assert (np.abs(q[0].astype(np.float64) - out) <= _prob_bound(out, tol, g["max_abs_logit"])).all(), "dtype %d" % dtype
        groups = int([s for s in secs if s["type"] == "softmax"][0].get("groups", 1))
        if groups == 1:
            cls, tk = eng.classify(x, top_k=5)
            want = np.argsort(-q[0], kind="stable")[:5]
            assert np.array_equal(cls[0], want) and np.array_equal(tk[0], q[0][want])
        else:
            with pytest.raises(hiplib.YoloError, match="groups"):
                eng.classify(x, top_k=5)
        three = np.concatenate([x, x[:, ::-1], x])
        q3 = eng.classify(three, top_k=0)
        assert np.array_equal(q3[0], q[0]) and np.array_equal(q3[2], q[0]) and not np.array_equal(q3[1], q[0])
        path = str(tmp_path / ("%s_%d.yolohip" % (name, dtype)))
        eng.export(path)
        e2 = hiplib.Engine.from_file(path, max_batch=3)
        assert e2.rows == 0 and e2.num_classes == 24
        assert np.array_equal(e2.classify(three, top_k=0), q3)
        ms = eng.time_layers(1, 2)
        assert ms.shape == (len(secs),) and np.isfinite(ms).all()
        e2.close(); eng.close()


# ---- check 7: the darknet veneer against libdarknet ----
class IMAGE(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


@pytest.mark.parametrize("name,logit_layer", [("mini_cls53", 7), ("mini_cls19", 8)])
def test_veneer_classify_matches_libdarknet(hiplib, tmp_path, name, logit_layer):
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")
    from yolo_tensorflow_amd import darknet_hip as DH
    os.environ["DARKNET_HIP_DTYPE"] = "fp32"
    g = golden(name + ".npz")
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(g["cfg"])); IO.write_weights_file(wf, g["weights"], 0, 2)
    names_file = str(tmp_path / "cls.names"); open(names_file, "w").write("".join("class%02d\n" % i for i in range(24)))
    data_file = str(tmp_path / "cls.data"); open(data_file, "w").write("classes = 24\nnames = %s\n" % names_file)
    ref = DR.lib()
    ref.network_predict_image.argtypes = [C.c_void_p, IMAGE]; ref.network_predict_image.restype = C.POINTER(C.c_float)
    with DR._Quiet():
        rnet = ref.load_network(cfg.encode(), wf.encode(), 0)
        ref.set_batch_network(rnet, 1)
    net = DH.load_net(cfg, wf)
    meta = DH.load_meta(data_file)
    assert meta.classes == 24
    try:
        for w, h in ((200, 120), (96, 250)):
            img = np.ascontiguousarray(np.random.default_rng(w * 7 + h).random((3, h, w), dtype=np.float32))
            want = np.ctypeslib.as_array(ref.network_predict_image(rnet, IMAGE(w, h, 3, img.ctypes.data_as(C.POINTER(C.c_float)))), shape=(24,)).copy()
            n_logits = ref.ref_layer_outputs(rnet, logit_layer)
            max_logit = float(np.abs(np.ctypeslib.as_array(ref.ref_layer_output(rnet, logit_layer), shape=(n_logits,))).max())
            im = DH.IMAGE(w, h, 3, img.ctypes.data_as(C.POINTER(C.c_float)))
            got = np.ctypeslib.as_array(DH.predict_image(net, im), shape=(24,)).copy()
            err = np.abs(got.astype(np.float64) - want)
            print("%s %dx%d: max err / bound %.3f" % (name, w, h, float((err / _prob_bound(want, 2e-4, max_logit)).max())))
            assert (err <= _prob_bound(want, 2e-4, max_logit)).all()
            num = C.c_int(-1)
            dets = DH._load().get_network_boxes(net, w, h, 0.5, 0.5, None, 0, C.byref(num))
            assert num.value == 0 and bool(dets)
            DH._load().free_detections(dets, num.value)
            num = C.c_int(-1)
            dets = DH._load().make_network_boxes(net, 0.5, C.byref(num))
            assert num.value == 0 and bool(dets)
            DH._load().free_detections(dets, num.value)
            res = DH.classify(net, meta, im)
            assert len(res) == 24
            order = np.argsort(-got, kind="stable")
            assert [r[0] for r in res] == [b"class%02d" % int(k) for k in order]
            assert np.array_equal(np.array([r[1] for r in res], dtype=np.float32), got[order])
    finally:
        DH.free_net(net)
        ref.free_network(rnet)


# ---- check 8: full-size classifiers ----
def _jpgs():
    from PIL import Image
    return [np.ascontiguousarray(np.asarray(Image.open(os.path.join(IMG_DIR, n)).convert("RGB"))) for n in JPGS]


@pytest.mark.parametrize("name", ["darknet53", "darknet19"])
def test_full_size_classifier(hiplib, name):
    from yolo_tensorflow_amd.classifier import Classifier
    imgs = _jpgs()
    clf = Classifier(name, dtype=hiplib.BF16, max_batch=8)
    assert clf.num_classes == 1000 and clf.engine.size == 256
    recs = clf.classify_from_images(imgs, top=5)
    assert len(recs) == 6 and all(len(r) == 5 for r in recs)
    full = clf.engine.classify_images(imgs, fit=hiplib.FIT_STRETCH, top_k=0)
    assert full.shape == (6, 1000) and np.abs(full.astype(np.float64).sum(axis=1) - 1).max() <= 1e-5
    for b, r in enumerate(recs):
        probs = [q for _, q in r]
        assert all(0.0 < q <= 1.0 for q in probs) and probs == sorted(probs, reverse=True)
        want = np.argsort(-full[b], kind="stable")[:5]
        assert [k for k, _ in r] == [int(k) for k in want]
        assert probs == [float(q) for q in full[b][want]]
        assert clf.classify_from_image(imgs[b], top=5) == r
    assert len(set(tuple(k for k, _ in r) for r in recs)) > 1 or not np.array_equal(full[0], full[1])      # the images are told apart
    clf.close()


def test_classifier_names(hiplib):
    g = golden("mini_cls19.npz")
    from yolo_tensorflow_amd.classifier import Classifier
    names = ["n%d" % i for i in range(24)]
    clf = Classifier(str(g["cfg"]), dtype=hiplib.FP32, names=names)
    clf.engine.set_weights(g["weights"])
    r = clf.classify_from_image(g["image_u8"], top=3)
    want = np.argsort(-g["output"], kind="stable")[:3]
    assert [k for k, _ in r] == [names[k] for k in want]
    clf.close()


# ---- check 9: refusals ----
def test_refusals(hiplib):
    g = golden("mini_cls19.npz")
    cfg = str(g["cfg"])
    with pytest.raises(hiplib.YoloError, match="tree"):
        hiplib.Engine(cfg.replace("[softmax]\n", "[softmax]\ntree=imagenet.tree\n"))
    with pytest.raises(hiplib.YoloError, match="spatial"):
        hiplib.Engine(cfg.replace("[softmax]\n", "[softmax]\nspatial=1\n"))
    with pytest.raises(hiplib.YoloError, match="fp8"):
        hiplib.Engine(cfg, dtype=hiplib.FP8)
    with pytest.raises(hiplib.YoloError, match="no \\[yolo\\] / \\[region\\] / \\[detection\\] head"):
        hiplib.Engine(cfg[:cfg.index("[avgpool]")])          # neither a head nor a softmax: as before
    eng = hiplib.Engine(cfg, max_batch=2, dtype=hiplib.BF16)
    eng.set_weights(g["weights"])
    x = g["image_u8"][None]
    with pytest.raises(hiplib.YoloError, match="classifier"):
        eng.detect(x)
    eng.classify(x)
    with pytest.raises(hiplib.YoloError, match="classifier"):
        eng.postprocess(1)
    with pytest.raises(hiplib.YoloError, match="classifier"):
        eng.detect_images([g["image_u8"]])
    with pytest.raises(hiplib.YoloError, match="classifier"):
        eng.darknet_boxes(0, 64, 64)
    with pytest.raises(hiplib.YoloError, match="top_k"):
        eng.classify(x, top_k=25)
    with pytest.raises(hiplib.YoloError, match="top_k"):
        eng.classify(x, top_k=33)
    eng.close()
    det = hiplib.Engine(IO.with_input_size(IO.cfg_text("yolov3-tiny"), 96), max_batch=1)
    assert det.num_classes == det.attrs - 5 == 80
    det.set_weights(IO.synth_weights(IO.parse_cfg(IO.with_input_size(IO.cfg_text("yolov3-tiny"), 96)), seed=0))
    with pytest.raises(hiplib.YoloError, match="detector"):
        det.classify(np.zeros((1, 96, 96, 3), dtype=np.uint8))
    det.close()
