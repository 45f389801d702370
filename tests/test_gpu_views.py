"""Multi-view classification on the device (yolo_classify_views_u8, yolo_op_view_reduce) against tests/golden/views_cases.npz: the
compiled reference's ten crops / mirror, its per-view network_predict rows, their axpy_cpu sum and its top_k (tools/make_views_golden.py)."""
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
from tests.test_views_host import V, bits
from tests.test_gpu_classifier import _prob_bound, _dtypes, _bf16, _jpgs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CASES = {c[0]: c for c in V.CASES}
MODE = {V.FLIP: "VIEWS_FLIP", V.TEN_CROP: "VIEWS_TEN_CROP"}


@pytest.fixture(scope="module")
def G():
    return golden("views_cases.npz")


@pytest.fixture(scope="module")
def treedir(tmp_path_factory, G):
    d = tmp_path_factory.mktemp("views_tree")
    (d / V.TREE_FILE).write_text(str(G["tree_text"]))
    return d


def make_engine(hiplib, G, treedir, net, max_batch, dtype):
    """the fixture's network `net` as the library reads it: planes cfgs get their yolo_input key, the tree cfg its tree's full path"""
    cfg = IO.with_planes_input(str(G[net + "_cfg"])).replace("tree=" + V.TREE_FILE, "tree=" + str(treedir / V.TREE_FILE))
    eng = hiplib.Engine(cfg, max_batch=max_batch, dtype=dtype, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(G[net + "_weights"])
    if net == "tree":
        eng.set_hierarchy_mode("leaves")          # classifier.c:287: hierarchy_predictions(.., only_leaves = 1, ..)
    return eng


def run_case(hiplib, eng, G, case, **kw):
    _, _, mode, shift, _, _ = CASES[case]
    return eng.classify_views([G[case + "_image_u8"]], getattr(hiplib, MODE[mode]), fit=hiplib.FIT_STRETCH, shift=shift, **kw)


def _stored(x, dtype, hiplib):
    return _bf16(x) if dtype == hiplib.BF16 else x.astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else x


# ---- 1: the staged views ----
@pytest.mark.parametrize("net", ["rgb", "grey", "rgbd", "tree"])
def test_staged_views_equal_the_reference_images(hiplib, G, treedir, net):
    """One step holds every slot (max_batch >= K): slot v of the staged input is the reference's view v, bit for bit in fp32, rounded to the type in bf16 / fp16;
    the channels past the image's own are zero."""
    for dtype in (hiplib.FP32, hiplib.BF16, hiplib.FP16):
        eng = make_engine(hiplib, G, treedir, net, 10, dtype)
        for case in (c[0] for c in V.CASES if c[1] == net):
            run_case(hiplib, eng, G, case)
            want = G[case + "_views"]
            K, ch = want.shape[0], want.shape[3]
            got = eng.staged_input(K)
            assert got.shape[:3] == want.shape[:3] and got.shape[3] == (ch + 7) // 8 * 8
            assert np.array_equal(bits(got[..., :ch]), bits(_stored(want, dtype, hiplib))), "%s dtype %d" % (case, dtype)
            assert not got[..., ch:].any()
        eng.close()


def test_flip_mirrors_every_fit(hiplib, G, treedir):
    """slot 1 equals slot 0 mirrored, bit for bit, whatever fitted slot 0; slot 0 is the fit's own image"""
    img = G["flip_rgb_image_u8"]
    eng = make_engine(hiplib, G, treedir, "rgb", 2, hiplib.FP32)
    for fit in (hiplib.FIT_STRETCH, hiplib.FIT_LETTERBOX, hiplib.FIT_CV2, hiplib.FIT_CV2_BGR, hiplib.FIT_CENTER_CROP):
        eng.classify_images([img], fit=fit, top_k=0)
        alone = eng.staged_input(1)[0]
        eng.classify_views([img], hiplib.VIEWS_FLIP, fit=fit)
        got = eng.staged_input(2)
        assert np.array_equal(bits(got[0]), bits(alone)), fit
        assert np.array_equal(bits(got[1]), bits(got[0][:, ::-1])), fit
        assert not np.array_equal(got[0], got[1])
    eng.close()
    grey = G["flip_grey_image_u8"]
    eng = make_engine(hiplib, G, treedir, "grey", 2, hiplib.FP32)
    for fit in (hiplib.FIT_STRETCH, hiplib.FIT_LETTERBOX, hiplib.FIT_CENTER_CROP):
        eng.classify_views([grey], hiplib.VIEWS_FLIP, fit=fit)
        got = eng.staged_input(2)
        assert np.array_equal(bits(got[1]), bits(got[0][:, ::-1])), fit
    eng.close()


# ---- 2: the sums against the compiled reference ----
@pytest.mark.parametrize("net", ["rgb", "grey", "rgbd", "tree"])
def test_sums_match_the_compiled_reference(hiplib, G, treedir, net):
    """|sum - reference sum| <= sum over the views of _prob_bound(p_ref_v, tol, max|logit_v|) + K 2^-24 sum: K values, each within its own bound, and K
    rounded additions.  In fp32 the top-5 classes are the reference's: the fixture's 5th and 6th sums are more than twice that bound apart."""
    top = int(G["top"])
    for dtype, tol in _dtypes(hiplib):
        if dtype == hiplib.FP16X2 and net in ("grey", "rgbd"):
            continue          # a network of planes plans in fp32, bf16 and fp16 (include/yolo_hip.h): there is no split-fp16 context to run
        eng = make_engine(hiplib, G, treedir, net, 4, dtype)          # (4 slots per step: an image's ten views span three steps)
        for case in (c[0] for c in V.CASES if c[1] == net):
            rows, ref = G[case + "_rows"], G[case + "_sum"]
            got = run_case(hiplib, eng, G, case)
            assert got.shape == (1, ref.size)
            bound = V.sum_bound(rows, ref, G[case + "_max_logit"], tol)
            assert np.array_equal(bound, sum(_prob_bound(rows[v], tol, G[case + "_max_logit"][v]) for v in range(rows.shape[0])) + rows.shape[0] * U * np.abs(ref.astype(np.float64)))
            err = np.abs(got[0].astype(np.float64) - ref)
            print("%s dtype %d: max err / bound %.3f" % (case, dtype, float((err / bound).max())))
            assert (err <= bound).all(), "%s dtype %d: %g over the bound" % (case, dtype, float((err - bound).max()))
            if dtype == hiplib.FP32:
                cls, val = run_case(hiplib, eng, G, case, top_k=top)
                assert np.array_equal(cls[0], G[case + "_topk"]), case
                assert np.array_equal(bits(val[0]), bits(got[0][cls[0]]))
        eng.close()


# ---- 3: the reduction is exact ----
@pytest.mark.parametrize("dtype_name", ["FP32", "BF16"])
def test_device_sum_is_the_sequential_sum_of_the_device_rows(hiplib, G, treedir, dtype_name):
    dtype = getattr(hiplib, dtype_name)
    for net, case in (("rgb", "s5_odd"), ("rgbd", "rgbd_s32"), ("tree", "tree_s5"), ("grey", "flip_grey")):
        eng = make_engine(hiplib, G, treedir, net, 10, dtype)
        rows = eng.classify(np.ascontiguousarray(G[case + "_views"]), top_k=0, scale=1.0)          # the fixture's views as pre-made inputs
        s = np.zeros(rows.shape[1], np.float32)
        for r in rows:
            s = s + r
        got = run_case(hiplib, eng, G, case)
        assert np.array_equal(bits(got[0]), bits(s)), case
        K = rows.shape[0]
        mean = run_case(hiplib, eng, G, case, scale=1.0 / K)
        assert np.array_equal(bits(mean[0]), bits(s * np.float32(1.0 / K))), case
        eng.close()


# ---- 4: independence from max_batch ----
def test_result_does_not_depend_on_max_batch(hiplib, G, treedir):
    imgs = [G[c + "_image_u8"] for c in ("s5_larger", "s5_exact", "s5_odd")]
    seen = []
    for mb in (1, 3, 7, 32):
        eng = make_engine(hiplib, G, treedir, "rgb", mb, hiplib.BF16)
        sums = eng.classify_views(imgs, hiplib.VIEWS_TEN_CROP, shift=5)
        cls, val = eng.classify_views(imgs, hiplib.VIEWS_TEN_CROP, shift=5, top_k=5)
        again = eng.classify_views(imgs, hiplib.VIEWS_TEN_CROP, shift=5)
        assert np.array_equal(bits(sums), bits(again))          # run to run
        seen.append((sums, cls, val))
        eng.close()
    for sums, cls, val in seen[1:]:
        assert np.array_equal(bits(sums), bits(seen[0][0])) and np.array_equal(cls, seen[0][1]) and np.array_equal(bits(val), bits(seen[0][2]))
    # each image is what it is alone
    eng = make_engine(hiplib, G, treedir, "rgb", 4, hiplib.BF16)
    for i, im in enumerate(imgs):
        assert np.array_equal(bits(eng.classify_views([im], hiplib.VIEWS_TEN_CROP, shift=5)[0]), bits(seen[0][0][i]))
    eng.close()


# ---- 5: the reduction launch alone ----
SOFTMAX_ROW_MAX = 8192          # the planner's largest [softmax] row with groups=1 (CLS_SOFTMAX_MAX)


def _reduce_inputs(kind, n, views, length):
    rng = np.random.default_rng(1000 * views + length + n)
    if kind == "eighths":          # multiples of 1/8: every partial sum is exact, and the sums tie at every level
        return (rng.integers(0, 9, (n * views, length)) / 8.0).astype(np.float32)
    if kind == "equal":
        return np.full((n * views, length), 0.375, np.float32)
    x = rng.uniform(0.5, 1.0, (n * views, length)).astype(np.float32)          # magnitudes 2^20 apart: any other order of additions changes bits
    x[rng.random((n * views, length)) < 0.5] *= np.float32(2.0 ** 20)
    return x


@pytest.mark.parametrize("length", [1, 33, 1000, SOFTMAX_ROW_MAX])
@pytest.mark.parametrize("views", [1, 2, 10, 32])
def test_op_view_reduce(hiplib, views, length):
    for n in (1, 3):
        for kind in ("eighths", "equal", "wide"):
            x = _reduce_inputs(kind, n, views, length)
            want = np.zeros((n, length), np.float32)
            for v in range(views):
                want = want + x.reshape(n, views, length)[:, v]
            got = hiplib.op_view_reduce(x, views)
            assert np.array_equal(bits(got), bits(want)), (kind, n)          # scale = 1 leaves the bits alone
            scaled = want * np.float32(1.0 / views)
            assert np.array_equal(bits(hiplib.op_view_reduce(x, views, scale=1.0 / views)), bits(scaled)), (kind, n)
            for k in sorted({1, min(5, length), min(32, length)}):
                sums, cls, top = hiplib.op_view_reduce(x, views, scale=1.0 / views, top_k=k)
                assert np.array_equal(bits(sums), bits(scaled))
                for b in range(n):
                    order = np.argsort(-scaled[b], kind="stable")[:k]
                    assert np.array_equal(cls[b], order.astype(np.int32)), (kind, n, k, b)
                    assert np.array_equal(bits(top[b]), bits(scaled[b][order]))


def test_op_view_reduce_ranks_negative_sums(hiplib):
    x = np.array([[-1.0, -3.0, 0.5, -1.0], [-1.0, 1.0, -2.5, -1.0]], np.float32)
    sums, cls, top = hiplib.op_view_reduce(x, 2, top_k=4)
    assert list(sums[0]) == [-2.0, -2.0, -2.0, -2.0] and list(cls[0]) == [0, 1, 2, 3]
    sums, cls, top = hiplib.op_view_reduce(x, 1, top_k=3)
    assert list(cls[0]) == [2, 0, 3] and list(cls[1]) == [1, 0, 3] and list(top[1]) == [1.0, -1.0, -1.0]


# ---- 6: refusals ----
RECURRENT_CLS = ("[net]\nbatch=1\nwidth=32\nheight=32\nchannels=3\ntime_steps=1\n\n[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=2\npad=1\nactivation=leaky\n\n"
                 "[crnn]\nhidden_filters=8\noutput_filters=8\nactivation=leaky\nbatch_normalize=1\n\n"
                 "[convolutional]\nfilters=6\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")


def _refused(hiplib, eng, code, *needles, images=None, views=None, **kw):
    images = [np.zeros((9, 11, eng.input_channels), np.uint8)] if images is None else images
    with pytest.raises(hiplib.YoloError) as e:
        eng.classify_views(images, hiplib.VIEWS_TEN_CROP if views is None else views, **kw)
    msg = str(e.value)
    assert "(%d)" % code in msg, msg
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals(hiplib, G, treedir):
    INVALID, UNSUPPORTED = -1, -6
    # a detector, a map network, a vector-input network: no classifier output to add
    det = hiplib.Engine(IO.with_input_size(IO.cfg_text("yolov3-tiny"), 96), max_batch=1)
    _refused(hiplib, det, INVALID, "detector")
    det.close()
    seg = hiplib.Engine(str(golden("mini_unet.npz")["cfg"]), max_batch=1, semantics=hiplib.SEM_DARKNET)
    _refused(hiplib, seg, INVALID, "map network")
    seg.close()
    vec = hiplib.Engine(str(golden("mini_char_rnn.npz")["cfg"]), max_batch=1, semantics=hiplib.SEM_DARKNET)
    _refused(hiplib, vec, INVALID, "vector-input", images=[np.zeros((9, 11, 3), np.uint8)])
    vec.close()
    # recurrent state: a batch slot is a stream there
    rec = hiplib.Engine(RECURRENT_CLS, max_batch=2, semantics=hiplib.SEM_DARKNET)
    assert rec.num_state_tensors > 0
    _refused(hiplib, rec, UNSUPPORTED, "yolo_classify_views_u8", "recurrent state", "stream")
    rec.close()
    # fp8 plans no [softmax]: such a context cannot exist, the entry point's own fp8 refusal stands behind the planner's
    rc, msg = hiplib.plan_check(str(G["rgb_cfg"]), dtype=hiplib.FP8)
    assert rc == UNSUPPORTED and "fp8" in msg
    # a classifier: every other refusal leaves the last forward as it was
    eng = make_engine(hiplib, G, treedir, "rgb", 2, hiplib.FP32)
    img = G["s5_odd_image_u8"]
    eng.classify_images([img], top_k=0)
    before = (eng.last_layer_output(1).copy(), eng.staged_input(1).copy())
    _refused(hiplib, eng, INVALID, "views", views=0)
    _refused(hiplib, eng, INVALID, "views", views=3)
    _refused(hiplib, eng, INVALID, "shift", shift=-1)
    _refused(hiplib, eng, INVALID, "shift", views=hiplib.VIEWS_FLIP, shift=-1)
    _refused(hiplib, eng, INVALID, "top_k", top_k=25)
    _refused(hiplib, eng, INVALID, "top_k", top_k=-1)
    _refused(hiplib, eng, INVALID, "bad fit", views=hiplib.VIEWS_FLIP, fit=9)
    buf, descs = hiplib.pack_images([img, img])
    bad = descs.copy(); bad[1]["h"] += 1
    _refused(hiplib, eng, INVALID, "image 1", "end past", images=(buf, bad))
    bad = descs.copy(); bad[0]["w"] = 0
    _refused(hiplib, eng, INVALID, "image 0", images=(buf, bad))
    assert np.array_equal(eng.last_layer_output(1), before[0]) and np.array_equal(eng.staged_input(1), before[1])
    eng.close()
    # W' < 2 or H' < 2: resize_image divides by the extent - 1
    one = hiplib.Engine("[net]\nbatch=1\nwidth=1\nheight=3\nchannels=3\n\n[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n",
                        max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    _refused(hiplib, one, INVALID, "less than 2 pixels", shift=0)
    _refused(hiplib, one, INVALID, "does not fit an int", shift=2 ** 31 - 1)
    one.close()
    # the cv2 fits mean an RGB / BGR image
    grey = make_engine(hiplib, G, treedir, "grey", 2, hiplib.FP32)
    for fit, name in ((hiplib.FIT_CV2, "YOLO_FIT_CV2"), (hiplib.FIT_CV2_BGR, "YOLO_FIT_CV2_BGR")):
        _refused(hiplib, grey, UNSUPPORTED, "yolo_classify_views_u8", name, "1 planes", views=hiplib.VIEWS_FLIP, fit=fit)
    grey.classify_views([G["grey_s5_image_u8"]], hiplib.VIEWS_TEN_CROP, fit=hiplib.FIT_CV2, shift=5)          # TEN_CROP does not read `fit`
    grey.close()


# ---- 7: the package level ----
def test_classifier_ten_crop_on_darknet19(hiplib):
    from yolo_tensorflow_amd.classifier import Classifier
    imgs = _jpgs()
    clf = Classifier("darknet19", dtype=hiplib.BF16, max_batch=4)
    recs = clf.classify_from_images(imgs, top=5, views="ten_crop")
    assert len(recs) == 6 and all(len(r) == 5 for r in recs)
    cls, val = clf.engine.classify_views(imgs, hiplib.VIEWS_TEN_CROP, shift=32, scale=1.0 / 10, top_k=5)
    for b, r in enumerate(recs):
        probs = [q for _, q in r]
        assert all(0.0 < q <= 1.0 for q in probs) and probs == sorted(probs, reverse=True)
        assert [k for k, _ in r] == [int(k) for k in cls[b]] and probs == [float(q) for q in val[b]]
    flip = clf.classify_from_images(imgs[:2], top=3, views="flip")
    assert len(flip) == 2 and all(len(r) == 3 for r in flip)
    assert clf.classify_from_images(imgs[:2], top=3) == clf.classify_from_images(imgs[:2], top=3, views=None)
    with pytest.raises(hiplib.YoloError, match="views"):
        clf.classify_from_images(imgs[:1], views="five_crop")
    clf.close()
