"""Classifiers and segmenters over decoded video frames and JPEG files on the device: yolo_classify_frames_u8, yolo_classify_views_frames_u8,
yolo_segment_frames_u8 and their JPEG forms against the project's own image path over the RGB bytes hip.frame_to_rgb / hip.jpeg_to_rgb return on the host --
bit for bit everywhere (the colour and JPEG rules are integer-exact, the px_* arithmetic is shared): the staged network input of every fit and every view,
probabilities, sums and top-k records, labels, the class methods, and every refusal before any launch.  Floats are compared as uint32."""
import ctypes as C
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_frames_host as FH
import test_jpeg_host as JH
from test_gpu_views import make_engine

pytestmark = pytest.mark.gpu

NV12, I420, RGB24, BGR24 = FH.NV12, FH.I420, FH.RGB24, FH.BGR24
# (h, w): where the chroma edge rules and the resize end points can go wrong, and one frame larger than every network input used here
SIZES = [(1, 1), (1, 2), (3, 5), (17, 9), (50, 35), (70, 90)]
# one file of each served kind at odd sizes: grey, 4:4:4, 4:2:2, 4:2:0, 4:4:0, and the 1 x 1 and 50 x 35 ends of 4:2:0
FILES = ["g23x19", "c33x31_444_opt", "c17x9_422_rst1", "c17x9_420_std", "c7x5_440_rst1", "c1x1_420_std", "c50x35_420_q10"]
FITS = ["FIT_STRETCH", "FIT_LETTERBOX", "FIT_CV2", "FIT_CENTER_CROP"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _kinds():
    """NV12, I420, RGB24 and BGR24 under each matrix"""
    return [(fmt, m) for m in FH.MATRICES for fmt in (NV12, I420, RGB24, BGR24)]


def _frame(rng, h, w, fmt, matrix=FH.MATRICES[0]):
    return FH.make_frame(rng, h, w, fmt, matrix, y_extra=1 if fmt in (RGB24, BGR24) else 3)


def _mixed(rng):
    """twelve frames: every (format, matrix) kind once, the sizes in rotation -- pitches above the row, planes reversed, 0xFF between samples"""
    return [_frame(rng, *SIZES[i % len(SIZES)], fmt, m) for i, (fmt, m) in enumerate(_kinds())]


def _rgbs(hip, frames):
    out = [hip.frame_to_rgb(f) for f in frames]
    for f, rgb in zip(frames, out):
        assert np.array_equal(rgb, FH.ref_of(f))
    return out


def _files():
    return [JH.path_of(n) for n in FILES]


def _cls19(hip, dtype, max_batch=12):
    g = golden("mini_cls19.npz")
    e = hip.Engine(str(g["cfg"]), max_batch=max_batch, dtype=dtype, semantics=hip.SEM_DARKNET)
    e.set_weights(g["weights"])
    return e


def _unet(hip, dtype=None, max_batch=3):
    g = golden("mini_unet.npz")
    e = hip.Engine(str(g["cfg"]), max_batch=max_batch, dtype=hip.FP32 if dtype is None else dtype, semantics=hip.SEM_DARKNET)
    e.set_weights(g["weights"])
    return e, float(np.median(g["layer_11"].max(axis=-1)))          # about half of the fixture's pixels are below it: both outcomes occur


@pytest.fixture(scope="module")
def G():
    return golden("views_cases.npz")


@pytest.fixture(scope="module")
def treedir(tmp_path_factory, G):
    from tests.test_views_host import V
    d = tmp_path_factory.mktemp("classify_frames_tree")
    (d / V.TREE_FILE).write_text(str(G["tree_text"]))
    return d


# ---- 1: staged input, whole frames ----
@pytest.mark.parametrize("dtype", ["FP32", "BF16", "FP16"])
def test_staged_input_of_frames_and_files_equals_that_of_the_restated_rgb(hiplib, dtype):
    rng = np.random.default_rng(241)
    e = _cls19(hiplib, getattr(hiplib, dtype))
    frames = _mixed(rng)
    sources = [(e.classify_frames, frames, _rgbs(hiplib, frames)), (e.classify_jpegs, _files(), [hiplib.jpeg_to_rgb(p) for p in _files()])]
    for fit in FITS:
        fit_id = getattr(hiplib, fit)
        for call, src, rgbs in sources:
            n = len(src)
            e.classify_images(rgbs, fit=fit_id, top_k=0)
            want = e.staged_input(n)
            e.classify(np.zeros((n, 64, 64, 3), np.uint8), top_k=0)          # (so that nothing of `want` is left staged)
            call(src, fit=fit_id, top_k=0)
            got = e.staged_input(n)
            assert want.shape == (n, 64, 64, 8) and want[..., :3].any() and not got[..., 3:].any()
            for i in range(n):
                assert np.array_equal(bits(got[i]), bits(want[i])), (dtype, fit, call.__name__, i)
    e.close()


# ---- 2: probabilities and top-k ----
def test_probabilities_and_top_k_equal_classify_images(hiplib):
    rng = np.random.default_rng(242)
    frames = _mixed(rng)
    for dtype in (hiplib.BF16, hiplib.FP32):
        e = _cls19(hiplib, dtype)
        for call, src, rgbs in ((e.classify_frames, frames, _rgbs(hiplib, frames)), (e.classify_jpegs, _files(), [hiplib.jpeg_to_rgb(p) for p in _files()])):
            for fit in (hiplib.FIT_STRETCH, hiplib.FIT_CENTER_CROP):
                want = e.classify_images(rgbs, fit=fit, top_k=0)
                got = call(src, fit=fit, top_k=0)
                assert got.shape == (len(src), 24) and np.array_equal(bits(got), bits(want)), (call.__name__, fit)
                wc, wp = e.classify_images(rgbs, fit=fit, top_k=5)
                gc, gp = call(src, fit=fit, top_k=5)
                assert np.array_equal(gc, wc) and np.array_equal(bits(gp), bits(wp)), (call.__name__, fit)
                assert len({tuple(r) for r in got.round(6).tolist()}) > 1          # the pictures are told apart
        e.close()


# ---- 3: views, staged ----
def _view_sources(hip, rng, shift):
    """[(what, frames-or-files call name, source, rgb)]: an odd NV12 frame and an odd 4:2:0 file (a mirror must move them), the other formats, and one source
    of exactly W' x H' = (24 + shift) x (20 + shift), where resize_image is the identity"""
    out = []
    for what, f in (("nv12_odd", _frame(rng, 17, 9, NV12, FH.MATRICES[1])), ("i420", _frame(rng, 50, 35, I420, FH.MATRICES[2])), ("bgr", _frame(rng, 3, 5, BGR24)),
                    ("nv12_1x2", _frame(rng, 1, 2, NV12)), ("exact", _frame(rng, 20 + shift, 24 + shift, NV12))):
        out.append((what, "frames", f, hip.frame_to_rgb(f)))
    for name in ("c17x9_420_std", "c33x31_444_opt", "g23x19", "c1x1_420_std", "c7x5_440_rst1", "c17x9_422_rst1"):
        out.append((name, "jpegs", JH.path_of(name), hip.jpeg_to_rgb(JH.path_of(name))))
    return out


def _views_call(e, kind, src, *a, **kw):
    return (e.classify_views_frames if kind == "frames" else e.classify_views_jpegs)([src], *a, **kw)


@pytest.mark.parametrize("dtype", ["FP32", "BF16"])
def test_staged_views_equal_those_of_the_restated_rgb(hiplib, G, treedir, dtype):
    rng = np.random.default_rng(243)
    e = make_engine(hiplib, G, treedir, "rgb", 10, getattr(hiplib, dtype))          # max_batch >= K: one step holds an image's views
    MOVED = ("nv12_odd", "c17x9_420_std")
    for fit in FITS:
        fit_id = getattr(hiplib, fit)
        for what, kind, src, rgb in _view_sources(hiplib, rng, 5):
            e.classify_views([rgb], hiplib.VIEWS_FLIP, fit=fit_id)
            want = e.staged_input(2)
            e.classify(np.zeros((2, 20, 24, 3), np.uint8), top_k=0)
            _views_call(e, kind, src, hiplib.VIEWS_FLIP, fit=fit_id)
            got = e.staged_input(2)
            assert np.array_equal(bits(got), bits(want)), (dtype, fit, what)
            assert np.array_equal(bits(got[1]), bits(got[0][:, ::-1]))
            if what in MOVED:
                assert not np.array_equal(got[0], got[1]), (fit, what)
    for shift in (0, 5):
        for what, kind, src, rgb in _view_sources(hiplib, rng, shift):
            if what == "exact":
                assert rgb.shape == (20 + shift, 24 + shift, 3)
            e.classify_views([rgb], hiplib.VIEWS_TEN_CROP, shift=shift)
            want = e.staged_input(10)
            e.classify(np.zeros((10, 20, 24, 3), np.uint8), top_k=0)
            _views_call(e, kind, src, hiplib.VIEWS_TEN_CROP, shift=shift)
            got = e.staged_input(10)
            assert want[..., :3].any() and np.array_equal(bits(got), bits(want)), (dtype, shift, what)
            if what in MOVED:
                for v in range(5):
                    assert not np.array_equal(got[v], got[v + 5]), (shift, what, v)
    e.close()


# ---- 4: views, sums ----
@pytest.mark.parametrize("net", ["rgb", "tree"])
def test_view_sums_equal_classify_views_and_do_not_depend_on_max_batch(hiplib, G, treedir, net):
    """three pictures of mixed formats at max_batch = 4: one picture's ten views span steps, pictures share a step"""
    rng = np.random.default_rng(244)
    frames = [_frame(rng, 17, 9, NV12, FH.MATRICES[1]), _frame(rng, 50, 35, I420, FH.MATRICES[2]), _frame(rng, 25, 29, BGR24)]
    files = [JH.path_of(n) for n in ("c17x9_420_std", "g23x19", "c50x35_422_rst3")]
    rgb_frames, rgb_files = [hiplib.frame_to_rgb(f) for f in frames], [hiplib.jpeg_to_rgb(p) for p in files]
    seen = {}
    for mb in (4, 10):
        e = make_engine(hiplib, G, treedir, net, mb, hiplib.BF16)
        for key, got_call, src, rgbs in (("frames", e.classify_views_frames, frames, rgb_frames), ("jpegs", e.classify_views_jpegs, files, rgb_files)):
            for views, shift in ((hiplib.VIEWS_TEN_CROP, 5), (hiplib.VIEWS_FLIP, 0)):
                want = e.classify_views(rgbs, views, fit=hiplib.FIT_CENTER_CROP, shift=shift)
                got = got_call(src, views, fit=hiplib.FIT_CENTER_CROP, shift=shift)
                assert got.shape == want.shape and want.any() and np.array_equal(bits(got), bits(want)), (net, mb, key, views)
                wc, wv = e.classify_views(rgbs, views, fit=hiplib.FIT_CENTER_CROP, shift=shift, scale=0.1, top_k=5)
                gc, gv = got_call(src, views, fit=hiplib.FIT_CENTER_CROP, shift=shift, scale=0.1, top_k=5)
                assert np.array_equal(gc, wc) and np.array_equal(bits(gv), bits(wv)), (net, mb, key, views)
                if mb == 4:
                    seen[key, views] = (got, gc, gv)
                else:
                    s, c, v = seen[key, views]
                    assert np.array_equal(bits(got), bits(s)) and np.array_equal(gc, c) and np.array_equal(bits(gv), bits(v)), (net, key, views)
        e.close()


# ---- 5: segmentation ----
@pytest.mark.parametrize("fit_name", ["FIT_LETTERBOX", "FIT_STRETCH"])
def test_labels_of_frames_and_files_equal_segment_images(hiplib, fit_name):
    import torch
    fit = getattr(hiplib, fit_name)
    rng = np.random.default_rng(245)
    e, thresh = _unet(hiplib)
    frames = [_frame(rng, 37, 91, NV12, FH.MATRICES[1]), _frame(rng, 12, 20, I420, FH.MATRICES[2]), _frame(rng, 50, 35, BGR24)]          # the second one: exactly the input's size
    files = [JH.path_of(n) for n in ("c17x9_420_std", "c50x35_440_rst3", "g23x19")]
    rgb_frames, rgb_files = [hiplib.frame_to_rgb(f) for f in frames], [hiplib.jpeg_to_rgb(p) for p in files]
    want = e.segment_images(rgb_frames, fit=fit, thresh=thresh)
    assert any((a == 255).any() for a in want) and any((a != 255).any() for a in want)
    buf, descs = hiplib.pack_frames(frames)
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    for src in (frames, (buf, descs), (dev, descs)):          # a list, packed on the host, packed on the device
        got = e.segment_frames(src, fit=fit, thresh=thresh)
        assert [a.shape for a in got] == [r.shape[:2] for r in rgb_frames] and all(a.dtype == np.uint8 for a in got)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    want_files = e.segment_images(rgb_files, fit=fit, thresh=thresh)
    got = e.segment_jpegs(files, fit=fit, thresh=thresh)
    assert [a.shape for a in got] == [r.shape[:2] for r in rgb_files] and all(np.array_equal(a, b) for a, b in zip(got, want_files))
    # placed labels: image i at offsets[i], out of order, with gaps -- which are zeroed
    def placed(rgbs, call):
        sizes = [r.shape[0] * r.shape[1] for r in rgbs]
        offs = np.array([sizes[2] + 13, sizes[2] + 13 + sizes[0] + 5, 3], dtype=np.uint64)
        total = int(offs[1]) + sizes[1]
        out = np.full(total + 8, 7, np.uint8)
        e._check(call(out, offs), "segment with label_offsets")
        assert (out[total:] == 7).all()
        return out, offs, sizes
    ibuf, idescs = hiplib.pack_images(rgb_frames)
    want_buf, offs, sizes = placed(rgb_frames, lambda out, offs: e.lib.yolo_segment_images_u8(e.ctx, ibuf.ctypes.data, idescs.ctypes.data, 3, fit, thresh, out.ctypes.data, offs.ctypes.data))
    for i in range(3):
        assert np.array_equal(want_buf[int(offs[i]):int(offs[i]) + sizes[i]], want[i].reshape(-1))
    assert not want_buf[:3].any() and not want_buf[3 + sizes[2]:sizes[2] + 13].any()
    for p, loc in ((buf.ctypes.data, hiplib.HOST), (C.c_void_p(dev.data_ptr()), hiplib.DEVICE)):
        got_buf, _, _ = placed(rgb_frames, lambda out, offs: e.lib.yolo_segment_frames_u8(e.ctx, p, buf.size, descs.ctypes.data, 3, fit, loc, thresh, out.ctypes.data, offs.ctypes.data))
        assert np.array_equal(got_buf, want_buf), loc
    jf = hiplib._JpegFiles(files)
    ibuf, idescs = hiplib.pack_images(rgb_files)
    want_buf, _, _ = placed(rgb_files, lambda out, offs: e.lib.yolo_segment_images_u8(e.ctx, ibuf.ctypes.data, idescs.ctypes.data, 3, fit, thresh, out.ctypes.data, offs.ctypes.data))
    got_buf, _, _ = placed(rgb_files, lambda out, offs: e.lib.yolo_segment_jpegs(e.ctx, jf.ptrs, jf.sizes, 3, fit, thresh, out.ctypes.data, offs.ctypes.data))
    assert np.array_equal(got_buf, want_buf)
    e.close()


# ---- 6: class methods ----
def test_classifier_and_segmenter_from_files_and_frames(hiplib):
    from yolo_tensorflow_amd.classifier import Classifier
    from yolo_tensorflow_amd.segmenter import Segmenter
    rng = np.random.default_rng(246)
    g = golden("mini_cls19.npz")
    files = [JH.path_of("c50x35_420_std"), JH.path_of("c33x31_444_opt"), JH.path_of("c17x9_422_rst1")]
    rgbs = [hiplib.jpeg_to_rgb(p) for p in files]
    frames = [_frame(rng, 70, 90, NV12), _frame(rng, 17, 9, I420, FH.MATRICES[1]), _frame(rng, 50, 35, RGB24)]
    clf = Classifier(str(g["cfg"]), dtype=hiplib.BF16, max_batch=2, fit=hiplib.FIT_CENTER_CROP, names=["n%d" % i for i in range(24)])          # (three pictures: two chunks)
    clf.engine.set_weights(g["weights"])
    for views in (None, "ten_crop", "flip"):
        want = clf.classify_from_images(rgbs, top=5, views=views)
        assert len(want) == 3 and all(len(r) == 5 and isinstance(r[0][0], str) for r in want)
        assert clf.classify_from_files(files, top=5, views=views) == want, views
        assert clf.classify_from_frames(frames, top=5, views=views) == clf.classify_from_images([hiplib.frame_to_rgb(f) for f in frames], top=5, views=views), views
    assert clf.classify_from_files(files, top=3, views="ten_crop", shift=7) == clf.classify_from_images(rgbs, top=3, views="ten_crop", shift=7)
    with open(files[0], "rb") as fh:
        assert clf.classify_from_files([fh.read()], top=5) == clf.classify_from_images(rgbs[:1], top=5)          # bytes as well as paths
    with pytest.raises(hiplib.YoloError, match="views"):
        clf.classify_from_files(files[:1], views="five_crop")
    clf.close()
    u = golden("mini_unet.npz")
    seg = Segmenter(str(u["cfg"]), u["weights"], max_batch=2, dtype=hiplib.BF16, fit="letterbox")
    want = seg.segment_from_images(rgbs, thresh=0.5)
    got = seg.segment_from_files(files, thresh=0.5)
    assert [a.shape for a in got] == [r.shape[:2] for r in rgbs] and all(np.array_equal(a, b) for a, b in zip(got, want))
    want = seg.segment_from_images([hiplib.frame_to_rgb(f) for f in frames], thresh=0.5)
    got = seg.segment_from_frames(frames, thresh=0.5)
    assert [a.shape for a in got] == [(f.h, f.w) for f in frames] and all(np.array_equal(a, b) for a, b in zip(got, want))
    seg.close()


# ---- 7: refusals ----
def _refused(hip, call, code, *needles):
    with pytest.raises(hip.YoloError) as err:
        call()
    msg = str(err.value)
    assert "(%d)" % code in msg, msg
    for n in needles:
        assert n in msg, (n, msg)


def test_refusals_come_before_any_launch_and_name_what_is_refused(hiplib, G, treedir):
    INVALID, UNSUPPORTED = -1, -6
    rng = np.random.default_rng(247)
    frames = [_frame(rng, 50, 35, I420, FH.MATRICES[1]), _frame(rng, 6, 9, NV12), _frame(rng, 20, 30, BGR24)]
    buf, descs = hiplib.pack_frames(frames)
    bad = descs.copy(); bad[1]["format"] = 4
    good_file, progressive = JH.path_of("c17x9_420_std"), JH.path_of("refused_progressive")
    TEN, FLIP = hiplib.VIEWS_TEN_CROP, hiplib.VIEWS_FLIP
    # a detector has no classifier output and no map
    det = hiplib.Engine(IO.with_input_size(IO.cfg_text("yolov3-tiny"), 96), max_batch=3)
    for call in (lambda: det.classify_frames(frames), lambda: det.classify_views_frames(frames, TEN), lambda: det.classify_jpegs([good_file]),
                 lambda: det.classify_views_jpegs([good_file], FLIP)):
        _refused(hiplib, call, INVALID, "detector")
    _refused(hiplib, lambda: det.segment_frames(frames), INVALID, "yolo_segment_frames_u8", "not a map network", "detector")
    det.close()
    # a map network is no classifier
    seg, thresh = _unet(hiplib)
    _refused(hiplib, lambda: seg.classify_frames(frames), INVALID, "map network")
    _refused(hiplib, lambda: seg.classify_views_jpegs([good_file], TEN), INVALID, "map network")
    want_labels = seg.segment_frames(frames, thresh=thresh)
    staged = seg.staged_input(3)
    _refused(hiplib, lambda: seg.segment_frames((buf, bad), thresh=thresh), INVALID, "frame 1", "format")
    _refused(hiplib, lambda: seg.segment_frames(frames, fit=hiplib.FIT_CV2_BGR), UNSUPPORTED, "YOLO_FIT_CV2_BGR")
    _refused(hiplib, lambda: seg.segment_frames(frames, fit=hiplib.FIT_CENTER_CROP), UNSUPPORTED, "yolo_segment_frames_u8", "YOLO_FIT_CENTER_CROP")
    _refused(hiplib, lambda: seg.segment_jpegs([good_file, progressive]), UNSUPPORTED, "file 1", "progressive")
    _refused(hiplib, lambda: seg.segment_frames(frames + frames[:1]), INVALID, "batch 4")
    assert np.array_equal(bits(seg.staged_input(3)), bits(staged))
    assert all(np.array_equal(a, b) for a, b in zip(seg.segment_frames(frames, thresh=thresh), want_labels))
    seg.close()
    # a classifier: no map; and every refusal of its own entry points leaves the last good call's staging alone
    e = make_engine(hiplib, G, treedir, "rgb", 4, hiplib.FP32)
    _refused(hiplib, lambda: e.segment_frames(frames), INVALID, "yolo_segment_frames_u8", "not a map network", "classifier")
    _refused(hiplib, lambda: e.segment_jpegs([good_file]), INVALID, "yolo_segment_jpegs", "classifier")
    good = e.classify_frames(frames, top_k=0)
    staged = e.staged_input(3)
    good_views = e.classify_views_frames(frames, TEN, shift=5)
    staged_views = e.staged_input(2)          # the last step of 30 slots at 4 per step holds 2
    for call in (lambda **kw: e.classify_frames(frames, **kw), lambda **kw: e.classify_views_frames(frames, FLIP, **kw)):
        _refused(hiplib, lambda: call(fit=hiplib.FIT_CV2_BGR), UNSUPPORTED, "YOLO_FIT_CV2_BGR", "frames")
        _refused(hiplib, lambda: call(fit=9), INVALID, "bad fit")
        _refused(hiplib, lambda: call(top_k=33), INVALID, "top_k 33")
    _refused(hiplib, lambda: e.classify_jpegs([good_file], top_k=33), INVALID, "top_k 33")
    _refused(hiplib, lambda: e.classify_views_jpegs([good_file], TEN, top_k=33), INVALID, "top_k 33")
    _refused(hiplib, lambda: e.classify_jpegs([good_file], fit=hiplib.FIT_CV2_BGR), UNSUPPORTED, "YOLO_FIT_CV2_BGR")
    _refused(hiplib, lambda: e.classify_views_jpegs([good_file], FLIP, fit=hiplib.FIT_CV2_BGR), UNSUPPORTED, "YOLO_FIT_CV2_BGR")
    _refused(hiplib, lambda: e.classify_frames((buf, bad)), INVALID, "frame 1", "format")
    _refused(hiplib, lambda: e.classify_views_frames((buf, bad), TEN), INVALID, "frame 1", "format")
    _refused(hiplib, lambda: e.classify_views_frames((buf, bad), FLIP), INVALID, "frame 1", "format")
    room = np.zeros(3 * e.num_classes, np.float32)          # frame 2 ends past a buffer that holds frames 0 and 1
    _refused(hiplib, lambda: e._check(e.lib.yolo_classify_views_frames_u8(e.ctx, buf.ctypes.data, int(descs["offset"][2, 0]) + 5, descs.ctypes.data, 3, TEN, 0, 5, hiplib.HOST, 1.0, 0,
                                                                          None, room.ctypes.data, hiplib.HOST), "yolo_classify_views_frames_u8"),
             INVALID, "frame 2", "past")
    assert not room.any()
    _refused(hiplib, lambda: e.classify_views_jpegs([good_file, progressive], TEN), UNSUPPORTED, "file 1", "progressive")
    _refused(hiplib, lambda: e.classify_jpegs([good_file, progressive]), UNSUPPORTED, "file 1", "progressive")
    _refused(hiplib, lambda: e.classify_views_frames(frames, 3), INVALID, "views")
    _refused(hiplib, lambda: e.classify_views_frames(frames, TEN, shift=-1), INVALID, "shift")
    _refused(hiplib, lambda: e.classify_frames(frames + frames[:2]), INVALID, "batch 5")
    thin = [_frame(rng, 1, 2000, NV12)]
    _refused(hiplib, lambda: e.classify_views_frames(thin, FLIP, fit=hiplib.FIT_LETTERBOX), INVALID, "frame 0: 1 x 2000 letterboxes")
    assert np.array_equal(bits(e.staged_input(2)), bits(staged_views))          # no refused call launched anything
    e.classify_views_frames(frames + frames, TEN, shift=5)          # six pictures at max_batch 4: the views form is not bound by max_batch
    assert np.array_equal(bits(e.classify_views_frames(frames, TEN, shift=5)), bits(good_views))
    assert np.array_equal(bits(e.staged_input(2)), bits(staged_views))
    _refused(hiplib, lambda: e.classify_views_frames((buf, bad), TEN), INVALID, "frame 1")
    assert np.array_equal(bits(e.staged_input(2)), bits(staged_views))
    assert np.array_equal(bits(e.classify_frames(frames, top_k=0)), bits(good)) and np.array_equal(bits(e.staged_input(3)), bits(staged))
    e.close()
    # W' < 2: resize_image divides by the extent - 1
    one = hiplib.Engine("[net]\nbatch=1\nwidth=1\nheight=3\nchannels=3\n\n[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n",
                        max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    _refused(hiplib, lambda: one.classify_views_frames(frames, TEN, shift=0), INVALID, "less than 2 pixels")
    _refused(hiplib, lambda: one.classify_views_jpegs([good_file], TEN, shift=0), INVALID, "less than 2 pixels")
    one.close()
    # a one-plane network: a frame is an RGB image after its conversion
    grey = make_engine(hiplib, G, treedir, "grey", 4, hiplib.FP32)
    for call in (lambda: grey.classify_frames(frames), lambda: grey.classify_jpegs([good_file])):
        _refused(hiplib, call, UNSUPPORTED, "frames", " 1 planes")
    _refused(hiplib, lambda: grey.classify_views_frames(frames, TEN), UNSUPPORTED, "yolo_classify_views_frames_u8", " 1 planes")
    _refused(hiplib, lambda: grey.classify_views_jpegs([good_file], TEN), UNSUPPORTED, "yolo_classify_views_jpegs", " 1 planes")
    grey.close()
