"""Ragged batches of native-size uint8 images in one device step (yolo_forward_images_u8 / yolo_detect_images_u8 /
yolo_detect_images_graph): every image of a batch equals, bit for bit, the same image run alone through the single-image entry points
(yolo_forward_image_u8, yolo_forward_letterbox_chw) and post-processed; the per-image box mapping equals the reference's host-side
steps (convert_to_original_size, V2 postprocess(image_shape=...), darknet's correct_yolo_boxes)."""
import ctypes as C
import os
import numpy as np
import pytest
from oracle import yolo_ref as R
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG_DIR = os.path.join(ROOT, "tests", "golden", "images")
JPGS = ["dog.jpg", "eagle.jpg", "giraffe.jpg", "horses.jpg", "kite.jpg", "person.jpg"]
S = 160
POST = dict(score_thr=0.3, iou_thr=0.45, max_out=30)


def _load(name):
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(IMG_DIR, name)).convert("RGB")))


_JPG_CACHE = {}


def _jpgs():
    if not _JPG_CACHE:
        _JPG_CACHE["v"] = [_load(n) for n in JPGS]
    return _JPG_CACHE["v"]


def _pool(seed=0):
    """the six test jpgs + the awkward synthetic sizes, shuffled"""
    rng = np.random.default_rng(seed)
    syn = [(1, 1), (1, 2000), (3000, 7), (S, S), (2 * S + 1, S - 1)]
    imgs = list(_jpgs()) + [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in syn]
    order = rng.permutation(len(imgs))
    return [imgs[i] for i in order]


def _engine(hip, cfg="yolov3", dtype=None, max_batch=32, decode=None, keep_layers=False, seed=2, semantics=None, obj_bias=-0.75):
    txt = IO.with_input_size(IO.cfg_text(cfg), S)
    flat = IO.synth_weights(IO.parse_cfg(txt), seed=seed, obj_bias=obj_bias)
    e = hip.Engine(txt, max_batch=max_batch, dtype=hip.BF16 if dtype is None else dtype, keep_layers=keep_layers,
                   decode=hip.DECODE_RATIO if decode is None else decode, semantics=hip.SEM_TF if semantics is None else semantics)
    e.set_weights(flat)
    return e, txt, flat


def _single(e, im, **kw):
    e.forward_image(im)
    return e.postprocess(1, **kw)[0]


def _recs_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("dtype", ["BF16", "FP32", "FP16", "FP8", "FP16X2"])
def test_stretch_batch_equals_single_images_bit_for_bit(hiplib, dtype):
    e, _, _ = _engine(hiplib, dtype=getattr(hiplib, dtype))
    pool = _pool()
    kept = 0
    for n in (1, 7, 32):
        imgs = [pool[i % len(pool)] for i in range(n)]
        got = e.detect_images(imgs, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_NETWORK, **POST)
        assert len(got) == n
        for i, im in enumerate(imgs):
            want = _single(e, im, **POST)
            assert _recs_equal(got[i], want), "image %d of %d (%s)" % (i, n, im.shape)
            kept += len(want)
    assert kept > 0
    e.close()


def test_stretch_network_input_equals_single_resize(hiplib):
    e, _, _ = _engine(hiplib, max_batch=7, keep_layers=True)
    imgs = _pool(1)[:7]
    det = e.forward_images(imgs, fit=hiplib.FIT_STRETCH)
    first = e.layer_output(0, 7)
    for i, im in enumerate(imgs):
        d1 = e.forward_image(im)
        assert np.array_equal(e.layer_output(0, 1)[0], first[i]), "image %d" % i     # the layer that reads the fitted input
        assert np.array_equal(d1[0], det[i])
    e.close()


@pytest.mark.parametrize("decode", ["DECODE_RATIO", "DECODE_PIXEL"])
def test_source_pixel_units_equal_convert_to_original_size(hiplib, decode):
    """V3/YOLO_V3_inference.py:55-57 (normalised boxes * original_size) and V3/convert_ckpt_and_inference.py:43-45 (network-pixel boxes
    * original_size / size), applied in numpy to the single-image records"""
    e, _, _ = _engine(hiplib, max_batch=11, decode=getattr(hiplib, decode))
    imgs = _pool(2)
    got = e.detect_images(imgs, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, **POST)
    kept = 0
    for i, im in enumerate(imgs):
        want = _single(e, im, **POST)
        h, w = im.shape[:2]
        original_size = np.array([w, h])
        ratio = original_size if decode == "DECODE_RATIO" else 1.0 * original_size / S
        box = np.stack([want["x0"], want["y0"], want["x1"], want["y1"]], -1).reshape(-1, 2, 2) * ratio
        box = box.reshape(-1, 4).astype(np.float32)
        gb = np.stack([got[i]["x0"], got[i]["y0"], got[i]["x1"], got[i]["y1"]], -1).reshape(-1, 4)
        assert gb.shape == box.shape
        np.testing.assert_array_max_ulp(gb, box, maxulp=1)
        assert np.array_equal(got[i]["score"], want["score"]) and np.array_equal(got[i]["cls"], want["cls"])
        kept += len(want)
    assert kept > 0
    e.close()


def test_per_class_nms_uses_each_images_shape(hiplib):
    """YOLO_NMS_PER_CLASS in source pixels == the oracle's V2 postprocess(image_shape=(h_i, w_i)) on each image's decoded tensor"""
    e, _, _ = _engine(hiplib, cfg="yolov2-tiny-voc", max_batch=11, seed=3)
    imgs = _pool(3)
    det = e.forward_images(imgs, fit=hiplib.FIT_STRETCH)
    sc = (det[..., 4:5] * det[..., 5:]).max(-1)
    thr = float(np.quantile(sc, 0.97))
    got = e.detect_images(imgs, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, score_thr=thr, iou_thr=0.5, max_out=400,
                          nms_mode=hiplib.NMS_PER_CLASS, select_mode=hiplib.SELECT_GT)
    kept = 0
    for i, im in enumerate(imgs):
        c4 = R.detections_boxes(det[i])
        wb, ws, wc = R.v2_postprocess(c4[:, :4], c4[:, 4], c4[:, 5:], image_shape=im.shape[:2], threshold=thr)
        gb = np.stack([got[i]["x0"], got[i]["y0"], got[i]["x1"], got[i]["y1"]], -1).reshape(-1, 4)
        assert np.array_equal(gb.astype(np.int32), wb) and np.array_equal(got[i]["score"], ws) and np.array_equal(got[i]["cls"], wc)
        kept += len(ws)
    assert kept > 0
    e.close()


def _chw_darknet(im):
    """the image as darknet's loader stores it: planar, (float)p/255."""
    return np.ascontiguousarray((im.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))


@pytest.mark.parametrize("relative", [1, 0])
def test_letterbox_darknet_boxes_equal_single_image_path(hiplib, relative):
    e, _, _ = _engine(hiplib, max_batch=7, semantics=hiplib.SEM_DARKNET, seed=4)
    rng = np.random.default_rng(9)
    imgs = list(_jpgs()) + [rng.integers(0, 256, (S + 37, S - 50, 3), dtype=np.uint8)]
    imgs = imgs[:7]
    e.forward_images(imgs, fit=hiplib.FIT_LETTERBOX)
    batched = [e.darknet_boxes(i, im.shape[1], im.shape[0], thresh=0.3, relative=relative) for i, im in enumerate(imgs)]
    total = 0
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        chw = _chw_darknet(im)
        rc = e.lib.yolo_forward_letterbox_chw(e.ctx, chw.ctypes.data, w, h, hiplib.HOST, None, hiplib.HOST)
        assert rc == 0
        single = e.darknet_boxes(0, w, h, thresh=0.3, relative=relative)
        assert single.shape == batched[i].shape and np.array_equal(single, batched[i]), "image %d" % i
        total += len(single)
    assert total > 0
    e.close()


def test_letterbox_detect_records_are_darknets_boxes_after_nms(hiplib):
    """yolo_detect_images_u8 with LETTERBOX: boxes are un-letterboxed BEFORE NMS (darknet's order); with DARKNET NMS every kept record
    is one of get_network_boxes' boxes for that image (x, y, w, h in source pixels)"""
    e, _, _ = _engine(hiplib, max_batch=6, semantics=hiplib.SEM_DARKNET, seed=4)
    imgs = list(_jpgs())
    got = e.detect_images(imgs, fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, score_thr=0.3, iou_thr=0.45, max_out=50,
                          nms_mode=hiplib.NMS_DARKNET)
    e.forward_images(imgs, fit=hiplib.FIT_LETTERBOX)
    kept = 0
    for i, im in enumerate(imgs):
        rec = e.darknet_boxes(i, im.shape[1], im.shape[0], thresh=0.0, relative=0)
        boxes = {tuple(r[:4].tolist()) for r in rec}
        for g in got[i]:
            assert (float(g["x0"]), float(g["y0"]), float(g["x1"]), float(g["y1"])) in boxes
        kept += len(got[i])
    assert kept > 0
    e.close()


def test_letterbox_matches_the_reference_library(hiplib, tmp_path):
    """The veneer test's 160 x 160 yolov3-tiny fp32 network: the per-image boxes of one batched letterbox forward against the compiled
    reference (network_predict_image + get_network_boxes on each image), within that test's tolerances"""
    from oracle import darknet_ref as DR
    if not DR.available():
        pytest.skip("oracle/_ref/libdarknet_ref.so not built")

    class IMAGE(C.Structure):
        _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]
    ref = DR.lib()
    ref.load_network.argtypes = [C.c_char_p, C.c_char_p, C.c_int]; ref.load_network.restype = C.c_void_p
    ref.free_network.argtypes = [C.c_void_p]
    ref.network_predict_image.argtypes = [C.c_void_p, IMAGE]; ref.network_predict_image.restype = C.POINTER(C.c_float)
    ref.get_network_boxes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int)]
    ref.get_network_boxes.restype = C.POINTER(DR.DETECTION)
    ref.free_detections.argtypes = [C.POINTER(DR.DETECTION), C.c_int]
    txt = IO.with_input_size(IO.cfg_text("yolov3-tiny"), S)
    flat = IO.synth_weights(IO.parse_cfg(txt), 21, obj_bias=0.0)
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(txt); IO.write_weights_file(wf, flat, 0, 2)
    with DR._Quiet():
        rnet = ref.load_network(cfg.encode(), wf.encode(), 0)
        ref.set_batch_network(rnet, 1)
    e = hiplib.Engine(txt, max_batch=6, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, decode=hiplib.DECODE_RATIO)
    e.set_weights(flat)
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(120, 200), (250, 96), (160, 160), (207, 331)]]
    imgs += list(_jpgs()[:2])
    e.forward_images(imgs, fit=hiplib.FIT_LETTERBOX)
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        chw = _chw_darknet(im)
        ref.network_predict_image(rnet, IMAGE(w, h, 3, chw.ctypes.data_as(C.POINTER(C.c_float))))
        n0 = C.c_int(0)
        d0 = ref.get_network_boxes(rnet, w, h, 0.0, .5, None, 1, C.byref(n0))
        obj_all = np.array([d0[k].objectness for k in range(n0.value)], np.float32); ref.free_detections(d0, n0.value)
        cand = np.sort(obj_all)[::-1]
        thresh = None
        for k in range(20, len(cand) - 1):          # a threshold no objectness sits near, so both sides select the same boxes
            if cand[k] - cand[k + 1] > 8e-3:
                thresh = float((cand[k] + cand[k + 1]) / 2); break
        assert thresh is not None
        nr = C.c_int(0)
        dr = ref.get_network_boxes(rnet, w, h, thresh, .5, None, 1, C.byref(nr))
        br = np.array([(dr[k].bbox.x, dr[k].bbox.y, dr[k].bbox.w, dr[k].bbox.h) for k in range(nr.value)], np.float32)
        orr = np.array([dr[k].objectness for k in range(nr.value)], np.float32)
        ref.free_detections(dr, nr.value)
        rec = e.darknet_boxes(i, w, h, thresh=thresh, relative=1)
        assert len(rec) == nr.value > 10
        np.testing.assert_allclose(rec[:, :4], br, rtol=2e-3, atol=2e-3)
        np.testing.assert_allclose(rec[:, 4], orr, rtol=2e-3, atol=2e-4)
    e.close()
    ref.free_network(rnet)


def test_graph_replays_with_new_image_sizes(hiplib):
    import torch
    e, _, _ = _engine(hiplib, max_batch=5)
    n, mo = 5, 30
    rng = np.random.default_rng(5)
    a = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(100, 200), (160, 160), (333, 41), (7, 9), (240, 180)]]
    b = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(50, 60), (300, 310), (161, 159), (1, 1), (90, 400)]]
    pa, da = hiplib.pack_images(a); pb, db = hiplib.pack_images(b)
    nbytes = max(pa.size, pb.size) + 64
    dev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    boxes = torch.zeros(n * mo * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    db = db.copy(); db["offset"] += 64                  # the second layout also moves within the buffer

    def run(pix, descs):
        dev.zero_()
        off = int(descs["offset"][0])
        dev[off:off + pix.size].copy_(torch.from_numpy(pix))
        e.detect_images_graph(dev, descs, boxes, counts, fit=hiplib.FIT_STRETCH, max_out=mo, **{k: v for k, v in POST.items() if k != "max_out"})
        e.synchronize()
        bx = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(n, mo); ct = counts.cpu().numpy()
        return [bx[i, :ct[i]].copy() for i in range(n)]

    def eager(imgs):
        return e.detect_images(imgs, fit=hiplib.FIT_STRETCH, **POST)

    want_a, want_b = eager(a), eager(b)
    assert sum(len(r) for r in want_a) > 0 and sum(len(r) for r in want_b) > 0
    for step, (pix, descs, want) in enumerate([(pa, da, want_a), (pa, da, want_a), (pb, db, want_b), (pa, da, want_a), (pb, db, want_b)]):
        got = run(pix, descs)          # call 1 eager, call 2 captures, then replays with other sizes and offsets
        for i in range(n):
            assert _recs_equal(got[i], want[i]), "call %d image %d" % (step + 1, i)
    e.close()


def test_invalid_descriptors_are_rejected_before_any_launch(hiplib):
    import torch
    e, _, _ = _engine(hiplib, max_batch=4)
    imgs = _pool(4)[:3]
    buf, descs = hiplib.pack_images(imgs)
    mo = 10
    dev = torch.from_numpy(buf).cuda()
    dboxes = torch.full((4 * mo * 6,), 7, dtype=torch.int32, device="cuda"); dcounts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def bad_sets():
        d = descs.copy(); d["h"][1] = 0; yield d, 3, buf.size
        d = descs.copy(); d["w"][2] = -5; yield d, 3, buf.size
        d = descs.copy(); d["offset"][2] += 1; yield d, 3, buf.size              # ends one byte past the buffer
        d = descs.copy(); d["offset"][0] = 2 ** 40; yield d, 3, buf.size
        yield descs, 0, buf.size
        yield np.concatenate([descs, descs[:2]]), 5, buf.size                     # more than max_batch
        yield descs, 3, buf.size - 1
    for d, n, nbytes in bad_sets():
        d = np.ascontiguousarray(d)
        boxes = np.full((4, mo), 0, dtype=hiplib.BOX_DTYPE); boxes["cls"] = 7; counts = np.full(4, 7, np.int32)
        rc = e.lib.yolo_detect_images_u8(e.ctx, buf.ctypes.data, nbytes, d.ctypes.data, n, hiplib.FIT_STRETCH, hiplib.HOST, 0.3, 0.45, mo,
                                         hiplib.NMS_TF, hiplib.SELECT_GT, hiplib.UNITS_NETWORK, boxes.ctypes.data, counts.ctypes.data, hiplib.HOST)
        assert rc == -1 and (counts == 7).all() and (boxes["cls"] == 7).all()
        rc = e.lib.yolo_forward_images_u8(e.ctx, buf.ctypes.data, nbytes, d.ctypes.data, n, hiplib.FIT_LETTERBOX, hiplib.HOST, None, hiplib.HOST)
        assert rc == -1
        rc = e.lib.yolo_detect_images_graph(e.ctx, C.c_void_p(dev.data_ptr()), nbytes, d.ctypes.data, n, hiplib.FIT_STRETCH, 0.3, 0.45, mo,
                                            hiplib.NMS_TF, hiplib.SELECT_GT, hiplib.UNITS_NETWORK, C.c_void_p(dboxes.data_ptr()),
                                            C.c_void_p(dcounts.data_ptr()))
        assert rc == -1
        e.synchronize()
        assert (dcounts.cpu().numpy() == 7).all()
    # a letterbox that would be less than one pixel high; a [detection] head cannot be letterboxed
    thin = [np.zeros((1, 2000, 3), np.uint8)]
    with pytest.raises(hiplib.YoloError, match=r"\(-1\)"):
        e.forward_images(thin, fit=hiplib.FIT_LETTERBOX)
    # a valid call afterwards still succeeds, on both entry points
    got = e.detect_images(imgs, fit=hiplib.FIT_STRETCH, score_thr=0.3, iou_thr=0.45, max_out=mo)
    for i, im in enumerate(imgs):
        assert _recs_equal(got[i], _single(e, im, score_thr=0.3, iou_thr=0.45, max_out=mo))
    for _ in range(3):
        e.detect_images_graph(dev, descs, dboxes, dcounts, fit=hiplib.FIT_STRETCH, score_thr=0.3, iou_thr=0.45, max_out=mo)
    e.synchronize()
    bx = dboxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(4, mo); ct = dcounts.cpu().numpy()
    for i in range(3):
        assert _recs_equal(bx[i, :ct[i]].copy(), got[i])
    e.close()


def test_detection_head_cannot_be_letterboxed(hiplib):
    txt = IO.cfg_text("yolov1-tiny")                   # (native input size: the [connected] layers fix it)
    e = hiplib.Engine(txt, max_batch=2)
    e.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=6))
    imgs = _pool(5)[:2]
    with pytest.raises(hiplib.YoloError, match=r"\(-6\)"):
        e.detect_images(imgs, fit=hiplib.FIT_LETTERBOX)
    assert len(e.detect_images(imgs, fit=hiplib.FIT_STRETCH, score_thr=0.05)) == 2
    e.close()


def test_detector_batches_equal_single_images(hiplib):
    from yolo_tensorflow_amd.detector import YOLOV3
    secs = IO.parse_cfg(IO.cfg_text("yolov3"))
    d = YOLOV3(None, weights=IO.synth_weights(secs, seed=7), max_batch=8)
    d.threshold = 0.3
    rng = np.random.default_rng(8)
    imgs = list(_jpgs()) + [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(480, 640), (33, 1000), (416, 416), (5, 5), (700, 300)]]
    got = d.detect_from_images(imgs)
    assert len(got) == 11
    n = 0
    for im, g in zip(imgs, got):
        want = d.detect_from_image(im)
        for a, b in zip(g, want):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        n += len(want[0])
    assert n > 0
    d.engine.close()
