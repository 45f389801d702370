"""Tiled detection of images larger than the network input (yolo_detect_tiled_u8, DESIGN.md "Tiled detection"), pinned by composing paths
that are already pinned to the oracle: a window is fitted bit for bit as its host-made crop is by yolo_forward_images_u8; the merged result
equals the decoded tensors of those crops, mapped to source pixels by a float32 numpy restatement of the stated expressions, concatenated
in (window, row) order and put through yolo_op_postprocess; one window equals yolo_detect_images_u8; chunking by max_batch, batching of
images and repetition change no bit; every refusal happens before any launch and names what it refuses.

Network input 96 x 96 (yolov3: 567 rows per window), synthetic weights with obj_bias=-0.75 so that candidates exist."""
import os
import numpy as np
import pytest
from conftest import golden
from oracle import postprocess_ref as P
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 96
ROWS = 567
F = np.float32
TILE, OVERLAP = 96, 64
IMG_HW = (150, 190)          # 3 x 4 = 12 windows at tile 96, overlap 64; neither 150 - 96 nor 190 - 96 is a multiple of the stride: the last row and column are pulled back
THR, IOU = 0.3, 0.45


def _kite():
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(os.path.join(ROOT, "tests", "golden", "images", "kite.jpg")).convert("RGB")))


def _image(hw=IMG_HW, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)


_CFG = {}


def _cfg():
    if not _CFG:
        txt = IO.with_input_size(IO.cfg_text("yolov3"), S)
        _CFG["v"] = (txt, IO.synth_weights(IO.parse_cfg(txt), seed=2, obj_bias=-0.75))
    return _CFG["v"]


def _engine(hip, max_batch=16, dtype="BF16", decode="DECODE_RATIO", keep_layers=False):
    txt, flat = _cfg()
    e = hip.Engine(txt, max_batch=max_batch, dtype=getattr(hip, dtype), decode=getattr(hip, decode), keep_layers=keep_layers)
    e.set_weights(flat)
    assert e.rows == ROWS
    return e


def _crops(hip, img, tile, overlap):
    wins = hip.tile_windows(img.shape[:2], tile, overlap)
    return wins, [np.ascontiguousarray(img[y0:y0 + h, x0:x0 + w]) for y0, x0, h, w in wins]


def _forward_crops(e, crops, fit):
    return np.concatenate([e.forward_images(crops[i:i + e.max_batch], fit=fit) for i in range(0, len(crops), e.max_batch)])


# ---- the mapping of a window's (cx, cy, w, h) rows to source-image pixels, restated in float32 numpy (DESIGN.md "Tiled detection") ----
def _letterbox_dims(netw, neth, w, h):
    """darknet's letterbox_image integers (DN/image.c:960-966)"""
    if F(netw) / F(w) < F(neth) / F(h):
        return netw, (h * netw) // w
    return (w * neth) // h, neth


def _correct_yolo_boxes(q, netw, neth, w, h):
    """correct_yolo_boxes with relative = 0 (DN/yolo_layer.c:247-273), operation for operation: x and y through double, w and h in float"""
    new_w, new_h = _letterbox_dims(netw, neth, w, h)
    x = ((q[:, 0].astype(np.float64) - (netw - new_w) / 2. / netw) / np.float64(F(new_w) / F(netw))).astype(F) * F(w)
    y = ((q[:, 1].astype(np.float64) - (neth - new_h) / 2. / neth) / np.float64(F(new_h) / F(neth))).astype(F) * F(h)
    bw = (q[:, 2] * (F(netw) / F(new_w))) * F(w)
    bh = (q[:, 3] * (F(neth) / F(new_h))) * F(h)
    return np.stack([x, y, bw, bh], -1).astype(F)


def map_boxes(q, win, fit_letterbox, net_pixels, centre):
    """q [rows, 4] float32 (cx, cy, w, h) as decoded for one window -> the rows its image's merged list holds: corners (x0, y0, x1, y1) in source
    pixels, or (cx, cy, w, h) with centre (the form YOLO_NMS_DARKNET reads)."""
    y0, x0, h, w = (int(v) for v in win)
    q = np.asarray(q, F)
    if net_pixels:
        q = (q / np.array([S, S, S, S], F)).astype(F)
    if fit_letterbox:
        q = _correct_yolo_boxes(q, S, S, w, h); sx = sy = F(1)
    else:
        sx, sy = F(w), F(h)
    X, Y = F(x0), F(y0)
    if centre:
        return np.stack([q[:, 0] * sx + X, q[:, 1] * sy + Y, q[:, 2] * sx, q[:, 3] * sy], -1).astype(F)
    w2 = q[:, 2] * F(0.5); h2 = q[:, 3] * F(0.5)
    return np.stack([(q[:, 0] - w2) * sx + X, (q[:, 1] - h2) * sy + Y, (q[:, 0] + w2) * sx + X, (q[:, 1] + h2) * sy + Y], -1).astype(F)


def merged_tensor(det, wins, fit_letterbox, net_pixels, centre):
    """the windows' decoded tensors [W, rows, 5 + C] -> [1, W * rows, 5 + C] in (window, row) order with mapped boxes"""
    out = det.copy()
    for k, win in enumerate(wins):
        out[k, :, :4] = map_boxes(det[k, :, :4], win, fit_letterbox, net_pixels, centre)
    return out.reshape(1, -1, det.shape[-1])


def compose(hip, merged, thr, iou, max_out, nms_mode, select):
    """-> (records, window of every kept record)"""
    rec, rows = hip.op_postprocess(merged, thr, iou, max_out, nms_mode, select, corners=True, return_rows=True)
    return rec[0], rows[0] // ROWS


def cross_window_suppressions(merged, thr, iou, max_out, nms_mode, select):
    """The greedy scheme over the merged rows in numpy (the device's order: score descending, ties to the lower row): how many candidates
    were removed by a kept box of ANOTHER window."""
    det = merged[0]
    scores, labels = P.row_scores(det)
    rows = P.select_rows(scores, thr, select)
    rows = rows[np.argsort(-scores[rows], kind="stable")]
    boxes, labels, win = det[rows, :4], labels[rows], rows // ROWS
    alive = np.ones(len(rows), bool)
    kept = cross = 0
    for i in range(len(rows)):
        if not alive[i]:
            continue
        kept += 1
        if nms_mode == P.NMS_TF and kept == max_out:
            break
        if nms_mode == P.NMS_TF:
            kill = P.iou_tf(boxes[i], boxes[i + 1:]) > F(iou)
        else:
            kill = (labels[i + 1:] == labels[i]) & (P.iou_darknet(boxes[i], boxes[i + 1:]) > F(iou))
        kill &= alive[i + 1:]
        cross += int((win[i + 1:][kill] != win[i]).sum())
        alive[i + 1:] &= ~kill
    return cross


def _boxes(r):
    return np.stack([r["x0"], r["y0"], r["x1"], r["y1"]], -1).reshape(-1, 4)


def _same(got, want, what=""):
    assert len(got) == len(want), "%s: %d records, %d expected" % (what, len(got), len(want))
    assert np.array_equal(got["score"], want["score"]) and np.array_equal(got["cls"], want["cls"]), what
    np.testing.assert_array_max_ulp(_boxes(got), _boxes(want), maxulp=1)


def _bytes_equal(a, b):
    return len(a) == len(b) and all(len(x) == len(y) and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- 1. a window is its crop ----
@pytest.mark.parametrize("fit", ["FIT_STRETCH", "FIT_LETTERBOX"])
def test_a_window_is_fitted_as_its_crop(hiplib, fit):
    """The layer that reads the fitted input (keep_layers), after one tiled step over all windows and after yolo_forward_images_u8 over the
    host-made crops: a 150 x 200 random image cut by the network's own tile (15 windows, the last row and column pulled back to the edge)
    and by an odd 77 x 131 tile with odd overlaps, and kite.jpg cut into its 12 windows of 416 x 416"""
    e = _engine(hiplib, max_batch=16, keep_layers=True)
    f = getattr(hiplib, fit)
    cases = [(_image((150, 200), 5), (96, 96), (64, 64)), (_image((150, 200), 5), (77, 131), (9, 31)), (_kite(), (416, 416), (64, 64))]
    for img, tile, overlap in cases:
        wins, crops = _crops(hiplib, img, tile, overlap)
        W = len(wins)
        assert 1 < W <= e.max_batch
        H, Wd = img.shape[:2]
        assert any(y0 + h == H and x0 + w == Wd for y0, x0, h, w in wins)          # a window at the right and bottom edge
        e.forward_images(crops, fit=f, want_detections=False)
        want = e.layer_output(0, W)
        e.detect_tiled([img], tile=tile, overlap=overlap, fit=f, score_thr=THR, iou_thr=IOU)
        got = e.layer_output(0, W)
        assert np.array_equal(got, want), (img.shape, tile)
        assert not np.array_equal(got[0], got[W - 1])
    e.close()


# ---- 2. merge + NMS equals the composition ----
@pytest.mark.parametrize("dtype,decode", [("BF16", "DECODE_RATIO"), ("BF16", "DECODE_PIXEL"), ("FP32", "DECODE_RATIO"), ("FP32", "DECODE_PIXEL")])
def test_merge_and_nms_equal_the_composition(hiplib, dtype, decode):
    e = _engine(hiplib, max_batch=16, dtype=dtype, decode=decode)
    img = _image()
    wins, crops = _crops(hiplib, img, TILE, OVERLAP)
    assert len(wins) == 12 and len(wins) * ROWS <= 32768
    net_pixels = decode == "DECODE_PIXEL"
    checked = other_window = suppressed = 0
    for fit in ("FIT_STRETCH", "FIT_LETTERBOX"):
        det = _forward_crops(e, crops, getattr(hiplib, fit))
        sc = np.sort((det[..., 4:5] * det[..., 5:]).astype(F).max(-1).reshape(-1))
        thr_on_a_score = float(sc[np.searchsorted(sc, F(THR)) + 5])          # a threshold that IS a row's score: `>` and `>=` select different sets
        for nms, max_out in (("NMS_TF", 20), ("NMS_DARKNET", 60)):
            merged = merged_tensor(det, wins, fit == "FIT_LETTERBOX", net_pixels, nms == "NMS_DARKNET")
            counts = []
            for select in ("SELECT_GT", "SELECT_GE"):
                kw = dict(score_thr=thr_on_a_score, iou_thr=IOU, max_out=max_out, nms_mode=getattr(hiplib, nms), select_mode=getattr(hiplib, select))
                want, want_win = compose(hiplib, merged, kw["score_thr"], IOU, max_out, kw["nms_mode"], kw["select_mode"])
                got = e.detect_tiled([img], tile=TILE, overlap=OVERLAP, fit=getattr(hiplib, fit), **kw)[0]
                print("%s %s %s %s %s: kept %d, from other windows %d" % (dtype, decode, fit, nms, select, len(want), int((want_win != 0).sum())))
                _same(got, want, "%s %s %s" % (fit, nms, select))
                cross = cross_window_suppressions(merged, kw["score_thr"], IOU, max_out, kw["nms_mode"], kw["select_mode"])
                print("    removed by a box of another window: %d" % cross)
                checked += 1; other_window += int((want_win != 0).sum()); suppressed += cross
                counts.append(int((P.select_rows(P.row_scores(merged[0])[0], kw["score_thr"], kw["select_mode"])).size))
            assert counts[1] > counts[0]          # the two selection modes were told apart
    assert checked == 8 and other_window > 0 and suppressed > 0
    e.close()


# ---- 3. one window is detect_images ----
@pytest.mark.parametrize("fit", ["FIT_STRETCH", "FIT_LETTERBOX"])
def test_one_window_equals_detect_images_in_source_pixels(hiplib, fit):
    e = _engine(hiplib, max_batch=4)
    imgs = [_image((80, 91), 3), _image((96, 96), 4), _image((33, 96), 6)]          # none larger than the tile
    kw = dict(fit=getattr(hiplib, fit), score_thr=THR, iou_thr=IOU, max_out=30)
    want = e.detect_images(imgs, units=hiplib.UNITS_SOURCE_PIXELS, **kw)
    got = e.detect_tiled(imgs, relative=False, **kw)
    assert sum(len(w) for w in want) > 0
    for g, w, im in zip(got, want, imgs):
        _same(g, w, str(im.shape))
    e.close()


# ---- 4. chunking and batching change nothing ----
def test_chunking_batching_and_repetition_change_no_bit(hiplib):
    img, small = _image(), _image((100, 75), 8)
    kw = dict(tile=TILE, overlap=OVERLAP, score_thr=THR, iou_thr=IOU, max_out=25)
    res = {}
    for mb in (4, 5, 16):          # three steps, a ragged last step, one step
        e = _engine(hiplib, max_batch=mb)
        res[mb] = e.detect_tiled([img], **kw)
        if mb == 5:                # two images of different sizes share steps; the second one's windows begin inside the third step
            both = e.detect_tiled([img, small], **kw)
            alone = e.detect_tiled([img], **kw) + e.detect_tiled([small], **kw)
            assert _bytes_equal(both, alone) and len(both[1]) > 0
            swapped = e.detect_tiled([small, img], **kw)
            assert _bytes_equal(swapped, alone[::-1])
            assert _bytes_equal(e.detect_tiled([img], **kw), res[mb])          # the same call again
        e.close()
    assert len(res[4][0]) > 0
    assert _bytes_equal(res[4], res[5]) and _bytes_equal(res[4], res[16])


# ---- 5. refusals, before any launch, each naming what it refuses ----
def test_refusals_name_what_they_refuse_and_touch_nothing(hiplib):
    e = _engine(hiplib, max_batch=4)
    img = _image()
    buf, descs = hiplib.pack_images([img])
    mo = 10
    good = dict(tile=(0, 0), overlap=(64, 64), fit=hiplib.FIT_STRETCH, nms=hiplib.NMS_TF, descs=descs, nbytes=buf.size)

    def call(**over):
        a = dict(good); a.update(over)
        boxes = np.zeros(mo, dtype=hiplib.BOX_DTYPE); boxes["cls"] = 7; counts = np.full(1, 7, np.int32)
        d = np.ascontiguousarray(a["descs"])
        rc = e.lib.yolo_detect_tiled_u8(e.ctx, buf.ctypes.data, a["nbytes"], d.ctypes.data, 1, a["tile"][0], a["tile"][1], a["overlap"][0], a["overlap"][1],
                                        a["fit"], hiplib.HOST, THR, IOU, mo, a["nms"], hiplib.SELECT_GT, 0, boxes.ctypes.data, counts.ctypes.data, hiplib.HOST)
        assert (counts == 7).all() and (boxes["cls"] == 7).all()          # nothing was written
        return rc, e.lib.yolo_last_error(e.ctx).decode()

    for fit in ("FIT_CV2", "FIT_CV2_BGR", "FIT_CENTER_CROP"):
        rc, msg = call(fit=getattr(hiplib, fit))
        assert rc == -6 and "YOLO_" + fit in msg, msg
    for nms in ("NMS_PER_CLASS", "NMS_TF_V1", "NMS_NUMPY_V3"):
        rc, msg = call(nms=getattr(hiplib, nms))
        assert rc == -6 and "YOLO_" + nms in msg, msg
    for overlap in ((96, 64), (64, 96), (200, 0), (-1, 0)):
        rc, msg = call(overlap=overlap)
        assert rc == -1 and "overlap" in msg, msg
    rc, msg = call(tile=(64, 64), overlap=(64, 0))
    assert rc == -1 and "overlap" in msg, msg
    d = descs.copy(); d["offset"][0] += 1                         # ends one byte past the buffer
    rc, msg = call(descs=d)
    assert rc == -1 and "past" in msg, msg
    rc, msg = call(nbytes=buf.size - 1)
    assert rc == -1 and "past" in msg, msg
    d = descs.copy(); d["h"][0] = 0
    assert call(descs=d)[0] == -1
    with pytest.raises(hiplib.YoloError, match="letterboxes to less than one pixel"):
        e.detect_tiled([np.zeros((1, 2000, 3), np.uint8)], tile=(96, 2000), fit=hiplib.FIT_LETTERBOX)
    # a valid call afterwards succeeds
    assert len(e.detect_tiled([img], score_thr=THR, iou_thr=IOU)[0]) > 0
    e.close()
    g = golden("mini_cls19.npz")
    clf = hiplib.Engine(str(g["cfg"]), max_batch=2)
    clf.set_weights(g["weights"])
    with pytest.raises(hiplib.YoloError, match="classifier"):
        clf.detect_tiled([img])
    clf.close()
    v1 = hiplib.Engine(IO.cfg_text("yolov1-tiny"), max_batch=1)
    v1.set_weights(IO.synth_weights(IO.parse_cfg(IO.cfg_text("yolov1-tiny")), seed=6))
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*\[detection\]"):
        v1.detect_tiled([img], fit=hiplib.FIT_LETTERBOX)
    v1.close()


def test_capacity_of_one_image_is_32768_candidates(hiplib):
    """With score_thr = 0 and `>=` every row is a candidate: 56 windows (31752 rows) are served, 64 windows (36288 rows) are refused with the
    image and the count named, and nothing is written -- also when a small image shares the call"""
    e = _engine(hiplib, max_batch=16)
    fits, over, small = _image((288, 320), 13), _image((320, 320), 14), _image((60, 70), 15)
    assert len(hiplib.tile_windows((288, 320), TILE, OVERLAP)) == 56 and len(hiplib.tile_windows((320, 320), TILE, OVERLAP)) == 64
    kw = dict(tile=TILE, overlap=OVERLAP, score_thr=0.0, iou_thr=IOU, max_out=7, select_mode=hiplib.SELECT_GE)
    got = e.detect_tiled([small, fits], **kw)
    assert [len(g) for g in got] == [7, 7]
    buf, descs = hiplib.pack_images([small, over])
    boxes = np.zeros((2, 7), dtype=hiplib.BOX_DTYPE); boxes["cls"] = 7; counts = np.full(2, 7, np.int32)
    rc = e.lib.yolo_detect_tiled_u8(e.ctx, buf.ctypes.data, buf.size, descs.ctypes.data, 2, TILE, TILE, OVERLAP, OVERLAP, hiplib.FIT_STRETCH, hiplib.HOST,
                                    0.0, IOU, 7, hiplib.NMS_TF, hiplib.SELECT_GE, 0, boxes.ctypes.data, counts.ctypes.data, hiplib.HOST)
    msg = e.lib.yolo_last_error(e.ctx).decode()
    assert rc == -6 and "image 1 " in msg and str(64 * ROWS) in msg, msg
    assert (counts == 7).all() and (boxes["cls"] == 7).all()
    assert _bytes_equal(e.detect_tiled([small, fits], **kw), got)          # the context serves the next call
    e.close()


# ---- 6. the detector's entry point ----
def test_detector_large_images_equal_the_composition(hiplib):
    from yolo_tensorflow_amd.detector import YOLOV3
    secs = IO.parse_cfg(IO.cfg_text("yolov3"))
    d = YOLOV3(None, weights=IO.synth_weights(secs, seed=7), max_batch=2)
    d.threshold = 0.3
    rows = d.engine.rows
    img = _image((416, 700), 9)                       # two windows of 416 x 416, 132 columns shared
    wins, crops = _crops(hiplib, img, 416, 64)
    assert len(wins) == 2 and 2 * rows <= 32768
    det = d.engine.forward_images(crops, fit=hiplib.FIT_STRETCH)
    merged = det.copy()
    for k, (y0, x0, h, w) in enumerate(wins):
        q = det[k, :, :4]; w2 = q[:, 2] * F(0.5); h2 = q[:, 3] * F(0.5)
        merged[k, :, :4] = np.stack([(q[:, 0] - w2) * F(w) + F(x0), (q[:, 1] - h2) * F(h) + F(y0), (q[:, 0] + w2) * F(w) + F(x0), (q[:, 1] + h2) * F(h) + F(y0)], -1)
    want = hiplib.op_postprocess(merged.reshape(1, -1, det.shape[-1]), d.threshold, d.iou_threshold, d.max_output_size, hiplib.NMS_TF, d.select_mode, corners=True)[0]
    want_boxes = (_boxes(want) / np.array([700, 416, 700, 416], F)).astype(F)
    (scores, boxes, classes), = d.detect_from_large_images([img])
    assert len(scores) == len(want) > 0
    assert np.array_equal(scores, want["score"]) and np.array_equal(classes, want["cls"])
    np.testing.assert_array_max_ulp(boxes, want_boxes, maxulp=1)
    assert boxes.dtype == np.float32 and boxes.shape == (len(scores), 4)
    d.engine.close()
