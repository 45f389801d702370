"""oracle/postprocess_ref.py (the vectorised record oracle the GPU path tests compare with) against the scalar restatements of
oracle/yolo_ref.py, which tests/golden pins to the reference: bit for bit, per flavour, on a few hundred seeded rows with exact score
ties, zero-area and inverted boxes, off-image boxes (V2) and more candidates than V2's top-400 cut.  No GPU."""
import numpy as np
import pytest
from oracle import yolo_ref as R
from oracle import postprocess_ref as P


def _rows(rng, rows, classes, clusters=12, lo=0.0):
    """(cx, cy, w, h, obj, cls...) rows drawn from a few clusters of non-square boxes, scores spread over (lo, 1), plus the awkward ones:
    a 9-way exact score tie, zero-width, zero-area and negative-size boxes."""
    c = rng.integers(0, clusters, rows)
    cen = rng.uniform(0.15, 0.85, (clusters, 2)); wh = np.stack([rng.uniform(0.08, 0.2, clusters), rng.uniform(0.25, 0.45, clusters)], -1)
    det = np.zeros((rows, 5 + classes), np.float32)
    det[:, 0:2] = cen[c] + rng.normal(0, 0.012, (rows, 2)); det[:, 2:4] = wh[c] * rng.uniform(0.85, 1.15, (rows, 2))
    det[:, 4] = rng.uniform(lo, 1, rows)
    det[:, 5:] = rng.uniform(0, 0.4, (rows, classes))
    det[np.arange(rows), 5 + (c % classes)] = rng.uniform(0.8, 1, rows)
    tie = rng.permutation(rows)[:9]
    det[tie, 4] = 0.75; det[tie, 5:] = 0.25; det[tie, 5 + 1] = 0.875
    odd = rng.permutation(rows)[:12]
    det[odd[0:4], 2] = 0; det[odd[4:8], 2:4] = 0; det[odd[8:12], 3] *= -1
    return det


def _assert_tf(det, thr, iou, max_out, select):
    rec, rows = P.postprocess_records(det, thr, iou, max_out, P.NMS_TF, select)
    scores, labels = P.row_scores(det)
    idx = P.select_rows(scores, thr, select)
    boxes = P.candidate_boxes(det[idx, :4], P.NMS_TF)
    sel = R.tf_nms(boxes[:, [1, 0, 3, 2]], scores[idx], max_out, iou)
    assert np.array_equal(rows, idx[sel])
    assert np.array_equal(np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], -1), boxes[sel])
    assert np.array_equal(rec["score"], scores[idx][sel]) and np.array_equal(rec["cls"], labels[idx][sel])
    return rec


def test_tf_flavour_equals_tf_nms_and_detect_v3_tf():
    det = _rows(np.random.default_rng(101), 400, 5)
    for thr, iou, mo in ((0.3, 0.5, 50), (0.5, 0.4, 7), (0.05, 0.45, 400)):
        rec = _assert_tf(det, thr, iou, mo, P.SELECT_GT)
        wb, ws, wc = R.detect_v3_tf(det, thr, iou, mo)
        assert 3 < len(ws) == len(rec) < 300
        assert np.array_equal(np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], -1), wb)
        assert np.array_equal(rec["score"], ws) and np.array_equal(rec["cls"], wc)
    # `>=` takes the rows that sit on the threshold, `>` does not (0.75 * 0.875 is exact in float32)
    t = float(np.float32(0.75) * np.float32(0.875))
    gt = _assert_tf(det, t, 1.0, 400, P.SELECT_GT); ge = _assert_tf(det, t, 1.0, 400, P.SELECT_GE)
    assert len(ge) == len(gt) + 9 and (ge["score"] == np.float32(t)).sum() == 9 and (gt["score"] == np.float32(t)).sum() == 0


def test_v1_flavour_equals_detect_v1_tf():
    rng = np.random.default_rng(102)
    S, B, C = 11, 2, 20                                             # 242 boxes
    pred = rng.uniform(0, 1, S * S * (C + 5 * B)).astype(np.float32)
    pred[S * S * (C + B):] = rng.uniform(0.05, 0.75, S * S * B * 4)
    pred[S * S * C:S * S * C + 6] = 0.5; pred[:3 * C] = np.tile(pred[:C], 3)      # equal confidences over equal class vectors: exact score ties
    det = R.v1_rows(pred, S, B, C)
    for thr, iou, mo in ((0.2, 0.4, 10), (0.05, 0.3, 60), (0.5, 0.5, 242)):
        wb, ws, wc = R.detect_v1_tf(pred, S, B, C, thr, iou, mo)
        rec, rows = P.postprocess_records(det, thr, iou, mo, P.NMS_TF_V1, P.SELECT_GE)
        assert 3 < len(ws) == len(rec)
        assert np.array_equal(rec["score"], ws) and np.array_equal(rec["cls"], wc) and np.array_equal(det[rows, :4], wb)
        h = np.float32(0.5)
        want = np.stack([wb[:, 0] - h * wb[:, 3], wb[:, 1] - h * wb[:, 2], wb[:, 0] + h * wb[:, 3], wb[:, 1] + h * wb[:, 2]], -1)
        assert np.array_equal(np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], -1), want)
    # the swapped extents matter: the plain TF flavour keeps another set on these non-square boxes
    plain, _ = P.postprocess_records(det, 0.05, 0.3, 60, P.NMS_TF, P.SELECT_GE)
    swapped, _ = P.postprocess_records(det, 0.05, 0.3, 60, P.NMS_TF_V1, P.SELECT_GE)
    assert not np.array_equal(plain["score"], swapped["score"])


def test_darknet_flavour_equals_dn_nms_sort():
    det = _rows(np.random.default_rng(103), 260, 3, clusters=8, lo=0.3)
    for thr, iou in ((0.5, 0.45), (0.3, 0.3)):
        scores, labels = P.row_scores(det)
        idx = P.select_rows(scores, thr, P.SELECT_GT)
        probs = np.zeros((len(idx), 3), np.float32); probs[np.arange(len(idx)), labels[idx]] = scores[idx]
        left = R.dn_nms_sort(det[idx, :4], probs, iou)
        alive = left[np.arange(len(idx)), labels[idx]] > 0
        order = np.argsort(-scores[idx], kind="stable")
        want_rows = idx[order][alive[order]]                          # survivors, score descending, ties to the lower candidate
        rec, rows = P.postprocess_records(det, thr, iou, len(det), P.NMS_DARKNET, P.SELECT_GT)
        assert 5 < len(want_rows) < len(idx) > 60
        assert np.array_equal(rows, want_rows)
        assert np.array_equal(np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], -1), det[want_rows, :4])
        assert np.array_equal(rec["score"], scores[want_rows]) and np.array_equal(rec["cls"], labels[want_rows])
        first, frows = P.postprocess_records(det, thr, iou, 4, P.NMS_DARKNET, P.SELECT_GT)      # uncapped: the first max_out of everything kept
        assert np.array_equal(first, rec[:4]) and np.array_equal(frows, rows[:4])


def test_v2_flavour_equals_v2_postprocess():
    rng = np.random.default_rng(104)
    rows, classes, hw = 640, 4, (576, 768)
    det = _rows(rng, rows, classes, clusters=10, lo=0.55)
    det[:, 0:2] = det[:, 0:2] * 1.3                                   # centres to ~1.1: clipped, off-image and inverted int boxes
    tiny = rng.permutation(rows)[:60]; det[tiny, 2:4] = rng.uniform(0, 0.002, (60, 2))       # zero-area int boxes: 0 / 0
    det[:, 5:] = 0; det[np.arange(rows), 5 + rng.integers(0, classes, rows)] = 1.0
    det[:, 4] = (0.3 + 0.69 * rng.permutation(rows) / rows).astype(np.float32)    # distinct scores (the reference's argsort is not stable)
    for thr, expect_cut in ((0.5, True), (0.8, False)):
        d = det
        h = np.float32(.5)
        corners = np.stack([d[:, 0] - d[:, 2] * h, d[:, 1] - d[:, 3] * h, d[:, 0] + d[:, 2] * h, d[:, 1] + d[:, 3] * h], -1)
        bb, ss, cc = R.v2_postprocess(corners, d[:, 4], d[:, 5:], image_shape=hw, threshold=thr, nms_threshold=0.5)
        rec, rws = P.postprocess_records(d, thr, 0.5, rows, P.NMS_PER_CLASS, P.SELECT_GT, image_hw=hw)
        assert ((d[:, 4] > np.float32(thr)).sum() > 400) == expect_cut
        assert 5 < len(ss) == len(rec)
        assert np.array_equal(rec["score"], ss.astype(np.float32)) and np.array_equal(rec["cls"], cc)
        got = np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], -1)
        assert np.array_equal(got.astype(np.int32), bb) and np.array_equal(got, bb.astype(np.float32))
        assert np.array_equal(d[rws, 4], rec["score"])
        assert ((bb[:, 2] <= bb[:, 0]) | (bb[:, 3] <= bb[:, 1])).any()          # degenerate int boxes take part


def test_numpy_v3_flavour_equals_np_nms_v3():
    rng = np.random.default_rng(105)
    det = np.empty((2, 320, 5 + 6), np.float32)
    for b in range(2):
        d = _rows(rng, 320, 6, clusters=9)
        det[b, :, 0:2] = d[:, 0:2] - d[:, 2:4] / 2; det[b, :, 2:4] = d[:, 0:2] + np.abs(d[:, 2:4]) / 2
        det[b, :, 4] = (0.05 + 0.9 * rng.permutation(320) / 320).astype(np.float32)          # distinct objectness
        det[b, :, 5:] = rng.uniform(0.01, 1, (320, 6))
    assert np.all(det != 0)
    want = R.np_nms_v3(det, 0.3, 0.4)
    got = P.np_nms_v3_fast(det, 0.3, 0.4)
    assert sorted(got) == sorted(int(k) for k in want) and sum(len(v) for v in want.values()) > 20
    for k in want:
        assert len(got[int(k)]) == len(want[k])
        for (gb, gs), (wb, ws) in zip(got[int(k)], want[k]):
            assert np.array_equal(gb, wb) and gs == ws and gs.dtype == ws.dtype
    # the record form: class ascending, rows point at the boxes, scores are the reference's shifted ones
    rec, rows = P.nms_v3_records(det[0], 0.3, 0.4, 320)
    one = P.np_nms_v3_fast(det[:1], 0.3, 0.4)
    assert list(rec["cls"]) == [k for k in sorted(one) for _ in one[k]]
    assert np.array_equal(np.stack([rec["x0"], rec["y0"], rec["x1"], rec["y1"]], -1), det[0][rows, :4])
    assert np.array_equal(rec["score"], np.array([s for k in sorted(one) for _, s in one[k]], np.float32))
    assert (rec["score"] != det[0][rows, 4]).any()                   # the off-by-one of V3/yolo_v3.py:414-418 is in
    cut, crow = P.nms_v3_records(det[0], 0.3, 0.4, 5)
    assert np.array_equal(cut, rec[:5]) and np.array_equal(crow, rows[:5])
    with pytest.raises(ValueError):
        P.postprocess_records(det[0], 0.3, 0.4, 5, P.NMS_NUMPY_V3, P.SELECT_GT)
