"""Vectorised restatement of threshold + NMS for ONE image, every flavour of the device's k_nms_image, as complete records.

**TEST INFRASTRUCTURE ONLY**, like yolo_ref.py beside it.  The scalar restatements there (`tf_nms` / `_tf_iou`, `dn_nms_sort` / `dn_box_iou`,
`v2_postprocess` / `v2_bboxes_iou`, `np_nms_v3` / `np_iou_v3`) are pinned to the reference by tests/golden, but walk pairs in Python: minutes at the
32768 rows the device's workspace is sized for.  The functions here do the same float32 (V2: int32 / float64) operations in the same order on
"the kept box against every later candidate" at once, and tests/test_postprocess_oracle_host.py holds them bit for bit to the scalar ones.

Order is the device's stated rule: score descending, ties to the lower candidate index (candidates in row order).  The greedy scheme "a kept
box removes every later candidate it overlaps" selects the same boxes as the reference's "a candidate is dropped when it overlaps a selected
box": every IoU form here is symmetric in its operands bit for bit (min / max, commutative sums and products only)."""
import numpy as np
from . import yolo_ref as R

NMS_TF, NMS_PER_CLASS, NMS_DARKNET, NMS_NUMPY_V3, NMS_TF_V1 = 0, 1, 2, 3, 4
SELECT_GT, SELECT_GE = 0, 1
V2_TOP_K = 400                               # bboxes_sort(top_k=400), V2/utils.py:146-151

# the device's record (include/yolo_hip.h: yolo_box)
REC_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("score", "<f4"), ("cls", "<i4")])


def row_scores(det):
    """score = max_k(obj * cls_k) in float32, label = first arg-max (V3/YOLOV3.py:353-357)."""
    sc = (det[:, 4:5] * det[:, 5:]).astype(np.float32)
    return sc.max(-1), sc.argmax(-1).astype(np.int32)


def select_rows(scores, score_thr, select):
    """Rows that pass, in row order (tf.boolean_mask): strict `>` (SELECT_GT) or `>=` (SELECT_GE) against the float32 threshold."""
    t = np.float32(score_thr)
    return np.nonzero(scores >= t if select == SELECT_GE else scores > t)[0]


def candidate_boxes(d4, mode, image_hw=None):
    """The box a candidate enters NMS with (and leaves in its record), from its (cx, cy, w, h): darknet keeps them as they are; YOLOv1 builds
    the horizontal extent from the height and the vertical one from the width (V1/YOLO_V1_Inference.py:259-262, see detect_v1_tf); corners
    through w * 0.5 otherwise (V3/YOLOV3.py:348-351); V2 then scales to the image, truncates to int32 and clips (V2/utils.py:32-43)."""
    d4 = np.asarray(d4, np.float32)
    q0, q1, q2, q3 = d4[:, 0], d4[:, 1], d4[:, 2], d4[:, 3]
    h = np.float32(0.5)
    if mode == NMS_DARKNET:
        return d4.copy()
    if mode == NMS_TF_V1:
        w2 = h * q2; h2 = h * q3
        return np.stack([q0 - h2, q1 - w2, q0 + h2, q1 + w2], -1).astype(np.float32)
    w2 = q2 * h; h2 = q3 * h
    b = np.stack([q0 - w2, q1 - h2, q0 + w2, q1 + h2], -1).astype(np.float32)
    if mode == NMS_PER_CLASS and image_hw is not None:
        ih, iw = int(image_hw[0]), int(image_hw[1])
        x0 = (b[:, 0] * np.float32(iw)).astype(np.int32); y0 = (b[:, 1] * np.float32(ih)).astype(np.int32)
        x1 = (b[:, 2] * np.float32(iw)).astype(np.int32); y1 = (b[:, 3] * np.float32(ih)).astype(np.int32)
        b = np.stack([np.maximum(x0, 0), np.maximum(y0, 0), np.minimum(x1, iw - 1), np.minimum(y1, ih - 1)], -1).astype(np.float32)
    return b


def iou_tf(bi, B):
    """`_tf_iou` of one (x0, y0, x1, y1) box against rows B, float32 step by step; 0 where an area is <= 0."""
    ymin_i = np.minimum(bi[1], bi[3]); xmin_i = np.minimum(bi[0], bi[2]); ymax_i = np.maximum(bi[1], bi[3]); xmax_i = np.maximum(bi[0], bi[2])
    ymin_j = np.minimum(B[:, 1], B[:, 3]); xmin_j = np.minimum(B[:, 0], B[:, 2]); ymax_j = np.maximum(B[:, 1], B[:, 3]); xmax_j = np.maximum(B[:, 0], B[:, 2])
    area_i = (ymax_i - ymin_i) * (xmax_i - xmin_i)
    area_j = (ymax_j - ymin_j) * (xmax_j - xmin_j)
    iy0 = np.maximum(ymin_i, ymin_j); ix0 = np.maximum(xmin_i, xmin_j)
    iy1 = np.minimum(ymax_i, ymax_j); ix1 = np.minimum(xmax_i, xmax_j)
    inter = np.maximum(iy1 - iy0, np.float32(0)) * np.maximum(ix1 - ix0, np.float32(0))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = inter / ((area_i + area_j) - inter)
    return np.where((area_i <= 0) | (area_j <= 0), np.float32(0), v).astype(np.float32)


def iou_darknet(bi, B):
    """`dn_box_iou` of one (cx, cy, w, h) box against rows B, float32 step by step (0 / 0 stays NaN: never above a threshold)."""
    two = np.float32(2)

    def overlap(x1, w1, x2, w2):
        l1 = x1 - w1 / two; l2 = x2 - w2 / two
        r1 = x1 + w1 / two; r2 = x2 + w2 / two
        return np.minimum(r1, r2) - np.maximum(l1, l2)
    w = overlap(bi[0], bi[2], B[:, 0], B[:, 2]); h = overlap(bi[1], bi[3], B[:, 1], B[:, 3])
    inter = np.where((w < 0) | (h < 0), np.float32(0), w * h).astype(np.float32)
    union = ((bi[2] * bi[3]) + (B[:, 2] * B[:, 3])) - inter
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / union).astype(np.float32)


def iou_numpy_v3(box, B):
    """`np_iou_v3` of one (x0, y0, x1, y1) box against rows B in the arrays' float32: no clamp of a negative overlap, + 1e-05."""
    ix0 = np.maximum(box[0], B[:, 0]); iy0 = np.maximum(box[1], B[:, 1])
    ix1 = np.minimum(box[2], B[:, 2]); iy1 = np.minimum(box[3], B[:, 3])
    inter = (ix1 - ix0) * (iy1 - iy0)
    a1 = (box[2] - box[0]) * (box[3] - box[1])
    a2 = (B[:, 2] - B[:, 0]) * (B[:, 3] - B[:, 1])
    return inter / (a1 + a2 - inter + 1e-05)


def _kills(mode, iou_thr, boxes, ibox, labels, i):
    """Which of the candidates after sorted position i the kept candidate i removes."""
    later = slice(i + 1, None)
    if mode in (NMS_TF, NMS_TF_V1):
        return iou_tf(boxes[i], boxes[later]) > np.float32(iou_thr)
    same = labels[later] == labels[i]
    if mode == NMS_DARKNET:
        return same & (iou_darknet(boxes[i], boxes[later]) > np.float32(iou_thr))
    # V2: int32 areas, float64 ratio, and the reference keeps `overlap < thr`, so a 0 / 0 (NaN) removes (V2/utils.py:176-187)
    v = R.v2_bboxes_iou(ibox[i], ibox[later])
    return same & ~(v < np.float64(np.float32(iou_thr)))


def greedy_keep(mode, iou_thr, boxes, labels, cap=None):
    """Sorted positions kept by the greedy scheme, in order; `cap`: stop after that many (tf.image.non_max_suppression's max_output_size)."""
    n = len(boxes)
    ibox = boxes.astype(np.int32) if mode == NMS_PER_CLASS else None
    alive = np.ones(n, bool)
    kept = []
    pos = 0
    while cap is None or len(kept) < cap:
        nxt = np.flatnonzero(alive[pos:])
        if nxt.size == 0:
            break
        i = pos + int(nxt[0])
        kept.append(i)
        if i + 1 < n:
            alive[i + 1:] &= ~_kills(mode, iou_thr, boxes, ibox, labels, i)
        pos = i + 1
    return np.array(kept, dtype=np.int64)


def candidates(det, score_thr, mode, select, image_hw=None):
    """Threshold, then the device's order.  -> (rows, boxes, scores, labels) of the candidates, sorted; V2 keeps its best 400."""
    det = np.asarray(det, np.float32)
    scores, labels = row_scores(det)
    rows = select_rows(scores, score_thr, select)
    order = np.argsort(-scores[rows], kind="stable")           # score descending, ties: lower candidate index
    rows = rows[order]
    if mode == NMS_PER_CLASS:
        rows = rows[:V2_TOP_K]
    return rows, candidate_boxes(det[rows, :4], mode, image_hw), scores[rows], labels[rows]


def postprocess_records(det, score_thr, iou_thr, max_out, mode, select, image_hw=None):
    """Threshold + NMS of one image's rows det [rows, 5 + C] = (cx, cy, w, h, obj, cls...) for the flavours NMS_TF (0), NMS_PER_CLASS (1, V2's
    numpy one: give image_hw), NMS_DARKNET (2) and NMS_TF_V1 (4).  -> (records [K] REC_DTYPE, rows [K] int32): the kept records in order and
    the row of `det` each was formed from.  The capped flavours (0, 4) stop at max_out kept boxes; the others keep everything and report the
    first max_out."""
    if mode not in (NMS_TF, NMS_PER_CLASS, NMS_DARKNET, NMS_TF_V1):
        raise ValueError("flavour %r: use nms_v3_records for the numpy-V3 one" % (mode,))
    rows, boxes, scores, labels = candidates(det, score_thr, mode, select, image_hw)
    capped = mode in (NMS_TF, NMS_TF_V1)
    kept = greedy_keep(mode, iou_thr, boxes, labels, cap=max_out if capped else None)[:max_out]
    rec = np.zeros(len(kept), REC_DTYPE)
    for k, name in enumerate(("x0", "y0", "x1", "y1")):
        rec[name] = boxes[kept, k]
    rec["score"] = scores[kept]; rec["cls"] = labels[kept]
    return rec, rows[kept].astype(np.int32)


def _v3_image(image_pred, confidence_threshold, iou_threshold):
    """One image of `non_max_suppression` (V3/yolo_v3.py:376-420) as [(class, box, score, row)] in class-ascending, then kept order, with the
    reference's behaviours (see np_nms_v3): objectness-only gate, class = argmax of the class scores, keep `iou < thr`, and the score list
    filtered with indices taken on cls_boxes[1:] (a survivor inherits the score of the element in front of it)."""
    p = np.asarray(image_pred)
    rows = np.nonzero(p[:, 4] > confidence_threshold)[0]
    sel = p[rows]
    # the reference drops zero ELEMENTS and reshapes: it only stays row-aligned when a passing row holds none
    assert np.all(sel != 0), "a passing row holds a zero: the reference's nonzero + reshape would misalign"
    classes = np.argmax(sel[:, 5:], axis=-1)
    out = []
    for cls in np.unique(classes):
        pick = np.nonzero(classes == cls)[0]
        srt = sel[pick, 4].argsort()[::-1]
        pick = pick[srt]
        cls_boxes = sel[pick, :4]; cls_scores = sel[pick, 4]; cls_rows = rows[pick]
        while len(cls_boxes) > 0:
            out.append((int(cls), cls_boxes[0], cls_scores[0], int(cls_rows[0])))
            box = cls_boxes[0]
            cls_boxes = cls_boxes[1:]; cls_rows = cls_rows[1:]
            keep = np.nonzero(iou_numpy_v3(box, cls_boxes) < iou_threshold)
            cls_boxes = cls_boxes[keep]; cls_rows = cls_rows[keep]
            cls_scores = cls_scores[keep]
    return out


def np_nms_v3_fast(predictions_with_boxes, confidence_threshold, iou_threshold=0.4):
    """What `np_nms_v3` returns -- {class: [(box, score)]}, shared across the batch -- with the pair loop vectorised."""
    result = {}
    for image_pred in np.asarray(predictions_with_boxes):
        for cls, box, score, _ in _v3_image(image_pred, confidence_threshold, iou_threshold):
            result.setdefault(cls, []).append((box, score))
    return result


def nms_v3_records(det, confidence_threshold, iou_threshold, max_out):
    """The numpy-V3 flavour of one image [rows, 5 + C] = (x0, y0, x1, y1, obj, cls...) as the device reports it: records in class-ascending,
    then kept order, the first max_out of them, and their rows."""
    items = _v3_image(det, confidence_threshold, iou_threshold)[:max_out]
    rec = np.zeros(len(items), REC_DTYPE)
    for k, (cls, box, score, _) in enumerate(items):
        rec[k] = (box[0], box[1], box[2], box[3], score, cls)
    return rec, np.array([it[3] for it in items], dtype=np.int32)
