"""k_nms_image (csrc/post_ops.hip) on every path it can take, for every NMS flavour, at the boundaries between the paths: complete records
(x0, y0, x1, y1, score, cls), their order and the counts against oracle/postprocess_ref.py, bit for bit (np.array_equal everywhere; the
oracle is pinned to the reference's restatements by tests/test_postprocess_oracle_host.py).

The path is a function of (M, nms_mode, max_out), M = the rows that pass the threshold.  With post_ops.hip's

    #define NMS_FAST 512        // most candidates the all-in-LDS paths take
    #define SORT_LDS 4096       // largest padded power of two the bitonic sort keeps in LDS
    (V2's bboxes_sort top_k)    // 400: `if (a.nms_mode == 1 && M > 400) M = 400`, once after nms_sort_lds, once inside nms_sort_global

    flavour (nms_mode)      M <= 512, max_out <= 64   M <= 512, max_out > 64   512 < M <= 4096              M > 4096
    ---------------------   -----------------------   ----------------------   --------------------------   ---------------------------
    TF (0), V1 TF (4)       sort_lds + nms_lazy       sort_lds + nms_matrix    LDS bitonic + nms_general    global bitonic + nms_general
    V2 numpy (1)            sort_lds + nms_matrix (cut to 400 behind the sort)     LDS bitonic + nms_general    global bitonic + nms_general
                                                                                   (cut to 400 in nms_sort_global, both)
    darknet (2)             sort_lds + nms_matrix (any max_out)                    LDS bitonic + nms_general    global bitonic + nms_general
    numpy-V3 (3)            LDS bitonic + nms_numpy_v3 (never the fast paths)  LDS bitonic + nms_numpy_v3   global bitonic + nms_numpy_v3

Every cell has a named case below: the ids read <flavour>-M<M>-out<max_out>.  The alive set is kept in 64-candidate words on the fast
paths (32 on the general ones), so M = 63 / 64 / 65 sit on a word boundary; rows = 32768 is what the threshold compaction (32 ballot words
per wave), the alive bitset and the numpy-V3 key's 15-bit index are sized for."""
import functools
import numpy as np
import pytest
from oracle import postprocess_ref as P

pytestmark = pytest.mark.gpu

THR = 0.5
IOU = 0.45
NAMES = {P.NMS_TF: "tf", P.NMS_PER_CLASS: "v2", P.NMS_DARKNET: "darknet", P.NMS_NUMPY_V3: "npv3", P.NMS_TF_V1: "v1"}


# ---------------------------------------------------------------------------------------------------------------------------------
# the one input builder
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planted(rows, M, seed, classes=6, clusters=30, centre_hi=0.85, distinct=False, tiny=0.0, equal=0, tie=None, lonely=None):
    """[rows, 5 + classes] float32 rows (cx, cy, w, h, obj, cls...) of which EXACTLY M score above THR: obj = 1.0 and a one-hot class
    vector holding the score, so score and label are what was planted; every other row scores below 0.45.  The passing rows come from
    `clusters` tight clusters of non-square boxes (h ~ 3 w: YOLOv1's swapped extents change every IoU), at random row positions.
    distinct: no two passing scores equal.  centre_hi > 1 / tiny: boxes that leave the image / collapse to zero-area int boxes (V2).
    equal: that many MORE rows, small boxes of their own, whose score is bit-equal to THR.  tie = (above, n): the candidates ranked
    above .. above + n - 1 by score all get one score.  lonely = (first, n): the candidates ranked first .. first + n - 1 get small boxes of
    their own, away from the clusters, so each of them is kept whenever it is admitted to the NMS at all."""
    rng = np.random.default_rng(seed)
    f = np.float32
    det = np.zeros((rows, 5 + classes), f)
    det[:, 0:2] = rng.uniform(0.1, 0.9, (rows, 2)); det[:, 2:4] = rng.uniform(0.05, 0.3, (rows, 2))
    det[:, 4] = rng.uniform(0.05, 0.9, rows); det[:, 5:] = rng.uniform(0, 0.5, (rows, classes))
    where = rng.permutation(rows)
    pos = np.sort(where[:M])
    c = rng.integers(0, clusters, M)
    cen = rng.uniform(0.15, centre_hi, (clusters, 2)); wh = np.stack([rng.uniform(0.06, 0.12, clusters), rng.uniform(0.2, 0.35, clusters)], -1)
    det[pos, 0:2] = cen[c] + rng.normal(0, 0.004, (M, 2)); det[pos, 2:4] = wh[c] * (1 + rng.normal(0, 0.02, (M, 2)))
    if tiny:
        t = rng.uniform(0, 1, M) < tiny
        det[pos[t], 2:4] = rng.uniform(0, 0.0015, (int(t.sum()), 2))
    score = (0.55 + 0.44 * rng.permutation(M) / max(M, 1)).astype(f) if distinct else rng.uniform(0.55, 0.999, M).astype(f)
    if tie:
        rank = np.argsort(-score, kind="stable")
        score[rank[tie[0]:tie[0] + tie[1]]] = score[rank[tie[0]]]
    if lonely:
        alone = np.argsort(-score, kind="stable")[lonely[0]:lonely[0] + lonely[1]]
        det[pos[alone], 0] = 0.04 + 0.92 * (np.arange(len(alone)) + 0.5) / max(len(alone), 1); det[pos[alone], 1] = 0.03
        det[pos[alone], 2] = 0.021; det[pos[alone], 3] = 0.033
    det[pos, 4] = 1.0; det[pos, 5:] = 0
    det[pos, 5 + c % classes] = score
    if equal:
        eq = where[M:M + equal]
        det[eq, 0:2] = rng.uniform(0.05, 0.95, (equal, 2)); det[eq, 2] = 0.011; det[eq, 3] = 0.017
        det[eq, 4] = 1.0; det[eq, 5:] = 0; det[eq, 5 + classes - 1] = f(THR)
    det.setflags(write=False)
    return det


@functools.lru_cache(maxsize=None)
def planted_v3(rows, M, seed, classes=12, clusters=30, spread=False):
    """The same rows in the numpy-V3 flavour's layout (x0, y0, x1, y1, obj, cls...): objectness = the planted score (distinct, M above
    THR), class scores nonzero with the planted class on top.  spread: the class follows the row instead of the cluster, so every class
    index is in use."""
    d = planted(rows, M, seed, classes=classes, clusters=clusters, distinct=True)
    scores, labels = P.row_scores(d)
    rng = np.random.default_rng(seed + 1)
    if spread:
        labels = (np.arange(rows) * 7 % classes).astype(np.int32)
    out = np.empty_like(d)
    out[:, 0:2] = d[:, 0:2] - d[:, 2:4] / 2; out[:, 2:4] = d[:, 0:2] + d[:, 2:4] / 2
    out[:, 4] = scores
    out[:, 5:] = rng.uniform(0.02, 0.5, (rows, classes)); out[np.arange(rows), 5 + labels] = 0.9
    assert np.all(out != 0)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle(key, mode, max_out, select=P.SELECT_GT, image_hw=None, iou=IOU):
    det = planted(*key[0], **dict(key[1]))
    return P.postprocess_records(det, THR, iou, max_out, mode, select, image_hw)


def case(rows, M, seed, **kw):
    """hashable name of a planted() input"""
    return ((rows, M, seed), tuple(sorted(kw.items())))


def det_of(key):
    return planted(*key[0], **dict(key[1]))


def passing(det, select=P.SELECT_GT):
    return len(P.select_rows(P.row_scores(det)[0], THR, select))


def rows_for(M):
    return 1500 if M <= 513 else 5000          # neither a multiple of the 1024-thread workgroup


def check(hiplib, key, M, mode, max_out, select=P.SELECT_GT, image_hw=None, iou=IOU, with_rows=False):
    det = det_of(key)
    assert passing(det, select) == M                                         # the case is the one designed
    want, want_rows = oracle(key, mode, max_out, select, image_hw, iou)
    if M >= 5:
        assert 5 <= len(want) < M                                            # something is kept, something is removed
    else:
        assert len(want) == M
    res = hiplib.op_postprocess(det[None], THR, iou, max_out, mode, select, image_hw=image_hw, return_rows=with_rows)
    got = res[0][0] if with_rows else res[0]
    assert len(got) == len(want), "kept %d, oracle %d" % (len(got), len(want))
    assert np.array_equal(got, want), "first differing record %d" % int(np.argmax(got != want))
    if with_rows:
        assert np.array_equal(res[1][0], want_rows)
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# flavour x path x boundary
# ---------------------------------------------------------------------------------------------------------------------------------
CAPPED_M = (0, 1, 63, 64, 65, 511, 512, 513, 4096, 4097)


@pytest.mark.parametrize("max_out", [20, 100], ids=lambda v: "out%d" % v)
@pytest.mark.parametrize("M", CAPPED_M, ids=lambda v: "M%d" % v)
@pytest.mark.parametrize("mode", [P.NMS_TF, P.NMS_TF_V1], ids=lambda v: NAMES[v])
def test_capped_flavours_on_every_path(hiplib, mode, M, max_out):
    """TF and YOLOv1's TF NMS: lazy (max_out 20) and matrix (100) up to 512 candidates, nms_general behind the LDS sort to 4096 and
    behind the global-memory sort above."""
    got = check(hiplib, case(rows_for(M), M, 1000 + M), M, mode, max_out)
    assert len(got) <= max_out


def test_v1_swapped_extents_change_the_answer(hiplib):
    """The planted boxes are far from square, so the V1 flavour (horizontal extent from the height) must keep another set than TF's."""
    key = case(1500, 512, 1512)
    a, _ = oracle(key, P.NMS_TF, 100); b, _ = oracle(key, P.NMS_TF_V1, 100)
    assert not np.array_equal(a["score"], b["score"])


@pytest.mark.parametrize("M", CAPPED_M, ids=lambda v: "M%d" % v)
def test_darknet_flavour_on_every_path(hiplib, M):
    check(hiplib, case(rows_for(M), M, 2000 + M), M, P.NMS_DARKNET, 400)


def test_darknet_flavour_keeps_more_than_max_out(hiplib):
    """Uncapped flavour: everything is kept, the count is clamped and the records are the first max_out."""
    key = case(1500, 600, 2600, clusters=60)
    got = check(hiplib, key, 600, P.NMS_DARKNET, 30)
    everything, _ = oracle(key, P.NMS_DARKNET, 1500)
    assert len(got) == 30 < len(everything) and np.array_equal(got, everything[:30])


@pytest.mark.parametrize("M", [399, 400, 401, 512, 513, 1500], ids=lambda v: "M%d" % v)
def test_v2_flavour_and_its_top_400_cut(hiplib, M):
    """V2's numpy NMS: int pixel boxes of a 576 x 768 image (clipped, off-image and zero-area ones: 0 / 0 removes), float64 ratio, and
    only the best 400 candidates enter -- cut behind the LDS sort up to 512 candidates and inside nms_sort_global above."""
    key = case(2000, M, 3000 + M, centre_hi=1.1, distinct=True, tiny=0.1, lonely=(394, 12))
    got = check(hiplib, key, M, P.NMS_PER_CLASS, 400, image_hw=(576, 768))
    ranked = np.sort(P.row_scores(det_of(key))[0])[::-1]
    # the candidates ranked 394 .. 405 stand alone: each one is kept if it enters, so the cut shows -- 399 is in, 400 is not
    assert all(ranked[k] in got["score"] for k in range(394, min(M, 400)))
    assert not any(ranked[k] in got["score"] for k in range(400, min(M, 406)))
    boxes = np.stack([got["x0"], got["y0"], got["x1"], got["y1"]], -1)
    assert ((boxes[:, 2] <= boxes[:, 0]) | (boxes[:, 3] <= boxes[:, 1])).any()          # degenerate int boxes are among the kept
    if M > 400:
        cut = np.sort(P.row_scores(det_of(key))[0])[-400]
        assert got["score"].min() >= cut                                                 # nothing below the 400th score comes out


def _v3_check(hiplib, det, thr=THR, iou=0.4):
    from yolo_tensorflow_amd import yolo_v3
    want = P.np_nms_v3_fast(det, thr, iou)
    got = yolo_v3.non_max_suppression(det, thr, iou)
    assert sorted(got) == sorted(want)
    for k in want:
        assert len(got[k]) == len(want[k])
        for (gb, gs), (wb, ws) in zip(got[k], want[k]):
            assert np.array_equal(gb, wb) and gs == ws
    return want


@pytest.mark.parametrize("M", [1, 513, 4096, 4097], ids=lambda v: "M%d" % v)
def test_numpy_v3_flavour_on_both_sorts(hiplib, M):
    det = planted_v3(rows_for(M), M, 4000 + M)
    assert int((det[:, 4] > np.float32(THR)).sum()) == M
    want = _v3_check(hiplib, det[None])
    kept = sum(len(v) for v in want.values())
    assert kept == M if M < 5 else 5 <= kept < M


# ---------------------------------------------------------------------------------------------------------------------------------
# the row-count limit
# ---------------------------------------------------------------------------------------------------------------------------------
def test_32768_rows_all_passing_tf(hiplib):
    key = case(32768, 32768, 5001, clusters=40)
    got = check(hiplib, key, 32768, P.NMS_TF, 100)
    assert len(got) < 100                                                    # a few dozen clusters: the scan runs to the last candidate


def test_32768_rows_all_passing_numpy_v3(hiplib):
    det = planted_v3(32768, 32768, 5002, classes=64, clusters=40, spread=True)
    assert int((det[:, 4] > np.float32(THR)).sum()) == 32768
    want = _v3_check(hiplib, det[None])
    assert len(want) == 64 and 64 * 5 <= sum(len(v) for v in want.values()) < 32768 // 4


def test_32769_rows_are_refused(hiplib):
    with pytest.raises(hiplib.YoloError):
        hiplib.op_postprocess(np.zeros((1, 32769, 6), np.float32), THR, IOU, 20)


# ---------------------------------------------------------------------------------------------------------------------------------
# ties, threshold equality, mixed batch, rows_out
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,mode,M,max_out", [("lazy", P.NMS_TF, 200, 64), ("matrix", P.NMS_TF, 200, 150), ("matrix_darknet", P.NMS_DARKNET, 200, 400),
                                                 ("general", P.NMS_TF, 600, 150)], ids=lambda v: v if isinstance(v, str) else "")
def test_70_way_tie_across_the_word_boundary(hiplib, path, mode, M, max_out):
    """Candidates 30 .. 99 of the sorted order share one score: the tie straddles candidate 64, the first word boundary of the alive set.
    Among equal scores the lower row comes first and wins."""
    key = case(rows_for(M), M, 6000 + M, distinct=True, tie=(30, 70), clusters=40)
    iou = 0.8                                                                # (tight clusters: most of the tie survives its neighbours)
    det = det_of(key)
    assert passing(det) == M
    want, want_rows = oracle(key, mode, max_out, iou=iou)
    res, rows = hiplib.op_postprocess(det[None], THR, iou, max_out, mode, return_rows=True)
    assert np.array_equal(res[0], want) and np.array_equal(rows[0], want_rows)
    order = list(P.candidates(det, THR, mode, P.SELECT_GT)[0])
    tied = want["score"] == np.sort(P.row_scores(det)[0])[::-1][30]
    where = np.array([order.index(r) for r in want_rows[tied]])
    assert (np.sort(P.row_scores(det)[0])[::-1][30:100] == want["score"][tied][0]).all()
    assert (where < 64).sum() >= 2 and (where >= 64).sum() >= 2              # kept on both sides of the boundary
    assert (np.diff(want_rows[tied]) > 0).all()                              # lower row first
    assert 5 <= len(want) < M


@pytest.mark.parametrize("M", [100, 600], ids=["fast", "general"])
def test_score_equal_to_the_threshold(hiplib, M):
    """Five rows score exactly THR: `>` leaves them out, `>=` takes them in (and keeps them: small boxes of their own)."""
    key = case(rows_for(M), M, 7000 + M, clusters=10, equal=5)
    gt = check(hiplib, key, M, P.NMS_TF, 100, select=P.SELECT_GT)
    ge = check(hiplib, key, M + 5, P.NMS_TF, 100, select=P.SELECT_GE)
    assert (gt["score"] == np.float32(THR)).sum() == 0 and (ge["score"] == np.float32(THR)).sum() == 5
    assert len(ge) == len(gt) + 5 and np.array_equal(ge[:len(gt)], gt)


@pytest.mark.parametrize("mode,max_out", [(P.NMS_TF, 20), (P.NMS_DARKNET, 400)], ids=["tf", "darknet"])
def test_mixed_batch_every_workgroup_its_own_path(hiplib, mode, max_out):
    """One launch, four images with 0, 70, 600 and 4500 candidates: nothing, a fast path, the LDS sort and the global-memory sort side
    by side, each image against its own oracle run."""
    Ms = (0, 70, 600, 4500)
    keys = [case(5000, M, 8000 + M) for M in Ms]
    batch = np.stack([det_of(k) for k in keys])
    got = hiplib.op_postprocess(batch, THR, IOU, max_out, mode)
    for k, M, g in zip(keys, Ms, got):
        assert passing(det_of(k)) == M
        want, _ = oracle(k, mode, max_out)
        assert (len(want) == 0) if M == 0 else (5 <= len(want) < M)
        assert len(g) == len(want) and np.array_equal(g, want)


@pytest.mark.parametrize("M", [513, 4097], ids=lambda v: "M%d" % v)
@pytest.mark.parametrize("mode", [P.NMS_TF, P.NMS_DARKNET, P.NMS_NUMPY_V3], ids=lambda v: NAMES[v])
def test_rows_out_on_the_general_paths(hiplib, mode, M):
    """return_rows: the row every kept record was formed from, behind the LDS sort and behind the global-memory sort."""
    if mode != P.NMS_NUMPY_V3:
        check(hiplib, case(rows_for(M), M, 9000 + M), M, mode, 100 if mode == P.NMS_TF else 400, with_rows=True)
        return
    det = planted_v3(rows_for(M), M, 9500 + M)
    want, want_rows = P.nms_v3_records(det, THR, 0.4, len(det))
    res, rows = hiplib.op_postprocess(det[None], THR, 0.4, len(det), P.NMS_NUMPY_V3, corners=True, return_rows=True)
    assert 5 <= len(want) < M
    assert np.array_equal(res[0], want) and np.array_equal(rows[0], want_rows)
