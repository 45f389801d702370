"""Frame averaging on the device (yolo_set_frame_average): the ring of activated head tensors, the decode of their mean and the
run path around them, on the three small detectors of tests/golden/frame_average_cases.npz (a yolov3-tiny shape 96 x 128 with 36 head channels,
stock yolov3-tiny and yolov2-tiny-voc at 96 x 96; synthetic weights, K + 2 noisy frames each).

  1  end to end (fp32)   darknet_boxes after every step against the compiled reference's get_network_boxes over the mean, at the tolerances
                         tests/test_gpu_darknet_veneer.py holds the unaveraged comparison to;
  2  isolation           the decoded tensor and darknet_boxes against tests/test_frame_average_host.py's restatement fed with the head_raw of a
                         twin engine with K = 1, at test_gpu_decode_forms.py's tolerance (rtol 3e-6, atol 1e-7), fp32 and bf16;
  3  streams             per-stream positions, reset_state, refused calls, time_forward, and K back to 1;
  4  graphs              detect_graph / detect_images_graph step for step against the eager calls of a twin engine, across the wrap-around;
  5  full decode         yolo_detect under K >= 2 keeps what postprocess keeps over the averaged forward;
  6  refusals            each names its reason and leaves the engine usable."""
import functools
import numpy as np
import pytest
from conftest import golden
from oracle import postprocess_ref as P
from yolo_tensorflow_amd import darknet_io as IO
import test_frame_average_host as H

pytestmark = pytest.mark.gpu
F = np.float32


@functools.lru_cache(maxsize=None)
def case(name):
    g = golden(H.FIXTURE)
    cfg = str(g[name + "_cfg"])
    heads, K, steps, means = H.case_means(g, name)
    w, h = (int(v) for v in g[name + "_src_wh"])
    return dict(g=g, name=name, cfg=cfg, flat=IO.synth_weights(IO.parse_cfg(cfg), int(g[name + "_weight_seed"]), obj_bias=0.0), heads=heads, K=K, steps=steps,
                means=means, frames=g[name + "_frames"], w=w, h=h)


def engine(hiplib, c, K=1, dtype=None, max_batch=1):
    eng = hiplib.Engine(c["cfg"], max_batch=max_batch, dtype=hiplib.FP32 if dtype is None else dtype, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(c["flat"])
    if K != 1:
        eng.set_frame_average(K)
    return eng


def gap_threshold(obj):
    """as tests/test_gpu_darknet_veneer.py finds it: the middle of the first hole wider than 8e-3 in the reference's sorted objectness -- here below
    the 21st box, so that more than 20 lie above it"""
    cand = np.sort(obj)[::-1]
    for k in range(20, len(cand) - 1):
        if cand[k] - cand[k + 1] > 8e-3:
            return float((cand[k] + cand[k + 1]) / 2)
    return None


def reference_at(kind, bb, obj, prob, thresh):
    """the golden's get_network_boxes at thresh 0 -> what it returns at `thresh` (get_yolo_detections / get_region_detections)"""
    if kind == "yolo":
        keep = obj > thresh
        return bb[keep], obj[keep], np.where(prob[keep] > thresh, prob[keep], F(0))
    on = obj > thresh
    return bb, np.where(on, obj, F(0)), np.where(on[:, None] & (prob > thresh), prob, F(0))


# ---- 1 ----
@pytest.mark.parametrize("name", H.cases())
def test_end_to_end_matches_the_compiled_reference(hiplib, name):
    c = case(name); g = c["g"]
    classes = c["heads"][0]["classes"]
    eng = engine(hiplib, c, c["K"])
    try:
        assert eng.frame_average() == c["K"]
        for t in range(c["steps"]):
            eng.forward(c["frames"][t:t + 1], want_detections=False)
            obj0, prob0 = g["%s_obj_t%d" % (name, t)], g["%s_prob_t%d" % (name, t)]
            thresh = gap_threshold(obj0)
            assert thresh is not None and (obj0 > thresh).sum() > 20
            for relative in (1, 0):
                bb, obj, prob = reference_at(c["heads"][0]["kind"], g["%s_bbox_t%d_rel%d" % (name, t, relative)], obj0, prob0, thresh)
                got = eng.darknet_boxes(0, c["w"], c["h"], thresh=thresh, relative=relative)
                assert got.shape == (len(bb), 5 + classes), (t, relative)
                scale = 1.0 if relative else max(c["w"], c["h"])
                print("%s step %d relative %d: thresh %.4f, %d boxes, max |d box| %.3g, |d obj| %.3g, |d prob| %.3g" % (
                    name, t, relative, thresh, len(bb), np.abs(got[:, :4] - bb).max(), np.abs(got[:, 4] - obj).max(), np.abs(got[:, 5:] - prob).max()))
                np.testing.assert_allclose(got[:, :4], bb, rtol=2e-3, atol=2e-3 * scale)
                np.testing.assert_allclose(got[:, 4], obj, rtol=2e-3, atol=2e-4)
                np.testing.assert_allclose(got[:, 5:], prob, rtol=2e-3, atol=2e-3)
    finally:
        eng.close()


# ---- 2 ----
# darknet_boxes at atol 1e-7.  relative = 1 meets test_gpu_decode_forms.py's rtol 3e-6 (measured: at most 1.7e-7).  relative = 0 does not: measured maximum
# 6.16e-6 (stock yolov3-tiny, fp32, step 1; bf16 5.4e-6; docs/NOTEBOOK.md "Frame averaging") -- the letterbox correction subtracts the pad offset from a centre
# that carries the decode's few units in the last place, (b.y - 0.203) / 0.594 * 120, so a box whose centre lies near the pad's edge keeps the absolute error
# and loses the magnitude; the K = 1 engine's own darknet_boxes needs up to 2.11e-5 against the same restatement on these fixtures (printed below).  Stated as
# the issue asks: the measured maximum times 2
DARKNET_BOXES_RTOL = {1: 3e-6, 0: 2 * 6.16e-6}


def activated(raw, hd):
    """head_raw of one image [gh, gw, na * attrs] -> darknet's l.output as [cell, anchor, attribute], fp32: logistic on x, y, objectness and a [yolo] head's
    classes, a [region] head's class softmax, w and h raw"""
    x = raw.reshape(hd["gh"] * hd["gw"], hd["na"], 5 + hd["classes"]).astype(F)
    sig = lambda v: F(1) / (F(1) + np.exp(-v))
    a = x.copy()
    a[..., 0:2] = sig(x[..., 0:2]); a[..., 4] = sig(x[..., 4])
    if hd["kind"] == "yolo":
        a[..., 5:] = sig(x[..., 5:])
    else:
        e = np.exp(x[..., 5:] - x[..., 5:].max(-1, keepdims=True))
        a[..., 5:] = e / e.sum(-1, keepdims=True, dtype=F)
    return a


@pytest.mark.parametrize("dtype", ["FP32", "BF16"])
@pytest.mark.parametrize("name", H.cases())
def test_decode_of_the_mean_against_the_restatement(hiplib, name, dtype):
    c = case(name); heads, K = c["heads"], c["K"]
    plain = engine(hiplib, c, 1, getattr(hiplib, dtype)); avg = engine(hiplib, c, K, getattr(hiplib, dtype))
    try:
        acts = [[] for _ in heads]
        worst_boxes = {1: 0.0, 0: 0.0}
        for t in range(c["steps"]):
            frame = c["frames"][t:t + 1]
            plain.forward(frame, want_detections=False)
            for k, hd in enumerate(heads):
                acts[k].append(activated(plain.head_raw(k, 1)[0], hd))
            # (figure only: what the UNAVERAGED darknet_boxes needs against the same restatement over this frame alone, relative = 0)
            single = [acts[k][-1] for k in range(len(heads))]
            bb1, obj1, prob1 = H.network_boxes(single, heads, c["w"], c["h"], 0)
            ref1 = np.concatenate([bb1, obj1[:, None], prob1], -1); got1 = plain.darknet_boxes(0, c["w"], c["h"], thresh=0.0, relative=0)
            print("%s %s step %d: unaveraged darknet_boxes relative 0 needs rtol %.3g" % (name, dtype, t, float(((np.abs(got1 - ref1) - 1e-7) / np.maximum(np.abs(ref1), 1e-30)).max())))
            means = [H.ring_means(acts[k], K)[-1] for k in range(len(heads))]
            want = H.decoded_rows(means, heads)
            det = avg.forward(frame)[0]
            assert det.shape == want.shape
            np.testing.assert_allclose(det, want, rtol=3e-6, atol=1e-7, err_msg="step %d" % t)
            for relative in (1, 0):
                bb, obj, prob = H.network_boxes(means, heads, c["w"], c["h"], relative)
                got = avg.darknet_boxes(0, c["w"], c["h"], thresh=0.0, relative=relative)
                assert got.shape[0] == len(bb)
                ref = np.concatenate([bb, obj[:, None], prob], -1)
                need = float(((np.abs(got - ref) - 1e-7) / np.maximum(np.abs(ref), 1e-30)).max())          # the rtol this comparison needs at atol 1e-7
                worst_boxes[relative] = max(worst_boxes[relative], need)
                print("%s %s step %d relative %d: darknet_boxes needs rtol %.3g" % (name, dtype, t, relative, need))
        assert worst_boxes[1] <= DARKNET_BOXES_RTOL[1] and worst_boxes[0] <= DARKNET_BOXES_RTOL[0], worst_boxes
    finally:
        plain.close(); avg.close()


# ---- 3 ----
def test_streams_reset_refusals_and_timing(hiplib):
    c = case("rect7"); K = c["K"]; fr = c["frames"]
    seq = [fr, fr[::-1], fr[:, :, ::-1]]                      # what stream s sees: the frames, the frames backwards, the frames mirrored
    solo = engine(hiplib, c, K); multi = engine(hiplib, c, K, max_batch=3)
    hist = [[], [], []]                                       # the frames every stream of `multi` has seen since its last reset

    def solo_last(frames):
        solo.reset_state()
        for f in frames:
            det = solo.forward(np.ascontiguousarray(f[None]))
        return det[0]

    def step(n):
        batch = np.ascontiguousarray(np.stack([seq[s][len(hist[s]) % len(fr)] for s in range(n)]))
        for s in range(n):
            hist[s].append(batch[s])
        det = multi.forward(batch)
        for s in range(n):
            assert np.array_equal(det[s], solo_last(hist[s])), "stream %d after %d steps" % (s, len(hist[s]))
    try:
        for _ in range(3):
            step(1)                                           # stream 0 alone: its position moves on, the others' do not
        step(3); step(3)                                      # stream 0 at its 4th and 5th step (wrapped), streams 1 and 2 at their 1st and 2nd
        multi.reset_state(1); hist[1] = []
        step(3)                                               # stream 1 starts over, 0 and 2 go on
        with pytest.raises(hiplib.YoloError, match="outside 1"):
            multi.forward(np.zeros((4,) + fr.shape[1:], np.uint8))          # more images than max_batch: refused before any launch
        with pytest.raises(hiplib.YoloError, match="outside 1..8"):
            multi.set_frame_average(9)
        assert multi.frame_average() == K
        step(2)
        multi.time_forward(3, 2)
        multi.time_layers(2, 1)
        step(3); step(3)
        # back to 1: today's behaviour, bit for bit
        multi.set_frame_average(1)
        assert multi.frame_average() == 1
        fresh = engine(hiplib, c, 1, max_batch=3)
        batch = np.ascontiguousarray(np.stack([seq[s][0] for s in range(3)]))
        assert np.array_equal(multi.forward(batch), fresh.forward(batch))
        thr = float(np.quantile(P.row_scores(fresh.forward(batch)[0])[0], 0.8))
        a, b = multi.detect_fused(batch, score_thr=thr, max_out=30), fresh.detect_fused(batch, score_thr=thr, max_out=30)
        assert all(len(x) > 2 and np.array_equal(x, y) for x, y in zip(a, b))
        fresh.close()
    finally:
        solo.close(); multi.close()


# ---- 4 ----
def _records(boxes, counts, hiplib, n, max_out):
    bx = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(n, max_out); ct = counts.cpu().numpy()
    return [bx[i, :ct[i]].copy() for i in range(n)]


@pytest.mark.parametrize("name", ["rect7", "voc"])
def test_graph_steps_equal_eager_steps(hiplib, name):
    import torch
    c = case(name); K = c["K"]; fr = c["frames"]; n, max_out = 2, 30
    post = dict(score_thr=0.05, iou_thr=0.45, max_out=max_out, nms_mode=hiplib.NMS_DARKNET)
    eager = engine(hiplib, c, K, max_batch=n); graph = engine(hiplib, c, K, max_batch=n)
    eager_i = engine(hiplib, c, K, max_batch=n); graph_i = engine(hiplib, c, K, max_batch=n)
    try:
        d_img = torch.zeros((n,) + fr.shape[1:], dtype=torch.uint8, device="cuda")
        boxes = torch.zeros(n * max_out * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_pix = torch.zeros(n * fr[0].size, dtype=torch.uint8, device="cuda")
        boxes_i = torch.zeros(n * max_out * 6, dtype=torch.int32, device="cuda"); counts_i = torch.zeros(n, dtype=torch.int32, device="cuda")
        kept = 0
        for t in range(K + 2):
            batch = np.ascontiguousarray(np.stack([fr[t], fr[(t + 1) % len(fr)][:, ::-1]]))
            want = eager.detect_fused(batch, **post)
            d_img.copy_(torch.from_numpy(batch).cuda()); torch.cuda.synchronize()
            graph.detect_graph(d_img, boxes, counts, **post); graph.synchronize()
            got = _records(boxes, counts, hiplib, n, max_out)
            want_i = eager_i.detect_images(list(batch), fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, **post)
            pix, descs = hiplib.pack_images(list(batch))
            d_pix[:pix.size] = torch.from_numpy(pix).cuda(); torch.cuda.synchronize()
            graph_i.detect_images_graph(d_pix, descs, boxes_i, counts_i, fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, nbytes=int(d_pix.numel()), **post)
            graph_i.synchronize()
            got_i = _records(boxes_i, counts_i, hiplib, n, max_out)
            for b in range(n):
                assert np.array_equal(got[b], want[b]), ("detect_graph", t, b)
                assert np.array_equal(got_i[b], want_i[b]), ("detect_images_graph", t, b)
                kept += len(want[b]) + len(want_i[b])
        assert kept > 20
    finally:
        for e in (eager, graph, eager_i, graph_i):
            e.close()


# ---- 5 ----
@pytest.mark.parametrize("name", H.cases())
def test_detect_runs_the_full_form_and_keeps_what_postprocess_keeps(hiplib, name):
    c = case(name); K = c["K"]
    a = engine(hiplib, c, K); b = engine(hiplib, c, K)
    try:
        for t in range(K + 1):
            frame = c["frames"][t:t + 1]
            det = b.forward(frame)
            thr = float(np.quantile(P.row_scores(det[0])[0], 0.6))
            mode = hiplib.NMS_TF if t % 2 == 0 else hiplib.NMS_DARKNET          # (a second detect on `a` would be a second step: the flavours take turns)
            got = a.detect_fused(frame, score_thr=thr, iou_thr=0.45, max_out=40, nms_mode=mode)[0]
            want = b.postprocess(1, score_thr=thr, iou_thr=0.45, max_out=40, nms_mode=mode)[0]
            assert len(want) > 2 and np.array_equal(got, want), (t, mode)
            # the decoded tensor was materialised: the flavour that needs it is served after yolo_detect (the lean decode would refuse it)
            a.postprocess(1, score_thr=1.0, nms_mode=hiplib.NMS_NUMPY_V3)
            ref, _ = P.postprocess_records(det[0], thr, 0.45, 40, mode, P.SELECT_GT)
            assert np.array_equal(want, ref)
    finally:
        a.close(); b.close()


# ---- 6 ----
def test_refusals_name_their_reason(hiplib, tmp_path):
    c = case("rect7")
    eng = engine(hiplib, c, 1, max_batch=2)
    try:
        for k in (0, 9, -3):
            with pytest.raises(hiplib.YoloError, match="outside 1..8"):
                eng.set_frame_average(k)
        assert eng.frame_average() == 1
        eng.set_frame_average(2)
        with pytest.raises(hiplib.YoloError, match="frame averaging is on"):
            eng.detect_tiled([np.zeros((150, 200, 3), np.uint8)], tile=(96, 128), overlap=(16, 16))
        assert eng.frame_average() == 2
        det = eng.forward(c["frames"][:2])                    # still usable: a step of two streams
        assert np.isfinite(det).all() and det[..., 4].max() <= 0.5 + 1e-6          # first of two slots: objectness halved
    finally:
        eng.close()
    conv = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=2\npad=1\nactivation=leaky\n\n"
    tree = tmp_path / "four.tree"
    tree.write_text("a -1\nb -1\nc 0\nd 0\n")
    nets = {
        "classifier": "[net]\nwidth=32\nheight=32\nchannels=3\n\n" + conv % 8 + "[convolutional]\nfilters=5\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\ngroups=1\n",
        r"\[detection\]": IO.cfg_text("yolov1-tiny"),
        "softmax tree": "[net]\nwidth=32\nheight=32\nchannels=3\n\n" + conv % 8 + "[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n\n"
                        "[region]\nanchors=1,1, 2,2\nbias_match=1\nclasses=4\ncoords=4\nnum=2\nsoftmax=1\ntree=%s\n" % tree,
    }
    for reason, txt in nets.items():
        e = hiplib.Engine(txt, max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
        try:
            with pytest.raises(hiplib.YoloError, match=reason):
                e.set_frame_average(3)
            assert e.frame_average() == 1
            e.set_frame_average(1)                            # off is always accepted
        finally:
            e.close()
    # fp8: heads are fp32 in every configuration, the setting is served
    txt = IO.with_input_size(IO.cfg_text("yolov3"), 96)
    e = hiplib.Engine(txt, max_batch=1, dtype=hiplib.FP8)
    try:
        e.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=0))
        img = np.random.default_rng(3).integers(0, 256, (1, 96, 96, 3), dtype=np.uint8)
        one = e.forward(img)
        e.set_frame_average(2)
        half = e.forward(img)
        assert e.frame_average() == 2 and np.allclose(half[..., 4:], one[..., 4:] / 2, rtol=1e-5, atol=1e-7)
    finally:
        e.close()


# ---- the detector classes ----
def test_detector_average_frames_and_reset_streams(hiplib):
    """YOLOV3Tiny(..., average_frames=2): detect_from_image is a step of stream 0, detect_from_images one of streams 0 .. len-1, reset_streams starts over"""
    from yolo_tensorflow_amd import detector as D
    txt = IO.cfg_text("yolov3-tiny")
    flat = IO.synth_weights(IO.parse_cfg(txt), 21, obj_bias=0.0)
    rng = np.random.default_rng(17)
    a, b = (rng.integers(0, 256, (120, 200, 3), dtype=np.uint8) for _ in range(2))
    det = D.YOLOV3Tiny(None, weights=flat, dtype=hiplib.FP32, max_batch=2, average_frames=2)
    plain = D.YOLOV3Tiny(None, weights=flat, dtype=hiplib.FP32, max_batch=2)
    same = lambda x, y: all(np.array_equal(p, q) for p, q in zip(x, y))
    try:
        assert det.engine.frame_average() == 2 and plain.engine.frame_average() == 1
        det.threshold = plain.threshold = 0.02
        one = plain.detect_from_image(a)
        assert len(one[0]) > 2 and one[0].max() > 0.25 and same(one, plain.detect_from_image(a))      # without averaging a call is a pure function of the image
        first = det.detect_from_image(a)                                            # one of two slots filled: objectness and classes halved, scores quartered
        assert len(first[0]) > 2 and first[0].max() <= 0.25
        second = det.detect_from_image(a)                                           # both slots hold the frame: 0.5 x + 0.5 x = x, the unaveraged result bit for bit
        assert same(second, one)
        det.reset_streams(0)
        assert same(det.detect_from_image(a), first)
        det.reset_streams()
        both = det.detect_from_images([a, b])                                      # streams 0 and 1, first step each
        again = det.detect_from_images([a, b])
        assert not same(again[0], both[0]) and not same(again[1], both[1])
        det.reset_streams(1)
        third = det.detect_from_images([a, b])
        assert same(third[1], both[1]) and same(third[0], again[0])
        with pytest.raises(ValueError, match="max_batch=2"):
            det.detect_from_images([a, b, a])
        assert same(det.detect_from_images([a, b])[0], again[0])                   # the refused call was no step
    finally:
        det.engine.close(); plain.engine.close()
