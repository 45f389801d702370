"""Whole-network parity through the C ABI: golden vectors from the compiled reference (darknet semantics),
the oracle in TF semantics, and size-independent properties at the BASELINE size (416x416, batch 32)."""
import numpy as np
import pytest
from conftest import golden
from oracle import yolo_ref as R
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu


def _relmax(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.mark.parametrize("name", ["mini_v3.npz", "mini_v2.npz"])
def test_mini_network_matches_compiled_reference_fp32(hiplib, name):
    """Every layer output of the reference's own C forward pass (golden), fp32 device path, darknet semantics.
    Tolerance 5e-4 of each tensor's scale: darknet's CPU batch-norm uses sqrt(var)+1e-6 where the folded
    weights use sqrt(var+1e-5) and the summation order differs."""
    g = golden(name)
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    eng.set_weights(g["weights"])
    eng.forward(g["image_u8"][None], scale=1.0 / 255.0)
    secs = IO.parse_cfg(str(g["cfg"]))
    for i, s in enumerate(secs[1:]):
        if s["type"] in ("yolo", "region"):
            continue
        got = eng.layer_output(i, 1)
        ref = g["layer_%02d" % i]
        assert got.shape == ref.shape
        assert _relmax(got, ref) < 5e-4, "layer %d (%s)" % (i, s["type"])
    eng.close()


@pytest.mark.parametrize("name", ["mini_v3.npz", "mini_v2.npz"])
def test_mini_network_bf16_tracks_reference(hiplib, name):
    g = golden(name)
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.BF16, semantics=hiplib.SEM_DARKNET, keep_layers=True)
    eng.set_weights(g["weights"])
    eng.forward(g["image_u8"][None])
    secs = IO.parse_cfg(str(g["cfg"]))
    for i, s in enumerate(secs[1:]):
        if s["type"] in ("yolo", "region"):
            continue
        # bf16 storage: 2^-8 relative per stored tensor, compounding over <= 13 layers
        assert _relmax(eng.layer_output(i, 1), g["layer_%02d" % i]) < 3e-2, "layer %d" % i
    eng.close()


def test_mini_v3_boxes_match_darknet(hiplib):
    """Decoded candidates == get_network_boxes of the compiled reference (fp32 path)."""
    g = golden("mini_v3.npz")
    eng = hiplib.Engine(str(g["cfg"]), max_batch=1, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(g["weights"])
    det = eng.forward(g["image_u8"][None])[0]
    keep = det[:, 4] > float(g["thresh"])
    assert keep.sum() == len(g["boxes_raw"])
    np.testing.assert_allclose(det[keep, :4], g["boxes_raw"], rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(det[keep, 4], g["obj_raw"], rtol=2e-3, atol=2e-4)
    eng.close()


@pytest.mark.parametrize("cfg,size", [("yolov3", 96), ("yolov2", 96), ("yolov3-tiny", 96), ("yolov2-tiny-voc", 96)])
def test_tf_semantics_network_vs_oracle(hiplib, cfg, size):
    txt = IO.with_input_size(IO.cfg_text(cfg), size)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=0)
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    x01 = img.astype(np.float32) / np.float32(255)
    osecs = R.parse_cfg(txt); params = R.unflatten_weights(flat, osecs)
    is_v3 = any(s["type"] == "yolo" for s in osecs)
    for dtype, emu, tol in ((hiplib.FP32, False, 2e-4), (hiplib.BF16, True, 3e-2)):
        eng = hiplib.Engine(txt, max_batch=2, dtype=dtype, keep_layers=True)
        eng.set_weights(flat)
        det = eng.forward(img)
        heads, outs = R.forward(osecs, params, R.to_bf16(x01) if emu else x01, emulate_bf16=emu, collect=True)
        for i, o in enumerate(outs):
            if o is not None:
                assert _relmax(eng.layer_output(i, 2), o) < tol, "%s layer %d dtype %d" % (cfg, i, dtype)
        if is_v3:
            ref = R.yolo_v3_detections(heads, size, ratio=True)
        else:
            s, raw = heads[0]
            bx, ob, cl = R.region_decode(raw, R.yolo_anchors(s), int(s["classes"]))
            b = bx.reshape(2, -1, 4)
            ref = np.concatenate([np.stack([(b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1),
                                  ob.reshape(2, -1, 1), cl.reshape(2, -1, cl.shape[-1])], -1)
        assert det.shape == ref.shape
        np.testing.assert_allclose(det, ref, rtol=tol * 10, atol=tol)
        eng.close()


def _iou(a, b):
    ix = max(0.0, min(a[2], b[2]) - max(a[0], b[0])); iy = max(0.0, min(a[3], b[3]) - max(a[1], b[1]))
    inter = ix * iy
    return inter / ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1]) - inter + 1e-12)


@pytest.fixture(scope="module")
def v3_416(hiplib):
    txt = IO.cfg_text("yolov3")
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=0)
    eng = hiplib.Engine(txt, max_batch=32)
    eng.set_weights(flat)
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (32, 416, 416, 3), dtype=np.uint8)
    yield eng, txt, flat, img
    eng.close()


def test_full_size_boxes_vs_oracle_one_image(hiplib, v3_416):
    """YOLOv3-416 (BASELINE config), one image: device boxes vs the fp32 oracle in TF semantics.
    Stated tolerance: fp32 path IoU >= 0.999 and |dscore| <= 1e-3; bf16 path IoU >= 0.99 and |dscore| <= 1e-2 (the bounds of
    tests/test_gpu_tuned.py, which covers all 32 images), fp16 storage IoU >= 0.998 and |dscore| <= 1e-3, for
    every oracle box whose score clears the threshold by more than that margin (threshold-flip band reported apart)."""
    eng, txt, flat, img = v3_416
    osecs = R.parse_cfg(txt); params = R.unflatten_weights(flat, osecs)
    x01 = img[:1].astype(np.float32) / np.float32(255)
    heads, _ = R.forward(osecs, params, x01)
    ref = R.yolo_v3_detections(heads, 416, ratio=True)[0]
    rb, rs, rc, ridx = R.select_threshold(ref, 0.5)
    assert len(rs) > 5
    for dtype, iou_min, ds in ((hiplib.FP32, 0.999, 1e-3), (hiplib.BF16, 0.99, 1e-2), (hiplib.FP16, 0.998, 1e-3)):
        e = eng if dtype == hiplib.BF16 else hiplib.Engine(txt, max_batch=1, dtype=dtype)
        if dtype != hiplib.BF16:
            e.set_weights(flat)
        det = e.forward(img[:1])[0]
        gb, gs, gc, gidx = R.select_threshold(det, 0.5)
        gmap = {int(r): k for k, r in enumerate(gidx)}
        checked = 0
        for k, r in enumerate(ridx):
            if rs[k] < 0.5 + ds:
                continue                      # may legitimately flip across the threshold
            assert int(r) in gmap, "candidate row %d lost (score %.4f)" % (r, rs[k])
            j = gmap[int(r)]
            assert _iou(rb[k], gb[j]) >= iou_min and abs(rs[k] - gs[j]) <= ds
            checked += 1
        assert checked > 3
        if dtype != hiplib.BF16:
            e.close()


def test_full_size_batch32_properties(hiplib, v3_416):
    eng, txt, flat, img = v3_416
    det = eng.forward(img)
    assert det.shape == (32, 10647, 85) and np.isfinite(det).all()
    # determinism: same input, same bits
    assert np.array_equal(det, eng.forward(img))
    # batch independence: an image alone == the same image inside the batch, bit for bit
    for i in (0, 17, 31):
        assert np.array_equal(eng.forward(img[i:i + 1])[0], det[i])
    # ranges promised by the decode: sigmoid outputs in [0,1], centres inside the image, sizes positive
    assert (det[..., 4:] >= 0).all() and (det[..., 4:] <= 1).all()
    assert (det[..., 0:2] >= 0).all() and (det[..., 0:2] <= 1).all() and (det[..., 2:4] > 0).all()
    # postprocess invariants (the API refuses to post-process more images than the last forward ran)
    with pytest.raises(hiplib.YoloError, match="last forward"):
        eng.postprocess(32)
    eng.forward(img, want_detections=False)
    res = eng.postprocess(32, score_thr=0.5, iou_thr=0.5, max_out=20)
    for b, r in enumerate(res):
        assert len(r) <= 20
        assert (np.diff(r["score"]) <= 0).all() and (r["score"] > 0.5).all()
        for i in range(len(r)):
            for j in range(i):
                bi = (r["x0"][i], r["y0"][i], r["x1"][i], r["y1"][i]); bj = (r["x0"][j], r["y0"][j], r["x1"][j], r["y1"][j])
                assert _iou(bi, bj) <= 0.5 + 1e-5
        # and equal to the oracle's tail applied to the device's own decoded tensor (bit-exact)
        ob, os_, oc = R.detect_v3_tf(det[b], 0.5, 0.5, 20)
        assert np.array_equal(r["score"], os_) and np.array_equal(r["cls"], oc)


def test_device_resident_input_and_u8_resize(hiplib, v3_416):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the GPU in this process")
    eng, txt, flat, img = v3_416
    host = eng.forward(img[:4])
    dev = eng.forward(torch.from_numpy(img[:4]).cuda())
    assert np.array_equal(host, dev)
    f32 = eng.forward(img[:4].astype(np.float32))             # `inputs / 255` on float input (V3/yolo_v3.py:215)
    assert np.array_equal(host, f32)
    # arbitrary-size uint8 image: on-device legacy bilinear == oracle resize then forward
    rng = np.random.default_rng(5)
    big = rng.integers(0, 256, (576, 768, 3), dtype=np.uint8)
    a = eng.forward_image(big)
    pre = R.input_process(big, 416)                            # [1,416,416,3] float 0..1
    b = eng.forward(np.ascontiguousarray(pre), scale=1.0)
    assert np.abs(a - b).max() < 2e-2                          # bf16 input rounding of 1-ulp-different pixels


def test_errors_are_codes_not_exits(hiplib):
    eng = hiplib.Engine(IO.cfg_text("yolov3-tiny"), max_batch=2)
    with pytest.raises(hiplib.YoloError, match="before weights"):
        eng.forward(np.zeros((1, 416, 416, 3), np.uint8))
    with pytest.raises(hiplib.YoloError, match="floats"):
        eng.set_weights(np.zeros(10, np.float32))
    with pytest.raises(hiplib.YoloError, match="cannot open"):
        eng.load_weights("/nonexistent/yolov3.weights")
    eng.set_weights(IO.synth_weights(IO.parse_cfg(IO.cfg_text("yolov3-tiny")), 0))
    with pytest.raises(hiplib.YoloError, match="batch"):
        eng.forward(np.zeros((3, 416, 416, 3), np.uint8))
    with pytest.raises(hiplib.YoloError):
        hiplib.Engine("[net]\nwidth=416\nheight=416\nchannels=3\n[softmax]\n", max_batch=1)
    eng.close()


def test_weights_file_loader(hiplib, tmp_path):
    txt = IO.with_input_size(IO.cfg_text("yolov3-tiny"), 96)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, 0)
    img = np.random.default_rng(0).integers(0, 256, (1, 96, 96, 3), dtype=np.uint8)
    a = hiplib.Engine(txt); a.set_weights(flat); ref = a.forward(img); a.close()
    for mj, mn, hdr in ((0, 2, 0), (0, 1, 0), (0, 2, 5), (0, 1, 4)):
        p = str(tmp_path / "w.weights"); IO.write_weights_file(p, flat, mj, mn)
        b = hiplib.Engine(txt); b.load_weights(p, hdr)
        assert np.array_equal(b.forward(img), ref)
        b.close()


def test_config2_yolov2_416_fp32_vs_oracle(hiplib):
    """BASELINE config 2: YOLOv2 416x416 batch 1, fp32 path, Darknet .weights stream through the C ABI -> decoded
    boxes vs the fp32 oracle (TF semantics).  Tolerance: 2e-4 of the decoded tensor's scale; kept set identical."""
    txt = IO.cfg_text("yolov2")
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=0, obj_bias=0.5)
    img = np.random.default_rng(2).integers(0, 256, (1, 416, 416, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=1, dtype=hiplib.FP32)
    eng.set_weights(flat)
    det = eng.forward(img)
    osecs = R.parse_cfg(txt)
    heads, _ = R.forward(osecs, R.unflatten_weights(flat, osecs), img.astype(np.float32) / np.float32(255))
    s, raw = heads[0]
    bx, ob, cl = R.region_decode(raw, R.yolo_anchors(s), 80)
    assert det.shape == (1, 845, 85)
    b = bx.reshape(1, -1, 4)
    ref = np.concatenate([np.stack([(b[..., 0] + b[..., 2]) / 2, (b[..., 1] + b[..., 3]) / 2, b[..., 2] - b[..., 0], b[..., 3] - b[..., 1]], -1),
                          ob.reshape(1, -1, 1), cl.reshape(1, -1, 80)], -1)
    np.testing.assert_allclose(det, ref, rtol=2e-3, atol=2e-4)
    # V2/postprocess.py tail: score >= 0.5, TF NMS (10, 0.5) -- device vs oracle on the device's own decoded tensor
    got = eng.postprocess(1, score_thr=0.5, iou_thr=0.5, max_out=10, nms_mode=hiplib.NMS_TF, select_mode=hiplib.SELECT_GE)[0]
    bb, sc, lb, _ = R.region_select(np.stack([det[0, :, 0] - det[0, :, 2] * np.float32(.5), det[0, :, 1] - det[0, :, 3] * np.float32(.5),
                                               det[0, :, 0] + det[0, :, 2] * np.float32(.5), det[0, :, 1] + det[0, :, 3] * np.float32(.5)], -1),
                                    det[0, :, 4], det[0, :, 5:], 0.5)
    sel = R.tf_nms(bb[:, [1, 0, 3, 2]], sc, 10, 0.5)
    assert len(got) == len(sel) > 0
    assert np.array_equal(got["score"], sc[sel]) and np.array_equal(got["cls"], lb[sel])
    eng.close()


def test_config4_yolov3_608_shard_properties(hiplib):
    """BASELINE config 4 per-GPU shard: YOLOv3 608x608, 8 images (batch 64 over 8 GPUs).  Same size-independent
    properties as at 416: shape 22743 rows, determinism, batch independence, NMS tail equal to the oracle's."""
    txt = IO.cfg_text("yolov3-608")
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=0)
    img = np.random.default_rng(3).integers(0, 256, (8, 608, 608, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=8)
    eng.set_weights(flat)
    det = eng.forward(img)
    assert det.shape == (8, 22743, 85) and np.isfinite(det).all()
    assert np.array_equal(det, eng.forward(img))
    assert np.array_equal(eng.forward(img[5:6])[0], det[5])
    eng.forward(img, want_detections=False)
    res = eng.postprocess(8, score_thr=0.5, iou_thr=0.5, max_out=20)
    for b in range(8):
        ob, os_, oc = R.detect_v3_tf(det[b], 0.5, 0.5, 20)
        assert np.array_equal(res[b]["score"], os_) and np.array_equal(res[b]["cls"], oc)
    eng.close()


def test_detect_graph_replay_equals_eager(hiplib, v3_416):
    """The HIP-graph replay of a detect step (third call onwards) returns exactly what eager launches return."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("torch does not see the GPU in this process")
    eng, txt, flat, img = v3_416
    n, max_out = 8, 20
    d_img = torch.from_numpy(img[:n]).cuda()
    boxes = torch.zeros((n, max_out * 6), dtype=torch.int32, device="cuda"); counts = torch.zeros((n,), dtype=torch.int32, device="cuda")
    eng.forward(d_img, want_detections=False)
    want = eng.postprocess(n, score_thr=0.5, iou_thr=0.5, max_out=max_out)
    for it in range(4):                     # eager, capture, replay, replay
        boxes.zero_(); counts.zero_()
        eng.detect_graph(d_img, boxes, counts, score_thr=0.5, iou_thr=0.5, max_out=max_out)
        eng.synchronize()
        got_counts = counts.cpu().numpy(); got = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(n, max_out)
        for b in range(n):
            assert got_counts[b] == len(want[b]) and np.array_equal(got[b, :got_counts[b]], want[b]), "call %d image %d" % (it, b)
    # a different argument re-captures transparently
    eng.detect_graph(d_img, boxes, counts, score_thr=0.6, iou_thr=0.5, max_out=max_out)
    eng.synchronize()


@pytest.mark.parametrize("size", [96, 160, 224])
def test_fused_plan_equals_layer_by_layer_plan(hiplib, size):
    """The production plan (fused stem kernel for conv0+conv1+conv2, shortcuts folded into conv epilogues, pooled
    buffers) gives bit-identical detections to the introspection plan that materialises every layer (keep_layers=1):
    the fusions keep every intermediate rounding and the K order of the unfused kernels."""
    txt = IO.with_input_size(IO.cfg_text("yolov3"), size)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=3)
    img = np.random.default_rng(size).integers(0, 256, (3, size, size, 3), dtype=np.uint8)
    dets = []
    for keep in (False, True):
        eng = hiplib.Engine(txt, max_batch=3, dtype=hiplib.BF16, keep_layers=keep)
        eng.set_weights(flat)
        dets.append(eng.forward(img))
        eng.close()
    assert np.array_equal(dets[0], dets[1])


@pytest.mark.parametrize("dtype_name", ["bf16", "fp8"])
def test_fused_1x1_tail_equals_separate_launch(hiplib, dtype_name):
    """A 1x1 conv folded into the epilogue of the 3x3 conv that feeds it (tile plan code cfg + 10000) gives the same
    bits as the two separate launches, on every producer the planner marks as fusable (with and without a shortcut),
    in the bf16 and in the fp8 configuration (there with non-trivial activation scales)."""
    dtype = hiplib.BF16 if dtype_name == "bf16" else hiplib.FP8
    size = 160
    txt = IO.with_input_size(IO.cfg_text("yolov3"), size)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=5)
    img = np.random.default_rng(9).integers(0, 256, (2, size, size, 3), dtype=np.uint8)
    scales = np.ones(len(secs) - 1, np.float32); scales[::2] = 0.5; scales[1::4] = 0.25
    ref = hiplib.Engine(txt, max_batch=2, dtype=dtype, keep_layers=True)
    if dtype == hiplib.FP8:
        ref.set_act_scales(scales)
    ref.set_weights(flat); want = ref.forward(img); ref.close()
    eng = hiplib.Engine(txt, max_batch=2, dtype=dtype)
    if dtype == hiplib.FP8:
        eng.set_act_scales(scales)
    eng.set_weights(flat)
    cfgs = np.full(eng.num_layers, -1, np.int32)
    fused = 0
    for i, s in enumerate(secs[1:]):
        if s["type"] != "convolutional" or int(s["filters"]) not in (128, 256):
            continue
        trial = cfgs.copy(); trial[i] = 32 + 10000
        try:
            eng.set_tile_configs(trial)
            cfgs = trial; fused += 1
        except hiplib.YoloError:
            pass                                            # not followed by a foldable 1x1 conv
    assert fused >= 10                                      # 8 + 2 producers with 256 channels (the 52x52-style stages)
    eng.set_tile_configs(cfgs)
    assert np.array_equal(eng.get_tile_configs()[cfgs >= 0], cfgs[cfgs >= 0])
    got = eng.forward(img)
    assert np.array_equal(got, want)
    # and through the graph path, twice (capture + replay)
    import torch
    dimg = torch.from_numpy(img).cuda(); boxes = torch.zeros((2, 20 * 6), dtype=torch.int32, device="cuda"); counts = torch.zeros((2,), dtype=torch.int32, device="cuda")
    for _ in range(3):
        eng.detect_graph(dimg, boxes, counts, score_thr=0.3, iou_thr=0.5, max_out=20)
    eng.synchronize()
    eng.close()


STEM_NET = """[net]
width=416
height=416
channels=3

[convolutional]
batch_normalize=1
filters=32
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=32
size=1
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[shortcut]
from=-3
activation=linear

[maxpool]
size=2
stride=2

[maxpool]
size=2
stride=2

[maxpool]
size=2
stride=2

[convolutional]
filters=255
size=1
stride=1
pad=1
activation=linear

[yolo]
mask=0,1,2
anchors=10,13, 16,30, 33,23
classes=80
num=3
"""


@pytest.mark.parametrize("size,batch,shortcut", [(416, 12, True), (400, 7, False), (400, 5, True), (80, 3, False)])
def test_halo32_ring_of_tiles_equals_the_tiled_kernel(hiplib, monkeypatch, size, batch, shortcut):
    """conv_halo_c32_c64 keeps input and shortcut tiles of TWO tiles ahead in flight (rings of three LDS slots, one counted vmcnt per
    tile): run it deep into its steady state -- up to 16 tiles per workgroup, with and without the shortcut, on grids its 8 x 16 tiles
    cover exactly (208 x 208) and raggedly (200 = 12.5 x 16; 40 = 2.5 x 16: the out-of-image stores are issued and dropped) -- and compare the whole first stage with the
    plan that runs the same layer through the tiled kernel (YOLO_NO_HALO): same K order, bit-identical."""
    txt = STEM_NET.replace("width=416", "width=%d" % size).replace("height=416", "height=%d" % size)
    if not shortcut:
        txt = txt.replace("[shortcut]\nfrom=-3\nactivation=linear\n\n", "")
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=21)
    img = np.random.default_rng(size + batch).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)
    outs = []
    for no_halo in (False, True):
        if no_halo: monkeypatch.setenv("YOLO_NO_HALO", "1")
        else: monkeypatch.delenv("YOLO_NO_HALO", raising=False)
        eng = hiplib.Engine(txt, max_batch=batch, keep_layers=True)
        eng.set_weights(flat)
        eng.forward(img)
        last = 4 if shortcut else 3
        outs.append(eng.layer_output(last, batch))
        eng.close()
    assert outs[0].shape == (batch, size // 2, size // 2, 64) and np.abs(outs[0]).max() > 0.1
    assert np.array_equal(outs[0], outs[1])


S2_NET = """[net]
width=208
height=208
channels=3

[convolutional]
batch_normalize=1
filters=64
size=3
stride=1
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=128
size=3
stride=2
pad=1
activation=%s

[maxpool]
size=2
stride=2

[maxpool]
size=2
stride=2

[convolutional]
filters=255
size=1
stride=1
pad=1
activation=linear

[yolo]
mask=0,1,2
anchors=10,13, 16,30, 33,23
classes=80
num=3
"""


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("size,batch,act", [(208, 20, "leaky"), (72, 3, "leaky"), (40, 2, "linear"), (104, 33, "leaky"), (27, 3, "leaky")])
def test_stride2_c64_kernel_equals_the_tiled_kernel_and_tracks_the_oracle(hiplib, monkeypatch, dtype_name, size, batch, act):
    """conv_s2.hip (3x3 / stride 2, 64 -> 128: darknet-53's cfg layer 5; the window of a tile staged once in LDS two tiles ahead, filters
    in registers) against the tiled kernel on the same layer (YOLO_NO_S2; same K order: bit-identical) deep into the ring of tiles (up to
    22 per workgroup), on output grids its 8 x 8 tiles cover exactly (104, 52) and raggedly (36 = 4.5 x 8, 20 = 2.5 x 8; 14 from an odd 27-pixel input), and against
    the oracle at the device's storage precision (bf16)."""
    txt = (S2_NET % act).replace("width=208", "width=%d" % size).replace("height=208", "height=%d" % size)
    if size % 8:                                 # an ODD input edge (27 -> 14 output pixels: the last window row / column is padding): no pooling behind it
        txt = txt.replace("[maxpool]\nsize=2\nstride=2\n\n", "")
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=31)
    img = np.random.default_rng(size + batch).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)
    dtype = hiplib.BF16 if dtype_name == "bf16" else hiplib.FP16
    outs = []
    for no_s2 in (False, True):
        if no_s2: monkeypatch.setenv("YOLO_NO_S2", "1")
        else: monkeypatch.delenv("YOLO_NO_S2", raising=False)
        eng = hiplib.Engine(txt, max_batch=batch, dtype=dtype, keep_layers=True)
        eng.set_weights(flat)
        eng.forward(img)
        outs.append(eng.layer_output(1, batch))
        eng.close()
    assert outs[0].shape == (batch, (size + 1) // 2, (size + 1) // 2, 128) and np.abs(outs[0]).max() > 0.1
    assert np.array_equal(outs[0], outs[1])
    if dtype_name == "bf16" and batch <= 3:
        osecs = R.parse_cfg(txt); params = R.unflatten_weights(flat, osecs)
        _, ref = R.forward(osecs, params, R.to_bf16(img.astype(np.float32) / np.float32(255)), emulate_bf16=True, collect=True)
        err = np.abs(outs[0] - ref[1])
        assert (err <= 2.0 ** -6 * np.abs(ref[1]) + 4e-2).all() and float(err.mean()) < 2e-3


def test_stem_and_halo_kernels_at_full_size_vs_oracle(hiplib):
    """The two special kernels of the first stage at their real geometry (416x416 in, 208x208 out, batch 2): conv_stem_c32_c64
    (conv0 + conv1 + conv2 in one launch) and conv_halo_c32_c64 (conv3 + shortcut).  (a) every layer of the layer-by-layer
    plan -- which runs conv3 through the halo kernel too -- against the oracle at the device's storage precision; (b) the production
    plan (fused stem, nothing materialised) bit-identical to the layer-by-layer plan."""
    secs = IO.parse_cfg(STEM_NET); flat = IO.synth_weights(secs, seed=6)
    img = np.random.default_rng(8).integers(0, 256, (2, 416, 416, 3), dtype=np.uint8)
    osecs = R.parse_cfg(STEM_NET); params = R.unflatten_weights(flat, osecs)
    _, outs = R.forward(osecs, params, R.to_bf16(img.astype(np.float32) / np.float32(255)), emulate_bf16=True, collect=True)
    full = hiplib.Engine(STEM_NET, max_batch=2, keep_layers=True)
    full.set_weights(flat)
    det_layers = full.forward(img)
    for i in range(5):
        got = full.layer_output(i, 2)
        assert got.shape == outs[i].shape == (2, (416, 208, 208, 208, 208)[i], (416, 208, 208, 208, 208)[i], (32, 64, 32, 64, 64)[i])
        err = np.abs(got - outs[i])
        # one bf16 ulp of the value plus the ulp of the pre-rounding operands that flipped upstream
        assert (err <= 2.0 ** -6 * np.abs(outs[i]) + 4e-2).all(), "layer %d: max err %.3e" % (i, err.max())
        assert float(err.mean()) < 2e-3, "layer %d: mean err %.3e" % (i, err.mean())
    full.close()
    prod = hiplib.Engine(STEM_NET, max_batch=2)
    prod.set_weights(flat)
    det = prod.forward(img)
    prod.close()
    assert np.array_equal(det, det_layers)


def test_fused_1x1_tail_halo_forms_full_size(hiplib, monkeypatch):
    """The same at 416 x 416, where the free-running halo forms apply: 256-channel producers under f176c256 (cfg 40), 128-channel
    producers (the 104 x 104 stage) under f176c128 (cfg 41, four tail channel tiles over eight waves), against the plan that
    materialises every layer.  (YOLO_NO_RESBLOCK: the production plan runs the 104 x 104 stage as fused residual blocks, conv_block.hip,
    which leaves no 128-channel producer for a tail; this test is about the tail form.)"""
    monkeypatch.setenv("YOLO_NO_RESBLOCK", "1")
    txt = IO.cfg_text("yolov3")
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=6)
    img = np.random.default_rng(10).integers(0, 256, (1, 416, 416, 3), dtype=np.uint8)
    ref = hiplib.Engine(txt, max_batch=1, dtype=hiplib.BF16, keep_layers=True)
    ref.set_weights(flat); want = ref.forward(img); ref.close()
    eng = hiplib.Engine(txt, max_batch=1, dtype=hiplib.BF16)
    eng.set_weights(flat)
    cfgs = np.full(eng.num_layers, -1, np.int32)
    fused = {128: 0, 256: 0}
    for i, s in enumerate(secs[1:]):
        if s["type"] != "convolutional" or int(s["filters"]) not in (128, 256):
            continue
        # 128-channel producers: f176c128 with two (41) and with three (43) filter stages, alternately
        for cand in (((43, 41) if fused[128] % 2 == 0 else (41, 43)) if int(s["filters"]) == 128 else (40, 32)):
            trial = cfgs.copy(); trial[i] = cand + 10000
            try:
                eng.set_tile_configs(trial)
                cfgs = trial; fused[int(s["filters"])] += 1
                break
            except hiplib.YoloError:
                pass
    assert fused[256] >= 10 and fused[128] >= 1, fused
    eng.set_tile_configs(cfgs)
    assert np.array_equal(eng.forward(img), want)
    eng.close()


@pytest.mark.parametrize("cfg", ["yolov2", "yolov3-tiny", "yolov2-tiny-voc"])
def test_halo_forms_on_the_other_topologies_full_size(hiplib, cfg):
    """The halo-staged / free-running 3x3 forms were tuned on YOLOv3; at 416 x 416 they also apply to the 13 / 26 / 52 / 104 / 208 grids
    of the other topologies (other channel counts: 1024 -> 1024, 3072 -> 1024 after the reorg concat, 512 -> 1024 ...).  Every layer
    that accepts one runs it; the decoded tensor must equal the default plan's bit for bit."""
    txt = IO.cfg_text(cfg)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=14)
    img = np.random.default_rng(15).integers(0, 256, (2, 416, 416, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.BF16)
    eng.set_weights(flat)
    want = eng.forward(img).copy()
    cfgs = np.full(eng.num_layers, -1, np.int32)
    used = {}
    for i, s in enumerate(secs[1:]):
        if s["type"] != "convolutional" or int(s["size"]) != 3:
            continue
        for cand in ((40, 43, 41, 36) if len(used) % 2 == 0 else (43, 41, 40, 36)):
            trial = cfgs.copy(); trial[i] = cand
            try:
                eng.set_tile_configs(trial)
                cfgs = trial; used[i] = cand
                break
            except hiplib.YoloError:
                pass
    assert len(used) >= 3, used
    eng.set_tile_configs(cfgs)
    assert np.array_equal(eng.forward(img), want)
    eng.close()



@pytest.mark.parametrize("dtype_name,size,batch", [("bf16", 416, 3), ("fp16", 416, 2), ("bf16", 416, 1), ("bf16", 608, 2), ("fp16", 608, 1)])
def test_fused_residual_block_equals_the_two_layers(hiplib, monkeypatch, dtype_name, size, batch):
    """conv_block.hip (1x1 128 -> 64, 3x3 64 -> 128 and the shortcut of darknet-53's 128-channel stage in one launch, whenever that stage's
    grid is whole 13 x 13 blocks -- 104 x 104 at 416 -- or, round 4, ragged ones that waste at most 15 %: 152 x 152 at 608) against the same engine with the block
    run as its two conv launches: decoded tensors bit for bit; 8 x 8 blocks per image, border and interior ones, batches of 1 to 3."""
    dtype = {"bf16": hiplib.BF16, "fp16": hiplib.FP16}[dtype_name]
    txt = IO.with_input_size(IO.cfg_text("yolov3"), size)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=21)
    img = np.random.default_rng(22).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=batch, dtype=dtype)
    eng.set_weights(flat); got = eng.forward(img); fused_bytes = eng.conv_bytes(batch); eng.close()
    monkeypatch.setenv("YOLO_NO_RESBLOCK", "1")
    ref = hiplib.Engine(txt, max_batch=batch, dtype=dtype)
    ref.set_weights(flat); want = ref.forward(img); plain_bytes = ref.conv_bytes(batch); ref.close()
    # the fused plan really ran: two blocks, each without the 64-channel tensor written once and read once
    g = size // 4
    assert plain_bytes - fused_bytes == 2 * 2 * batch * g * g * 64 * 2
    assert np.isfinite(got).all() and np.array_equal(got, want)


@pytest.mark.parametrize("dtype_name,batch,size,cfgs", [("bf16", 3, 416, (40,)), ("fp16", 1, 416, (40,)), ("bf16", 2, 608, (54,))])
def test_head_as_the_tail_of_its_3x3_equals_the_separate_launch(hiplib, dtype_name, batch, size, cfgs):
    """Round 5: darknet-53's 52 x 52 detection head (1x1, 256 -> 255, fp32, linear; cfg layer 105) computed in the epilogue of the 3x3 conv in
    front of it (cfg layer 104, halo-staged 176 x 256 form) from the finished tile in LDS -- the plan code `40 + 10000` on layer 104 -- against
    the plan that launches the head conv itself: decoded tensors, raw head tensors and detections bit for bit (same K order, fp32 accumulator
    + bias, the objectness plane the lean decode reads included)."""
    dtype = {"bf16": hiplib.BF16, "fp16": hiplib.FP16}[dtype_name]
    txt = IO.with_input_size(IO.cfg_text("yolov3"), size)            # (608: the 76 x 76 head behind the 10 x 19-block form, configuration 54)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=31)
    img = np.random.default_rng(32).integers(0, 256, (batch, size, size, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=batch, dtype=dtype)
    eng.set_weights(flat)
    plain = eng.get_tile_configs().copy()
    plain = np.where(plain >= 10000, plain - 10000, plain)
    eng.set_tile_configs(plain)
    want = eng.forward(img); want_raw = eng.head_raw(2, batch)
    want_boxes = eng.detect(img, score_thr=0.5, iou_thr=0.5, max_out=20)
    layer = [i for i, s in enumerate(secs[1:]) if s["type"] == "yolo"][2] - 2            # the 3x3 in front of the last head conv
    assert int(secs[1 + layer]["filters"]) == 256 and int(secs[1 + layer]["size"]) == 3
    for cfg in cfgs:
        trial = plain.copy(); trial[layer] = 10000 + cfg
        eng.set_tile_configs(trial)
        got = eng.forward(img)
        assert np.array_equal(got, want), cfg
        assert np.array_equal(eng.head_raw(2, batch), want_raw), cfg
        boxes = eng.detect(img, score_thr=0.5, iou_thr=0.5, max_out=20)              # the lean path: objectness plane written by the tail
        for b in range(batch):
            assert np.array_equal(boxes[b], want_boxes[b]), (cfg, b)
    # a tile configuration that cannot host a head is refused
    bad = plain.copy(); bad[layer] = 10000 + 36
    with pytest.raises(hiplib.YoloError):
        eng.set_tile_configs(bad)
    eng.close()


def _with_classes(txt, classes):
    """yolov3 cfg text with another class count: `classes=` of every [yolo] section and the filter count of the head conv in front of it."""
    out = []; secs = txt.split("[")
    for k, sec in enumerate(secs):
        if sec.startswith("yolo]"):
            sec = "\n".join(("classes=%d" % classes) if l.split("=")[0].strip() == "classes" else l for l in sec.split("\n"))
            prev = out[-1].split("\n")
            out[-1] = "\n".join(("filters=%d" % (3 * (5 + classes))) if l.split("=")[0].strip() == "filters" else l for l in prev)
        out.append(sec)
    return "[".join(out)


@pytest.mark.parametrize("classes", [20, 1])
def test_head_tail_with_few_filters_reads_inside_its_fragment_image(hiplib, classes):
    """a detection head fused as the tail of its 3x3 is read by all eight waves, 32 filter rows each, whatever its filter count --
    a VOC head (75 filters) or a 1-class head (18) used to get a fragment image of roundup(filters, 16) rows and was read past its end.
    The image is now the padded 256 rows: the fused plan equals the plan that launches the head, bit for bit, at both class counts."""
    txt = _with_classes(IO.cfg_text("yolov3"), classes)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=33)
    img = np.random.default_rng(34).integers(0, 256, (2, 416, 416, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=2, dtype=hiplib.BF16)
    eng.set_weights(flat)
    plain = eng.get_tile_configs().copy(); plain = np.where(plain >= 10000, plain - 10000, plain)
    eng.set_tile_configs(plain)
    want = eng.forward(img); want_raw = eng.head_raw(2, 2)
    assert want.shape[-1] == 5 + classes
    layer = [i for i, s in enumerate(secs[1:]) if s["type"] == "yolo"][2] - 2
    trial = plain.copy(); trial[layer] = 10000 + 40
    eng.set_tile_configs(trial)
    assert np.array_equal(eng.forward(img), want)
    assert np.array_equal(eng.head_raw(2, 2), want_raw)
    eng.close()


def test_tail_flag_on_a_fixed_kernel_is_refused(hiplib):
    """the window-staged stride-2 layer (and every other fixed kernel: stem, conv3, fused blocks) hosts no 1x1 tail -- its launch
    ignores the tail's arguments, so a plan carrying `cfg + 10000` there would silently skip the 1x1 conv.  The planner no longer offers it
    as a producer and yolo_set_tile_configs refuses the flag; at 320 x 320 (where the following 1x1 is NOT absorbed by a fused block) the
    network still equals the oracle-checked layer-by-layer plan."""
    for size in (416, 320):
        txt = IO.with_input_size(IO.cfg_text("yolov3"), size)
        eng = hiplib.Engine(txt, max_batch=1, dtype=hiplib.BF16)
        eng.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=35))
        cfgs = eng.get_tile_configs().copy()
        bad = cfgs.copy(); bad[5] = 10000 + 36              # cfg layer 5: 3x3 / stride 2, 64 -> 128
        with pytest.raises(hiplib.YoloError):
            eng.set_tile_configs(bad)
        eng.close()
    txt = IO.with_input_size(IO.cfg_text("yolov3"), 320)
    secs = IO.parse_cfg(txt); flat = IO.synth_weights(secs, seed=35)
    img = np.random.default_rng(36).integers(0, 256, (1, 320, 320, 3), dtype=np.uint8)
    eng = hiplib.Engine(txt, max_batch=1, dtype=hiplib.BF16); eng.set_weights(flat)
    got = eng.forward(img); eng.close()
    ref = hiplib.Engine(txt, max_batch=1, dtype=hiplib.BF16, keep_layers=True); ref.set_weights(flat)
    want = ref.forward(img); ref.close()
    assert np.array_equal(got, want)
