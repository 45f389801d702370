"""Image networks of any channel count ([net] yolo_input=planes) on the device: the four fixtures of the compiled reference layer by layer, the input
staging kernels in their N-plane form (the three formats of yolo_forward; the stretch, letterbox and centre-crop fits of ragged batches; the single-image
entry points) against the three-channel form of the same arithmetic and against the reference's own letterbox_image / resize_min + crop_image, the
refusals, the darknet veneer, an export artifact and the captured step.  Every shape is at most 32 x 32."""
import ctypes as C
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO

pytestmark = pytest.mark.gpu

FIXTURES = ["mini_planes_grey", "mini_planes_rgbd", "mini_planes_nine", "mini_planes_17"]
MARGIN_TOL = 5e-4                            # the fp32 bound of test_gpu_unet.py, as a share of the tensor's largest value
TOL16 = {"bf16": 3e-2, "fp16": 4e-3}         # test_gpu_unet.py's bounds of a 16-bit network's final tensor
PLANES = [1, 4, 9]


def _relmax(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / (np.abs(b).max() + 1e-12))


def _bf16(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    return u.astype(np.uint32).view(np.float32)


def _stored(hiplib, x, dtype):
    return _bf16(x) if dtype == hiplib.BF16 else np.asarray(x, np.float32).astype(np.float16).astype(np.float32) if dtype == hiplib.FP16 else np.asarray(x, dtype=np.float32)


def _fixture_engine(hiplib, g, dtype, batch=3, keep=False):
    eng = hiplib.Engine(IO.with_planes_input(str(g["cfg"])), max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET, keep_layers=keep)
    assert eng.weights_count() == g["weights"].size and eng.input_channels == g["image_u8"].shape[2]
    eng.set_weights(g["weights"])
    return eng


def _final(hiplib, eng, g, n):
    """the network's final tensor of the last forward and the fixture's: a detector's head conv, a classifier's probabilities, a map"""
    secs = IO.parse_cfg(str(g["cfg"]))[1:]
    if secs[-1]["type"] == "yolo":
        return eng.head_raw(0, n), g["layer_%02d" % (len(secs) - 2)]
    if secs[-1]["type"] == "softmax":
        return eng.last_layer_output(n).reshape(n, 1, 1, -1), g["layer_%02d" % (len(secs) - 1)]
    return eng.output_map(n), g["layer_%02d" % (len(secs) - 1)]


# ---- 1: the fixtures ----
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_matches_compiled_reference_fp32(hiplib, name):
    """every layer of the reference's forward pass, fp32, batch 3 (the fixture's input three times): 5e-4 of each tensor's largest value, every image"""
    g = golden(name + ".npz")
    eng = _fixture_engine(hiplib, g, hiplib.FP32, keep=True)
    x = np.repeat(g["image_u8"][None], 3, axis=0)
    det = eng.forward(x, want_detections=eng.rows > 0)
    for i, s in enumerate(IO.parse_cfg(str(g["cfg"]))[1:]):
        if s["type"] == "yolo":
            continue
        got, ref = eng.layer_output(i, 3), g["layer_%02d" % i]
        assert got.shape[1:] == ref.shape[1:], "layer %d (%s)" % (i, s["type"])
        for b in range(3):
            r = _relmax(got[b], ref[0])
            print("%s layer %d (%s) image %d: relmax %.3e" % (name, i, s["type"], b, r))
            assert r < MARGIN_TOL, "layer %d (%s) image %d: %.3e" % (i, s["type"], b, r)
    if name == "mini_planes_grey":          # the decoded candidates against the reference's get_network_boxes (test_gpu_grouped.py's comparison of mini_dw_v3)
        for b in range(3):
            keep = det[b][:, 4] > float(g["thresh"])
            assert keep.sum() == len(g["boxes_raw"])
            np.testing.assert_allclose(det[b][keep, :4], g["boxes_raw"], rtol=2e-3, atol=2e-4)
            np.testing.assert_allclose(det[b][keep, 4], g["obj_raw"], rtol=2e-3, atol=2e-4)
    eng.close()
    # the plan that keeps no layer gives the same final tensor
    lean = _fixture_engine(hiplib, g, hiplib.FP32)
    lean.forward(x, want_detections=False)
    kept = _fixture_engine(hiplib, g, hiplib.FP32, keep=True)
    kept.forward(x, want_detections=False)
    assert np.array_equal(_final(hiplib, lean, g, 3)[0], _final(hiplib, kept, g, 3)[0])
    lean.close(); kept.close()


@pytest.mark.parametrize("dtype_name", ["bf16", "fp16"])
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_16_bit_final_tensor(hiplib, name, dtype_name):
    g = golden(name + ".npz")
    eng = _fixture_engine(hiplib, g, getattr(hiplib, dtype_name.upper()))
    eng.forward(np.repeat(g["image_u8"][None], 3, axis=0), want_detections=False)
    got, ref = _final(hiplib, eng, g, 3)
    eng.close()
    for b in range(3):
        r = _relmax(got[b], ref[0])
        print("%s %s image %d: relmax of the final tensor %.3e" % (name, dtype_name, b, r))
        assert r <= TOL16[dtype_name]


# ---- 2: the staged input ----
def _staging_cfg(n, net_h=16, net_w=16, extra=""):
    """a classifier over n planes whose first layer is a 1x1 conv: what is checked is the staged input itself (Engine.staged_input)"""
    return ("[net]\nyolo_input=planes\nheight=%d\nwidth=%d\nchannels=%d\n%s\n" % (net_h, net_w, n, extra) +
            "[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")


def _staging_engine(hiplib, n, dtype, batch=3, net_h=16, net_w=16, extra=""):
    cfg = _staging_cfg(n, net_h, net_w, extra)
    eng = hiplib.Engine(cfg, max_batch=batch, dtype=dtype, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(cfg), seed=3))
    return eng


@pytest.mark.parametrize("dtype_name", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("n", PLANES + [17])
def test_forward_formats_stage_the_same_input(hiplib, n, dtype_name):
    """uint8 HWC, float HWC and planar float of the same 13 x 11 images (3 x 143 pixels: more than one block) give the same staged tensor: value x scale in
    fp32, rounded once to the storage type; the channels n .. roundup(n, 8) - 1 are zero; yolo_input_mul / yolo_input_add touch the real channels only"""
    dtype = getattr(hiplib, dtype_name.upper())
    img = np.random.default_rng(n).integers(0, 256, (3, 13, 11, n), dtype=np.uint8)
    scale = np.float32(1.0 / 255.0)
    want = img.astype(np.float32) * scale
    for extra, mul, add in (("", None, None), ("yolo_input_mul=2\nyolo_input_add=-1\n", np.float32(2), np.float32(-1))):
        eng = _staging_engine(hiplib, n, dtype, net_h=13, net_w=11, extra=extra)
        assert eng.input_channels == n
        w = want if mul is None else want * mul + add
        staged = []
        for images, fmt in ((img, hiplib.IMG_U8), (img.astype(np.float32), hiplib.IMG_F32), (np.ascontiguousarray(img.astype(np.float32).transpose(0, 3, 1, 2)), hiplib.IMG_F32_CHW)):
            eng.forward(images, scale=float(scale), want_detections=False, fmt=fmt)
            staged.append(eng.staged_input(3))
            assert staged[-1].shape == (3, 13, 11, (n + 7) // 8 * 8)
            assert np.array_equal(staged[-1][..., :n], _stored(hiplib, w, dtype)), fmt
            assert not staged[-1][..., n:].any(), fmt
        p = eng.classify(img, top_k=0)
        assert np.isfinite(p).all() and np.allclose(p.sum(axis=1), 1, atol=1e-5)
        eng.close()


def _fit_images(cases, n):
    return [cases["fit_%d_%dx%d_image_u8" % (c, h, w)] for c, h, w in cases["cases"] if c == n], [(int(h), int(w)) for c, h, w in cases["cases"] if c == n]


@pytest.fixture(scope="module")
def cases():
    return golden("planes_fit_cases.npz")


@pytest.fixture(scope="module")
def rgb_engine(hiplib):
    """the three-channel network of the same size: its fits are the existing kernels"""
    cfg = _staging_cfg(3).replace("yolo_input=planes\n", "")
    eng = hiplib.Engine(cfg, max_batch=9, dtype=hiplib.FP32, semantics=hiplib.SEM_DARKNET)
    eng.set_weights(IO.synth_weights(IO.parse_cfg(cfg), seed=3))
    yield eng
    eng.close()


@pytest.mark.parametrize("fit_name", ["FIT_STRETCH", "FIT_LETTERBOX", "FIT_CENTER_CROP"])
@pytest.mark.parametrize("n", PLANES)
def test_fits_equal_the_three_channel_fit_plane_by_plane(hiplib, cases, rgb_engine, n, fit_name):
    """two images per plane count (odd sizes, one wider and one taller than the 16 x 16 network) and a third, tiny one: plane c of the N-plane fit equals,
    bit for bit, plane 0 of the three-channel fit of the grey image made of that plane; the padding channels are zero (the letterbox's 0.5 fill too belongs
    to the real channels); a ragged batch of the three equals each image alone; LETTERBOX and CENTER_CROP equal the reference's own functions within 2e-6"""
    fit = getattr(hiplib, fit_name)
    imgs, sizes = _fit_images(cases, n)
    assert len(imgs) == 2 and sizes[0][1] > sizes[0][0] and sizes[1][0] > sizes[1][1] and all(h % 2 and w % 2 for h, w in sizes)
    imgs = imgs + [np.random.default_rng(n).integers(0, 256, (3, 5, n), dtype=np.uint8)]
    eng = _staging_engine(hiplib, n, hiplib.FP32)
    eng.forward_images(imgs, fit=fit, want_detections=False)
    batch = eng.staged_input(3)
    assert batch.shape == (3, 16, 16, (n + 7) // 8 * 8) and not batch[..., n:].any()
    for k, im in enumerate(imgs):
        eng.forward_images([im], fit=fit, want_detections=False)
        assert np.array_equal(eng.staged_input(1)[0], batch[k]), k
        rgb_engine.forward_images([np.repeat(im[:, :, c:c + 1], 3, axis=2) for c in range(n)], fit=fit, want_detections=False)
        grey = rgb_engine.staged_input(n)
        assert not grey[..., 3:].any()
        for c in range(n):
            assert np.array_equal(batch[k, :, :, c], grey[c, :, :, 0]), (k, c)
        if k < 2 and fit != hiplib.FIT_STRETCH:
            tag = "fit_%d_%dx%d_%s" % (n, sizes[k][0], sizes[k][1], "letterbox" if fit == hiplib.FIT_LETTERBOX else "center_crop")
            np.testing.assert_allclose(batch[k, :, :, :n], cases[tag], rtol=0, atol=2e-6)
    if fit == hiplib.FIT_LETTERBOX:
        assert (batch[0, 0, :, :n] == 0.5).all()          # the wide image leaves rows of fill
    eng.close()


@pytest.mark.parametrize("n", PLANES)
def test_single_image_entry_points(hiplib, cases, n):
    """yolo_forward_image_u8 stages the stretch of a one-image batch, yolo_forward_letterbox_chw the letterbox fit's arithmetic on the planar float image"""
    imgs, _ = _fit_images(cases, n)
    for dtype in (hiplib.FP32, hiplib.BF16):
        eng = _staging_engine(hiplib, n, dtype, batch=1)
        for im in imgs:
            eng.forward_images([im], fit=hiplib.FIT_STRETCH, want_detections=False)
            want = eng.staged_input(1)
            rc = eng.lib.yolo_forward_image_u8(eng.ctx, im.ctypes.data, im.shape[0], im.shape[1], hiplib.HOST, None, hiplib.HOST)
            assert rc == 0 and np.array_equal(eng.staged_input(1), want)
            eng.forward_images([im], fit=hiplib.FIT_LETTERBOX, want_detections=False)
            want = eng.staged_input(1)
            chw = np.ascontiguousarray((im.astype(np.float64) / 255.).astype(np.float32).transpose(2, 0, 1))
            rc = eng.lib.yolo_forward_letterbox_chw(eng.ctx, chw.ctypes.data, im.shape[1], im.shape[0], hiplib.HOST, None, hiplib.HOST)
            assert rc == 0 and np.array_equal(eng.staged_input(1), want)
        eng.close()


# ---- 3: refusals ----
def test_refusals(hiplib):
    g = golden("mini_planes_grey.npz")
    eng = _fixture_engine(hiplib, g, hiplib.BF16)
    im = g["image_u8"]
    want = eng.detect_images([im], fit=hiplib.FIT_STRETCH, score_thr=0.3)
    for fit in (hiplib.FIT_CV2, hiplib.FIT_CV2_BGR):
        with pytest.raises(hiplib.YoloError, match=r"\(-6\).*YOLO_FIT_CV2.* 1 planes"):
            eng.detect_images([im], fit=fit)
        with pytest.raises(hiplib.YoloError, match=r"\(-6\).*YOLO_FIT_CV2.* 1 planes"):
            eng.forward_images([im], fit=fit)
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*yolo_detect_tiled_u8.* 1 planes"):
        eng.detect_tiled([im], tile=16, overlap=4)
    with pytest.raises(ValueError, match="3 channels.*reads 1"):
        eng.detect_images([np.zeros((8, 8, 3), np.uint8)])
    with pytest.raises(ValueError, match="3 channels.*reads 1"):
        eng.forward(np.zeros((1, 32, 32, 3), np.uint8))
    with pytest.raises(ValueError, match="reads 1"):
        eng.forward_image(np.zeros((8, 8, 3), np.uint8))
    # a 2-D array is one plane; the refused calls left the context as it was
    again = eng.detect_images([im[:, :, 0]], fit=hiplib.FIT_STRETCH, score_thr=0.3)
    assert len(again[0]) == len(want[0]) > 0 and np.array_equal(again[0].view(np.uint8), want[0].view(np.uint8))
    eng.close()


# ---- 4: the public surface ----
def test_veneer_loads_the_unmodified_cfg(hiplib, tmp_path, monkeypatch):
    """libdarknet_hip's load_network adds the key itself: darknet's own cfg text of mini_planes_grey, network_predict over 1 x 32 x 32 planar floats, the
    [yolo] layer's output within the fp32 bound of the fixture; network_predict_image refuses an image of another channel count"""
    from yolo_tensorflow_amd import darknet_hip as DH
    monkeypatch.setenv("DARKNET_HIP_DTYPE", "fp32")
    g = golden("mini_planes_grey.npz")
    assert "yolo_input" not in str(g["cfg"])
    cfg = str(tmp_path / "net.cfg"); wf = str(tmp_path / "net.weights")
    open(cfg, "w").write(str(g["cfg"])); IO.write_weights_file(wf, g["weights"], 0, 2)
    x = np.ascontiguousarray((g["image_u8"].astype(np.float32) / np.float32(255)).transpose(2, 0, 1))
    net = DH.load_net(cfg, wf)
    assert net
    try:
        lib = DH._load()
        out = np.ctypeslib.as_array(lib.network_predict(net, x.ctypes.data_as(C.POINTER(C.c_float))), shape=(21, 16, 16)).copy()
        rgb = lib.make_image(8, 8, 3)
        assert not lib.network_predict_image(net, rgb)
        lib.free_image(rgb)
    finally:
        DH.free_net(net)
    assert _relmax(out.transpose(1, 2, 0), g["layer_03"][0]) < MARGIN_TOL


def test_export_round_trip(hiplib, tmp_path):
    g = golden("mini_planes_rgbd.npz")
    x = np.repeat(g["image_u8"][None], 3, axis=0)
    eng = _fixture_engine(hiplib, g, hiplib.BF16)
    p = eng.classify(x, top_k=0)
    path = str(tmp_path / "rgbd.yolo")
    eng.export(path)
    eng.close()
    e2 = hiplib.Engine.from_file(path, max_batch=3)
    assert e2.input_channels == 4 and e2.input_hw == (22, 30)
    assert np.array_equal(e2.classify(x, top_k=0), p)
    e2.close()


def test_graph_form(hiplib):
    """detect_images_graph on mini_planes_grey: one buffer, one captured step, two sets of image sizes -- each call equals detect_images"""
    import torch
    g = golden("mini_planes_grey.npz")
    rng = np.random.default_rng(5)
    sets = [[g["image_u8"], rng.integers(0, 256, (17, 29, 1), dtype=np.uint8)], [rng.integers(0, 256, (31, 9, 1), dtype=np.uint8), g["image_u8"][:, ::-1]]]
    post = dict(score_thr=0.3, iou_thr=0.45, max_out=30)
    ref = _fixture_engine(hiplib, g, hiplib.BF16, batch=2)
    want = [ref.detect_images(s, fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, **post) for s in sets]
    ref.close()
    assert all(sum(len(r) for r in w) > 0 for w in want)
    eng = _fixture_engine(hiplib, g, hiplib.BF16, batch=2)
    cap = 4096
    dpix = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    boxes = torch.zeros(2 * 30 * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    for k in (0, 0, 1, 0, 1):
        pix, descs = hiplib.pack_images(sets[k], channels=1)
        assert pix.size <= cap
        dpix[:pix.size] = torch.from_numpy(pix).cuda()
        eng.detect_images_graph(dpix, descs, boxes, counts, fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, nbytes=cap, **post)
        eng.synchronize()
        bx = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(2, 30); ct = counts.cpu().numpy()
        for b in range(2):
            assert ct[b] == len(want[k][b]) and np.array_equal(bx[b, :ct[b]].view(np.uint8), want[k][b].view(np.uint8)), (k, b)
    eng.close()


def test_classifier_and_segmenter_take_darknet_cfgs(hiplib):
    """the classes add the key themselves: darknet's own cfg text of the 4-plane classifier and of the 9-plane map network, ragged batches of [h, w, C] images"""
    from yolo_tensorflow_amd.classifier import Classifier
    from yolo_tensorflow_amd.segmenter import Segmenter
    rng = np.random.default_rng(8)
    g = golden("mini_planes_rgbd.npz")
    clf = Classifier(str(g["cfg"]), max_batch=2, dtype=hiplib.FP32)
    clf.engine.set_weights(g["weights"])
    imgs = [g["image_u8"], rng.integers(0, 256, (13, 31, 4), dtype=np.uint8)]
    both = clf.classify_from_images(imgs, top=3)
    want = g["layer_04"].reshape(-1)
    assert [k for k, _ in both[0]] == list(np.argsort(-want, kind="stable")[:3])          # (the image at network size: the stretch is the identity)
    assert np.allclose([p for _, p in both[0]], np.sort(want)[::-1][:3], rtol=0, atol=MARGIN_TOL * want.max())
    assert clf.classify_from_images(imgs[1:], top=3)[0] == both[1]
    with pytest.raises(ValueError, match="3 channels, the network reads 4"):
        clf.classify_from_image(np.zeros((9, 9, 3), np.uint8))
    clf.close()
    g = golden("mini_planes_nine.npz")
    seg = Segmenter(str(g["cfg"]), weights=g["weights"], max_batch=2, dtype=hiplib.FP32, fit="letterbox")
    imgs = [g["image_u8"], rng.integers(0, 256, (21, 12, 9), dtype=np.uint8)]
    labels = seg.segment_from_images(imgs, thresh=-1e30)
    assert [l.shape for l in labels] == [(15, 22), (21, 12)] and all(l.dtype == np.uint8 and l.max() < 5 for l in labels)
    assert np.array_equal(seg.segment_from_images(imgs[1:], thresh=-1e30)[0], labels[1])
    m = seg.predict_from_images(imgs[:1])[0]
    assert _relmax(m, g["layer_03"][0]) < MARGIN_TOL          # (15 x 22 into 15 x 22: the letterbox copies the image)
    seg.close()
