"""Decoded video frames on the device: the yolo_*_frames_* entry points against the yolo_*_images_* ones over the RGB
images a numpy restatement of the colour rule yields (tests/test_frames_host.py ref_rgb) -- bit for bit everywhere: the operator, the
staged network input of every fit, the records in every storage type, the captured graph, tiling with windows on odd coordinates,
frame averaging and recurrent state, and every refusal before any launch."""
import ctypes as C
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_frames_host as FH

pytestmark = pytest.mark.gpu

NV12, I420, RGB24, BGR24 = FH.NV12, FH.I420, FH.RGB24, FH.BGR24
M601, M709, MFULL = FH.MATRICES
S = 160
POST = dict(score_thr=0.3, iou_thr=0.45, max_out=30)


def _recs_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _engine(hip, size=S, cfg="yolov3", dtype=None, max_batch=7, seed=2):
    txt = IO.with_input_size(IO.cfg_text(cfg), size)
    e = hip.Engine(txt, max_batch=max_batch, dtype=hip.BF16 if dtype is None else dtype)
    e.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=seed, obj_bias=-0.75))
    return e


def _mixed(rng, sizes, rot=0):
    """frames of `sizes`, formats and matrices in rotation: NV12 / BT601, I420 / BT709, NV12 / BT601_FULL, BGR24, RGB24; all at non-trivial pitches"""
    kinds = [(NV12, M601), (I420, M709), (NV12, MFULL), (BGR24, M601), (RGB24, M601)]
    out = []
    for i, (h, w) in enumerate(sizes):
        fmt, m = kinds[(i + rot) % len(kinds)]
        out.append(FH.make_frame(rng, h, w, fmt, m, y_extra=1 if fmt in (RGB24, BGR24) else 3))
    return out


# ---- 1: the operator ----
def test_operator_equals_the_restatement(hiplib):
    rng = np.random.default_rng(31)
    for f in FH.layout_frames(rng):
        got = hiplib.frame_to_rgb(f, device=0)
        assert np.array_equal(got, FH.ref_of(f)), (f.h, f.w, f.format, f.matrix)
        assert np.array_equal(got, hiplib.frame_to_rgb(f))
    for k, (m, fmt) in enumerate([(M601, NV12), (M709, I420), (MFULL, NV12)]):          # every chroma pair, four luma values each, per matrix
        planes = FH.exhaustive_planes(17 * k + 5, fmt)
        f = hiplib.Frame(np.concatenate([p.reshape(-1) for p in planes]), 512, 512, fmt, matrix=m)
        assert np.array_equal(hiplib.frame_to_rgb(f, device=0), FH.ref_of(f)), m


# ---- 2: the fit ----
FIT_SIZES = [(1, 1), (2, 3), (97, 131), (64, 96), (200, 120), (3, 300)]


def _staging_engine(hip, extra=""):
    cfg = ("[net]\nheight=64\nwidth=96\nchannels=3\n%s\n" % extra +
           "[convolutional]\nfilters=4\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[avgpool]\n\n[softmax]\n")
    e = hip.Engine(cfg, max_batch=6, dtype=hip.BF16, semantics=hip.SEM_DARKNET)
    e.set_weights(IO.synth_weights(IO.parse_cfg(cfg), seed=3))
    return e


@pytest.mark.parametrize("fit", ["FIT_STRETCH", "FIT_LETTERBOX", "FIT_CV2", "FIT_CENTER_CROP"])
def test_fit_of_frames_equals_fit_of_the_restated_rgb(hiplib, fit):
    """forward_frames then staged_input == forward_images over the restated RGB then staged_input, on a 64 x 96 network, one batch mixing the
    five format / matrix kinds.  The letterbox of the 3 x 300 frame is less than one pixel high: both forms refuse it (-1), the other five are compared."""
    fit_id = getattr(hiplib, fit)
    rng = np.random.default_rng(32)
    for extra in ("", "yolo_input_mul=2\nyolo_input_add=-1\n"):
        e = _staging_engine(hiplib, extra)
        for rot in (0, 2):
            frames = _mixed(rng, FIT_SIZES, rot)
            rgbs = [FH.ref_of(f) for f in frames]
            if fit == "FIT_LETTERBOX":
                for call, arg in ((e.forward_frames, frames), (e.forward_images, rgbs)):
                    with pytest.raises(hiplib.YoloError, match=r"\(-1\).* 5: 3 x 300 letterboxes"):
                        call(arg, fit=fit_id, want_detections=False)
                frames, rgbs = frames[:5], rgbs[:5]
            n = len(frames)
            e.forward_images(rgbs, fit=fit_id, want_detections=False)
            want = e.staged_input(n)
            e.forward(np.zeros((n, 64, 96, 3), np.uint8), want_detections=False)          # (so that nothing of `want` is left staged)
            e.forward_frames(frames, fit=fit_id, want_detections=False)
            got = e.staged_input(n)
            assert want.shape == (n, 64, 96, 8) and want[..., :3].any()
            for i in range(n):
                assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32)), (fit, rot, i, FIT_SIZES[i])
        e.close()


# ---- 3: records ----
REC_SIZES = [(97, 131), (S, S), (200, 120), (33, 301), (241, 180), (64, 96), (5, 7)]


@pytest.mark.parametrize("dtype", ["BF16", "FP32", "FP16", "FP8", "FP16X2"])
def test_records_equal_detect_images_on_the_restated_rgb(hiplib, dtype):
    e = _engine(hiplib, dtype=getattr(hiplib, dtype))
    rng = np.random.default_rng(33)
    kept = 0
    for n in (1, 7):
        frames = _mixed(rng, REC_SIZES[:n], rot=n)
        rgbs = [FH.ref_of(f) for f in frames]
        for kw in (dict(fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, nms_mode=hiplib.NMS_TF),
                   dict(fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, nms_mode=hiplib.NMS_DARKNET)):
            want = e.detect_images(rgbs, **kw, **POST)
            got = e.detect_frames(frames, **kw, **POST)
            assert len(got) == n
            for i in range(n):
                assert _recs_equal(got[i], want[i]), (dtype, n, kw["fit"], i)
                kept += len(want[i])
    assert kept > 0
    e.close()


def test_detector_frames_equal_detector_images(hiplib):
    from yolo_tensorflow_amd.detector import YOLOV3
    secs = IO.parse_cfg(IO.cfg_text("yolov3"))
    d = YOLOV3(None, weights=IO.synth_weights(secs, seed=7), max_batch=3)
    d.threshold = 0.3
    rng = np.random.default_rng(34)
    frames = _mixed(rng, [(240, 320), (33, 500), (416, 416), (5, 5)], rot=1)
    rgbs = [FH.ref_of(f) for f in frames]
    kept = 0
    for got, want in ((d.detect_from_frames(frames), d.detect_from_images(rgbs)),
                      (d.detect_from_large_frames(frames[:2], tile=224), d.detect_from_large_images(rgbs[:2], tile=224))):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            kept += len(w[0])
    assert kept > 0
    d.engine.close()


# ---- 4: graph ----
def test_graph_replays_with_new_sizes_and_formats_beside_the_image_graph(hiplib):
    """eager, capture, three replays with other sizes, formats, pitches and offsets: each call equals the eager detect_frames.  detect_images_graph is called
    between them with its own buffers: each entry point keeps a captured step of its own (yolo_ctx::graph[1] / graph[2]), and both keep answering as the
    eager calls do -- what the existing graph tests read are the records."""
    import torch
    e = _engine(hiplib, max_batch=5)
    n, mo = 5, 30
    rng = np.random.default_rng(35)
    sets = [_mixed(rng, [(100, 200), (S, S), (333, 41), (7, 9), (240, 180)], 0), _mixed(rng, [(50, 60), (300, 310), (161, 159), (1, 1), (90, 400)], 3),
            _mixed(rng, [(97, 131), (2, 3), (64, 96), (200, 120), (3, 300)], 1)]
    packed = [hiplib.pack_frames(s) for s in sets]
    imgs = [[FH.ref_of(f) for f in s] for s in sets[:2]]
    ipacked = [hiplib.pack_images(s) for s in imgs]
    dev = torch.zeros(max(p.size for p, _ in packed) + 64, dtype=torch.uint8, device="cuda")
    idev = torch.zeros(max(p.size for p, _ in ipacked), dtype=torch.uint8, device="cuda")
    boxes = torch.zeros(n * mo * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    iboxes = torch.zeros(n * mo * 6, dtype=torch.int32, device="cuda"); icounts = torch.zeros(n, dtype=torch.int32, device="cuda")
    kw = {k: v for k, v in POST.items() if k != "max_out"}

    def read(bx, ct):
        e.synchronize()
        b = bx.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(n, mo); c = ct.cpu().numpy()
        return [b[i, :c[i]].copy() for i in range(n)]

    def run_frames(k, shift):
        pix, descs = packed[k]
        descs = descs.copy(); descs["offset"] += shift
        dev.fill_(0xFF); dev[shift:shift + pix.size].copy_(torch.from_numpy(pix)); torch.cuda.synchronize()
        e.detect_frames_graph(dev, descs, boxes, counts, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, max_out=mo, **kw)
        return read(boxes, counts)

    def run_images(k):
        pix, descs = ipacked[k]
        idev.zero_(); idev[:pix.size].copy_(torch.from_numpy(pix)); torch.cuda.synchronize()
        e.detect_images_graph(idev, descs, iboxes, icounts, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, max_out=mo, **kw)
        return read(iboxes, icounts)

    want = [e.detect_frames(s, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, **POST) for s in sets]
    iwant = [e.detect_images(s, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, **POST) for s in imgs]
    assert all(sum(len(r) for r in w) > 0 for w in want)
    for step, (k, shift) in enumerate([(0, 0), (0, 0), (1, 64), (2, 0), (0, 33)]):          # call 1 eager, call 2 captures, then three replays
        got = run_frames(k, shift)
        for i in range(n):
            assert _recs_equal(got[i], want[k][i]), "frames call %d frame %d" % (step + 1, i)
        igot = run_images(step % 2)
        for i in range(n):
            assert _recs_equal(igot[i], iwant[step % 2][i]), "images call %d image %d" % (step + 1, i)
    e.close()


# ---- 5: tiling ----
@pytest.mark.parametrize("max_batch", [1, 5])
def test_tiled_frames_equal_tiled_images_with_windows_on_odd_coordinates(hiplib, max_batch):
    e = _engine(hiplib, max_batch=max_batch)
    rng = np.random.default_rng(36)
    frames = [FH.make_frame(rng, 301, 423, NV12, M601), FH.make_frame(rng, 160, 500, I420, M709)]
    wins = hiplib.tile_windows((301, 423), S, 32)
    assert (wins[-1, 0] & 1) and (wins[-1, 1] & 1) and len(wins) == 12          # the pulled-back last row and column: 141 and 263
    rgbs = [FH.ref_of(f) for f in frames]
    kept = 0
    for kw in (dict(fit=hiplib.FIT_STRETCH, nms_mode=hiplib.NMS_TF, relative=False), dict(fit=hiplib.FIT_LETTERBOX, nms_mode=hiplib.NMS_DARKNET, relative=True)):
        want = e.detect_tiled(rgbs, tile=S, overlap=32, **kw, **POST)
        got = e.detect_tiled_frames(frames, tile=S, overlap=32, **kw, **POST)
        for i in range(2):
            assert _recs_equal(got[i], want[i]), (max_batch, kw["fit"], i)
            kept += len(want[i])
    assert kept > 0
    e.close()


# ---- 6: state ----
def test_frame_average_over_frames_equals_frame_average_over_rgb(hiplib):
    a = _engine(hiplib, size=(64, 96), max_batch=2); b = _engine(hiplib, size=(64, 96), max_batch=2)
    a.set_frame_average(3); b.set_frame_average(3)
    rng = np.random.default_rng(37)
    kept = 0
    for t in range(4):
        frames = [FH.make_frame(rng, 97 + t, 131, NV12, M601), FH.make_frame(rng, 64, 96 + 2 * t, NV12, MFULL)]
        want = b.detect_images([FH.ref_of(f) for f in frames], fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, score_thr=0.1, iou_thr=0.45, max_out=30)
        got = a.detect_frames(frames, fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, score_thr=0.1, iou_thr=0.45, max_out=30)
        for i in range(2):
            assert _recs_equal(got[i], want[i]), (t, i)
            kept += len(want[i])
    assert kept > 0
    a.close(); b.close()


def test_recurrent_state_steps_over_frames(hiplib):
    g = golden("mini_crnn.npz")
    cfg, flat = str(g["cfg"]), g["weights"]
    engs = []
    for _ in range(2):
        e = hiplib.Engine(cfg, max_batch=2, dtype=hiplib.BF16, semantics=hiplib.SEM_DARKNET)
        e.set_weights(flat)
        engs.append(e)
    a, b = engs
    assert a.num_state_tensors > 0
    rng = np.random.default_rng(38)
    for t in range(3):
        frames = [FH.make_frame(rng, 40 + t, 52, NV12, M709), FH.make_frame(rng, 33, 31 + t, I420, M601)]
        want = b.forward_images([FH.ref_of(f) for f in frames], fit=hiplib.FIT_STRETCH)
        got = a.forward_frames(frames, fit=hiplib.FIT_STRETCH)
        assert want.any() and np.array_equal(got.view(np.uint32), want.view(np.uint32)), t
    for k in range(a.num_state_tensors):
        for s in range(2):
            assert np.array_equal(a.state(k, s), b.state(k, s)) and a.state(k, s).any()
    a.close(); b.close()


# ---- 7: refusals ----
def test_refusals_come_before_any_launch_and_name_the_frame(hiplib):
    import torch
    e = _engine(hiplib, cfg="yolov3-tiny", max_batch=4)
    rng = np.random.default_rng(39)
    frames = [FH.make_frame(rng, 50, 70, I420, M709), FH.make_frame(rng, 6, 9, NV12, reverse=False, gap=0), FH.make_frame(rng, 20, 30, BGR24, y_extra=1)]
    buf, descs = hiplib.pack_frames(frames)
    mo = 10
    dev = torch.from_numpy(buf).cuda()
    dboxes = torch.full((4 * mo * 6,), 7, dtype=torch.int32, device="cuda"); dcounts = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = e.detect_frames((buf, descs), fit=hiplib.FIT_STRETCH, score_thr=0.3, iou_thr=0.45, max_out=mo)
    staged = e.staged_input(3)

    def calls(d, n, nbytes, fit, tiled=True):
        """the four entry points over the same arguments -> [(return code, message)]; a refused call has written nothing"""
        d = np.ascontiguousarray(d)
        boxes = np.zeros((4, mo), dtype=hiplib.BOX_DTYPE); boxes["cls"] = 7; counts = np.full(4, 7, np.int32)
        out = []

        def note(rc, untouched):
            assert rc == 0 or untouched()
            out.append((rc, e.lib.yolo_last_error(e.ctx).decode() if rc else ""))
        host_untouched = lambda: (counts == 7).all() and (boxes["cls"] == 7).all()
        note(e.lib.yolo_detect_frames_u8(e.ctx, buf.ctypes.data, nbytes, d.ctypes.data, n, fit, hiplib.HOST, 0.3, 0.45, mo, hiplib.NMS_TF, hiplib.SELECT_GT,
                                         hiplib.UNITS_NETWORK, boxes.ctypes.data, counts.ctypes.data, hiplib.HOST), host_untouched)
        note(e.lib.yolo_forward_frames_u8(e.ctx, buf.ctypes.data, nbytes, d.ctypes.data, n, fit, hiplib.HOST, None, hiplib.HOST), lambda: True)
        rc = e.lib.yolo_detect_frames_graph(e.ctx, C.c_void_p(dev.data_ptr()), nbytes, d.ctypes.data, n, fit, 0.3, 0.45, mo, hiplib.NMS_TF, hiplib.SELECT_GT,
                                            hiplib.UNITS_NETWORK, C.c_void_p(dboxes.data_ptr()), C.c_void_p(dcounts.data_ptr()))
        e.synchronize()
        note(rc, lambda: (dcounts.cpu().numpy() == 7).all())
        if tiled:
            boxes["cls"] = 7; counts[:] = 7
            note(e.lib.yolo_detect_tiled_frames_u8(e.ctx, buf.ctypes.data, nbytes, d.ctypes.data, n, 0, 0, 16, 16, fit, hiplib.HOST, 0.3, 0.45, mo, hiplib.NMS_TF,
                                                   hiplib.SELECT_GT, 0, boxes.ctypes.data, counts.ctypes.data, hiplib.HOST), host_untouched)
        return out

    def codes(*a, **kw):
        return [rc for rc, _ in calls(*a, **kw)]

    def refused(d, n, nbytes, fit, code, *words, tiled=True):
        """every entry point returns `code` with a message that holds `words`"""
        for rc, msg in calls(d, n, nbytes, fit, tiled):
            assert rc == code and all(w in msg for w in words), (rc, msg, words)

    # every descriptor the host function refuses, as frame 1 of the batch (the short-buffer cases apart: here other frames lie behind frame 1)
    checked = 0
    for bad, nbytes, what in FH.bad_descs(buf, descs[1:2].copy()):
        if what == "past":
            continue
        d = descs.copy(); d[1] = bad[0]
        refused(d, 3, buf.size, hiplib.FIT_STRETCH, -1, "frame 1", what)
        checked += 1
    assert checked == 12
    # frame 1's chroma plane ends one byte past the buffer
    refused(descs[:2], 2, int(descs["offset"][1, 1]) + 2 * int(descs["pitch"][1, 1]) + 9, hiplib.FIT_STRETCH, -1, "frame 1", "past")
    # what images_check refuses: the batch size (tiling is not bound by max_batch), the buffer's size, an unknown fit, a letterbox of less than one pixel
    refused(descs, 0, buf.size, hiplib.FIT_STRETCH, -1)
    refused(np.concatenate([descs, descs[:2]]), 5, buf.size, hiplib.FIT_STRETCH, -1, tiled=False)
    refused(descs, 3, 0, hiplib.FIT_STRETCH, -1)
    refused(descs, 3, buf.size, 9, -1)
    thin = [FH.make_frame(rng, 1, 2000, NV12)]
    with pytest.raises(hiplib.YoloError, match=r"\(-1\).*frame 0: 1 x 2000 letterboxes"):
        e.forward_frames(thin, fit=hiplib.FIT_LETTERBOX)
    # YOLO_ERR_UNSUPPORTED: the frame's format states its channel order
    refused(descs, 3, buf.size, hiplib.FIT_CV2_BGR, -6, "YOLO_FIT_CV2_BGR")
    # no refused call launched anything: the staged input is still the last good call's
    assert np.array_equal(e.staged_input(3), staged)
    # ... and what the image form of the same entry point refuses (a plain forward takes the centre crop, as yolo_forward_images_u8 does)
    assert codes(descs, 3, buf.size, hiplib.FIT_CENTER_CROP) == [-6, 0, -6, -6]
    assert codes(descs, 3, buf.size, hiplib.FIT_CV2) == [0, 0, 0, -6]
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*YOLO_NMS_PER_CLASS"):
        e.detect_tiled_frames(frames, nms_mode=hiplib.NMS_PER_CLASS)
    again = e.detect_frames((buf, descs), fit=hiplib.FIT_STRETCH, score_thr=0.3, iou_thr=0.45, max_out=mo)
    assert sum(len(x) for x in good) > 0 and all(_recs_equal(x, y) for x, y in zip(good, again))
    e.close()
    # a planes network
    g = golden("mini_planes_grey.npz")
    p = hiplib.Engine(IO.with_planes_input(str(g["cfg"])), max_batch=2, semantics=hiplib.SEM_DARKNET)
    p.set_weights(g["weights"])
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*frames.* 1 planes"):
        p.forward_frames(frames[:2])
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*frames.* 1 planes"):
        p.detect_frames(frames[:2])
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*yolo_detect_tiled_frames_u8.* 1 planes"):
        p.detect_tiled_frames(frames[:2])
    p.close()
