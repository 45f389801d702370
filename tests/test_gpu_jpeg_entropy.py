"""The entropy stage on the device: k_jpeg_entropy decodes restart intervals, one lane each.  Everything here is a comparison with the host
stage, bit for bit: the operator's coefficients, the planes and the frame table of a mixed batch across lane and workgroup boundaries, the results of every
*_jpegs entry point under both modes, the captured graph, the detector class, and the verdicts -- code and message -- on malformed streams.  The malformed
streams are input-validation cases: tests/c/jpeg_intervals.cpp has run the same decoder over such inputs under the sanitizers on the host."""
import hashlib
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_jpeg_host as JH
import test_gpu_jpeg as GJ
import test_jpeg_intervals_host as IH

pytestmark = pytest.mark.gpu

PHOTOS = ["dog", "eagle", "giraffe", "horses", "kite", "person"]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _same(a, b):
    """two results of one entry point, bit for bit: arrays, or lists / tuples / dicts of results"""
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _both(e, call):
    """call() under the host stage, then under the device stage"""
    e.set_jpeg_entropy("host")
    want = call()
    assert e.jpeg_entropy_times()["device_files"] == 0
    e.set_jpeg_entropy("auto")
    got = call()
    return want, got


def _cls19(hip, dtype, max_batch=12):
    g = golden("mini_cls19.npz")
    e = hip.Engine(str(g["cfg"]), max_batch=max_batch, dtype=dtype, semantics=hip.SEM_DARKNET)
    e.set_weights(g["weights"])
    return e


def _unet(hip, dtype, max_batch=12):
    g = golden("mini_unet.npz")
    e = hip.Engine(str(g["cfg"]), max_batch=max_batch, dtype=dtype, semantics=hip.SEM_DARKNET)
    e.set_weights(g["weights"])
    return e, float(np.median(g["layer_11"].max(axis=-1)))


# ---- 1: the operator ----
def test_operator_equals_the_host_stage_on_every_dri_fixture(hiplib):
    names = IH.dri_fixtures()
    assert len(names) == 36 and {"c1x1_444_rst1", "c1x1_420_rst1", "c16x16_420_rst1", "c17x9_422_rst1", "c7x5_440_rst1", "c50x35_444_rst3"} <= set(names)
    for name in names:
        want, got = hiplib.jpeg_coefficients(JH.path_of(name)), hiplib.jpeg_coefficients_device(JH.path_of(name))
        assert _same(want, got), name
        assert any(p.any() for p in want)


@pytest.mark.parametrize("photo", ["dog", "kite"])
def test_operator_equals_the_host_stage_on_a_photograph(hiplib, photo):
    data = _read(GJ._photo(photo))
    assert len(hiplib.jpeg_intervals(data)) == IH.PHOTOS[photo][1]
    digest = [hashlib.sha256(np.concatenate([p.ravel() for p in coef]).tobytes()).hexdigest() for coef in (hiplib.jpeg_coefficients(data), hiplib.jpeg_coefficients_device(data))]
    assert digest[0] == digest[1]


def test_operator_refuses_a_file_without_a_restart_interval(hiplib):
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*no restart interval"):
        hiplib.jpeg_coefficients_device(JH.path_of("c17x9_420_std"))
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*progressive"):
        hiplib.jpeg_coefficients_device(JH.path_of("refused_progressive"))


# ---- 2: lane and workgroup boundaries ----
def test_mixed_batch_across_workgroup_boundaries_equals_the_host_stage(hiplib):
    """8 x c50x35_444_rst1 is 8 x 35 = 280 intervals: every file fills part of one workgroup of 64 lanes, the rest of its lanes idle; between them lie files the
    host stage decodes (no DRI) and one eligible file of each other format, a three-MCU interval among them"""
    big = "c50x35_444_rst1"
    names = [big, "g23x19", big, "c17x9_420_rst1", big, "c33x31_444_opt", big, big, "c50x35_422_rst3", "c1x1_420_std", big, "c7x5_440_rst1", big, "c50x35_420_q10", big, "g1x1",
             "c16x16_420_rst1", "c50x35_440_rst3", "c1x1_444_rst1"]
    files = [JH.path_of(n) for n in names]
    eligible = [n for n in names if JH.name_geometry(n)[3]]
    intervals = sum(len(hiplib.jpeg_intervals(JH.path_of(n))) for n in eligible)
    assert names.count(big) == 8 and intervals >= 280
    e = GJ._mini(hiplib, hiplib.BF16, max_batch=len(names))
    assert e.jpeg_entropy == "host"
    want = e.decode_jpegs(files)
    want_descs, want_surface = want.descs.copy(), GJ._surface(e, want)
    assert e.jpeg_entropy_times() == {"device_files": 0, "host_files": len(names), "intervals": 0, "scan_ms": 0.0, "device_ms": 0.0, "stream_bytes": 0}
    e.set_jpeg_entropy("auto")
    got = e.decode_jpegs(files)
    t = e.jpeg_entropy_times()
    assert (t["device_files"], t["host_files"], t["intervals"]) == (len(eligible), len(names) - len(eligible), intervals) and t["device_ms"] > 0 and t["stream_bytes"] > 0
    assert (got.pixels, got.nbytes) == (want.pixels, want.nbytes)
    assert np.array_equal(got.descs.view(np.uint8), want_descs.view(np.uint8)) and np.array_equal(GJ._surface(e, got), want_surface)
    # a second, smaller batch into the same surface: one eligible file, one that is not
    again = e.decode_jpegs(files[2:4])
    assert (again.pixels, again.nbytes) == (want.pixels, want.nbytes) and len(again) == 2
    t = e.jpeg_entropy_times()
    assert (t["device_files"], t["host_files"], t["intervals"]) == (2, 0, 35 + len(hiplib.jpeg_intervals(files[3])))
    surface = GJ._surface(e, again)
    e.set_jpeg_entropy("host")
    host = e.decode_jpegs(files[2:4])
    assert np.array_equal(again.descs.view(np.uint8), host.descs.view(np.uint8)) and np.array_equal(surface, GJ._surface(e, host))
    e.close()


# ---- 3: end to end ----
MIXED = GJ.MIXED + ["c50x35_444_rst1"]


@pytest.mark.parametrize("dtype", ["BF16", "FP32"])
def test_detect_jpegs_is_the_same_under_both_modes(hiplib, dtype):
    e = GJ._mini(hiplib, getattr(hiplib, dtype), max_batch=len(MIXED) + 2)
    files = [JH.path_of(n) for n in MIXED] + [GJ._photo("dog"), GJ._photo("giraffe")]
    kept = 0
    for kw in (dict(fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, nms_mode=hiplib.NMS_TF), dict(fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_NETWORK, nms_mode=hiplib.NMS_DARKNET)):
        want, got = _both(e, lambda: e.detect_jpegs(files, score_thr=0.05, iou_thr=0.45, max_out=30, **kw))
        t = e.jpeg_entropy_times()
        assert t["device_files"] == sum(1 for n in MIXED if JH.name_geometry(n)[3]) + 1 and t["host_files"] == len(files) - t["device_files"]
        assert _same(want, got), (dtype, kw["fit"])
        kept += sum(len(r) for r in want)
    assert kept > 0 or dtype != "BF16"
    e.close()


@pytest.mark.parametrize("dtype", ["BF16", "FP32"])
def test_classify_jpegs_and_views_are_the_same_under_both_modes(hiplib, dtype):
    e = _cls19(hiplib, getattr(hiplib, dtype), max_batch=len(MIXED))
    files = [JH.path_of(n) for n in MIXED]
    for fit in (hiplib.FIT_STRETCH, hiplib.FIT_CENTER_CROP):
        want, got = _both(e, lambda: e.classify_jpegs(files, fit=fit, top_k=3))
        assert e.jpeg_entropy_times()["device_files"] > 0 and _same(want, got), (dtype, fit)
    for views in (hiplib.VIEWS_FLIP, hiplib.VIEWS_TEN_CROP):
        want, got = _both(e, lambda: e.classify_views_jpegs(files[:6] + files[-1:], views, top_k=3))
        assert e.jpeg_entropy_times()["device_files"] > 0 and _same(want, got), (dtype, views)
    e.close()


@pytest.mark.parametrize("dtype", ["BF16", "FP32"])
def test_segment_jpegs_is_the_same_under_both_modes(hiplib, dtype):
    e, thresh = _unet(hiplib, getattr(hiplib, dtype), max_batch=len(MIXED))
    files = [JH.path_of(n) for n in MIXED]
    for fit in (hiplib.FIT_LETTERBOX, hiplib.FIT_STRETCH):
        want, got = _both(e, lambda: e.segment_jpegs(files, fit=fit, thresh=thresh))
        assert e.jpeg_entropy_times()["device_files"] > 0 and _same(want, got), (dtype, fit)
    e.close()


def test_graph_replays_over_two_batches_decoded_on_the_device(hiplib):
    """test_gpu_jpeg's graph test with the decodes under "auto": eager, capture, three replays; every call's records equal detect_jpegs of the host stage"""
    import torch
    e = GJ._engine(hiplib, max_batch=3)
    n, mo = 3, 30
    sets = [["dog", "c50x35_420_std", "kite"], ["person", "giraffe", "c33x31_422_rst1"]]
    files = [[GJ._file(k) for k in s] for s in sets]
    boxes = torch.zeros(n * mo * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    kw = dict(fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS)
    want = [e.detect_jpegs(f, **kw, **GJ.POST) for f in files]
    assert all(sum(len(r) for r in w) > 0 for w in want)
    e.set_jpeg_entropy("auto")
    surfaces = set()
    for step, k in enumerate([0, 0, 1, 0, 1]):
        handle = e.decode_jpegs(files[k])
        assert e.jpeg_entropy_times()["device_files"] == 2
        surfaces.add((handle.pixels, handle.nbytes))
        e.detect_frames_graph(handle.pixels, handle.descs, boxes, counts, nbytes=handle.nbytes, max_out=mo, score_thr=GJ.POST["score_thr"], iou_thr=GJ.POST["iou_thr"], **kw)
        e.synchronize()
        b = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(n, mo); c = counts.cpu().numpy()
        for i in range(n):
            assert GJ._recs_equal(b[i, :c[i]], want[k][i]), "call %d file %s" % (step + 1, sets[k][i])
    assert len(surfaces) == 1
    e.close()


def test_detector_files_with_the_device_stage_equal_the_default(hiplib):
    from yolo_tensorflow_amd.detector import YOLOV3
    w = IO.synth_weights(IO.parse_cfg(IO.cfg_text("yolov3")), seed=7)
    paths = [GJ._photo(p) for p in PHOTOS]
    out = []
    for kw in ({}, {"jpeg_entropy": "auto"}):
        d = YOLOV3(None, weights=w, max_batch=6, **kw)
        d.threshold = 0.3
        assert d.engine.jpeg_entropy == kw.get("jpeg_entropy", "host")
        out.append(d.detect_from_files(paths))
        t = d.engine.jpeg_entropy_times()
        assert (t["device_files"], t["host_files"]) == ((5, 1) if kw else (0, 6))          # giraffe has no restart interval
        d.engine.close()
    assert _same(out[0], out[1]) and sum(len(r[0]) for r in out[0]) > 0


# ---- 4: verdicts ----
def _mutations(hip):
    """(what, bytes): streams made of a fixture's bytes, each malformed -- or merely changed -- in one way"""
    data = _read(JH.path_of("c50x35_444_rst1"))
    iv = hip.jpeg_intervals(data)
    at = int(iv[10, 1])          # the marker behind interval 10
    mid = (int(iv[20, 0]) + int(iv[20, 1])) // 2
    assert int(iv[20, 1]) - int(iv[20, 0]) >= 8
    out = [("a marker deleted", data[:at] + data[at + 2:]),
           ("a junk byte before a marker", data[:at] + b"\x5a" + data[at:]),
           ("an interval cut short", data[:at - 3] + data[at:]),
           ("EOI mid-scan", data[:mid] + b"\xff\xd9" + data[mid:]),
           ("EOI in a marker's place", data[:at] + b"\xff\xd9" + data[at + 2:]),
           ("the file cut short", data[:int(iv[30, 0]) + 2])]
    # single flipped bytes inside interval 20, found on the host: the first the host stage refuses, the first it still serves with other coefficients
    want = hip.jpeg_coefficients(data)
    bad = good = None
    for k in range(int(iv[20, 0]), int(iv[20, 1])):
        for flip in (0x01, 0x10, 0x80, 0x7f):
            m = data[:k] + bytes([data[k] ^ flip]) + data[k + 1:]
            if m[k] == 0xFF or data[k] == 0xFF or (k and data[k - 1] == 0xFF):
                continue
            try:
                served = not _same(hip.jpeg_coefficients(m), want)
            except hip.YoloError:
                served = None
            if served is None and bad is None:
                bad = m
            if served and good is None:
                good = m
    assert bad is not None and good is not None
    return out + [("a flipped byte that yields a refusal", bad), ("a flipped byte that still decodes", good)]


def _verdict(call):
    try:
        return ("served", call())
    except Exception as err:          # YoloError: "<entry point> failed (code): message" -- the code and the library's message are the verdict
        return (type(err).__name__, str(err).split(" failed ", 1)[-1])


def test_verdicts_are_the_host_stage_s(hiplib):
    e = GJ._mini(hiplib, hiplib.BF16, max_batch=4)
    ok = _read(JH.path_of("c17x9_422_rst1"))
    served = refused = 0
    for what, m in _mutations(hiplib):
        # the operator: the coefficients, or the refusal, of the host stage
        a, b = _verdict(lambda: hiplib.jpeg_coefficients(m)), _verdict(lambda: hiplib.jpeg_coefficients_device(m))
        assert a[0] == b[0] and _same(a[1], b[1]), what
        # a batch with the stream in its middle: code and message, or the planes
        batch = [ok, m, ok]
        e.set_jpeg_entropy("host")
        want = _verdict(lambda: GJ._surface(e, e.decode_jpegs(batch)))
        e.set_jpeg_entropy("auto")
        got = _verdict(lambda: GJ._surface(e, e.decode_jpegs(batch)))
        assert want[0] == got[0] and _same(want[1], got[1]), (what, want, got)
        if want[0] == "served":
            served += 1
            # the two intact files are the device's; the stream is too, unless it was handed back, and then its intervals are not counted either
            t = e.jpeg_entropy_times()
            own = len(hiplib.jpeg_intervals(ok))
            assert (t["device_files"], t["host_files"]) in ((3, 0), (2, 1)), (what, t)
            assert t["intervals"] == 2 * own + (len(hiplib.jpeg_intervals(m)) if t["device_files"] == 3 else 0), (what, t)
        else:
            refused += 1
            assert "(-1)" in want[1] and "file 1" in want[1], (what, want[1])
    assert served >= 1 and refused >= 4
    # the engine answers as before
    e.set_jpeg_entropy("auto")
    assert len(e.decode_jpegs([ok, ok])) == 2 and e.jpeg_entropy_times()["device_files"] == 2
    e.close()


# ---- 5: bookkeeping ----
def test_mode_and_times_bookkeeping(hiplib):
    e = GJ._mini(hiplib, hiplib.BF16, max_batch=4)
    assert e.lib.yolo_jpeg_entropy(e.ctx) == 0 and e.jpeg_entropy == "host"
    with pytest.raises(hiplib.YoloError, match=r"\(-3\).*before any decode"):
        e.jpeg_entropy_times()
    files = [JH.path_of(n) for n in ("c17x9_420_rst1", "g23x19", "c50x35_422_rst3", "c8x8_444_std")]
    e.decode_jpegs(files)
    assert e.jpeg_entropy_times()["device_files"] == 0 and e.jpeg_entropy_times()["host_files"] == 4
    e.set_jpeg_entropy("auto")
    assert e.lib.yolo_jpeg_entropy(e.ctx) == 1 and e.jpeg_entropy == "auto"
    e.decode_jpegs(files)
    t = e.jpeg_entropy_times()
    assert (t["device_files"], t["host_files"]) == (2, 2) and t["intervals"] == sum(len(hiplib.jpeg_intervals(f)) for f in files) and t["scan_ms"] >= 0
    assert t["stream_bytes"] >= sum(len(_read(f)) for f in (files[0], files[2]))
    d = e.jpeg_decode_times()
    assert d["upload_bytes"] > t["stream_bytes"] and d["idct_ms"] > 0
    e.decode_jpegs(files[1::2])          # nothing eligible: the host path
    t = e.jpeg_entropy_times()
    assert (t["device_files"], t["host_files"], t["intervals"], t["stream_bytes"]) == (0, 2, 0, 0)
    for mode in (2, -1, 7):
        assert e.lib.yolo_set_jpeg_entropy(e.ctx, mode) == -1
        assert b"yolo_set_jpeg_entropy" in e.lib.yolo_last_error(e.ctx) and e.jpeg_entropy == "auto"
    with pytest.raises(hiplib.YoloError):
        e.set_jpeg_entropy("device")
    e.set_jpeg_entropy("host")
    assert e.jpeg_entropy == "host"
    e.close()
