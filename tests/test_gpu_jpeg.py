"""JPEG files on the device: host entropy stage, k_jpeg_idct, and the JPEG frame formats inside the fit launch, against what the
compiled reference decodes (tests/golden/jpeg_cases.npz; tests/test_jpeg_host.py holds the host twin to the same) -- bit for bit everywhere: the
operator, a mixed batch's frame table, the staged network input of every fit, the records in every storage type, the captured graph, tiling with
windows on odd coordinates, the detector class, the veneer's resize, and the refusals before any launch."""
import ctypes as C
import hashlib
import os
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import darknet_io as IO
import test_jpeg_host as JH

pytestmark = pytest.mark.gpu

POST = dict(score_thr=0.3, iou_thr=0.45, max_out=30)
# one batch that mixes the five formats, sizes below and above one MCU, every variant of the entropy stage
MIXED = ["c17x9_420_rst1", "g23x19", "c33x31_444_opt", "c50x35_422_rst3", "c1x1_420_std", "c7x5_440_rst1", "c50x35_420_q10", "c33x31_422_q100", "g1x1", "c2x2_422_opt",
         "c50x35_440_rst3", "c8x8_444_std"]


def _recs_equal(a, b):
    return len(a) == len(b) and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _photo(name):
    p = os.path.join(JH.IMAGES, name + ".jpg")
    assert os.path.exists(p), p
    return p


def _file(name):
    """a fixture of tests/golden/jpeg or a photograph of tests/golden/images, by name"""
    return _photo(name) if name in ("dog", "eagle", "giraffe", "horses", "kite", "person") else JH.path_of(name)


def _engine(hip, size=160, cfg="yolov3", dtype=None, max_batch=7, seed=2):
    txt = IO.with_input_size(IO.cfg_text(cfg), size)
    e = hip.Engine(txt, max_batch=max_batch, dtype=hip.BF16 if dtype is None else dtype)
    e.set_weights(IO.synth_weights(IO.parse_cfg(txt), seed=seed, obj_bias=-0.75))
    return e


def _mini(hip, dtype, max_batch=12):
    g = golden("mini_v3.npz")
    e = hip.Engine(str(g["cfg"]), max_batch=max_batch, dtype=dtype, semantics=hip.SEM_DARKNET)
    e.set_weights(g["weights"])
    return e


@pytest.fixture(scope="module")
def decoded():
    """the reference's decode of every file the tests use, computed once: the fixtures from jpeg_cases.npz, the photographs from the host twin,
    which is held to the reference's digest here"""
    g, names = JH.cases()
    out = {n: g["rgb/" + n] for n in names}
    from yolo_tensorflow_amd import hip
    for name, sha in zip(g["photos"], g["photo_sha256"]):
        rgb = hip.jpeg_to_rgb(_photo(str(name)))
        assert hashlib.sha256(rgb.tobytes()).hexdigest() == str(sha), name
        out[str(name)] = rgb
    return out


# ---- 1: the operator ----
def test_operator_equals_the_reference_on_every_fixture(hiplib, decoded):
    _, names = JH.cases()
    for name in names:
        got = hiplib.jpeg_to_rgb(JH.path_of(name), device=0)
        assert got.shape == decoded[name].shape and np.array_equal(got, decoded[name]), name
    g = golden("jpeg_cases.npz")
    for photo in ("dog", "giraffe"):          # sampled 1 x 2 and 1 x 1: tens of thousands of blocks, restart intervals of a row of MCUs
        got = hiplib.jpeg_to_rgb(_photo(photo), device=0)
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(g["photo_sha256"][list(g["photos"]).index(photo)]), photo


# ---- 2: one decode of a mixed batch ----
def _surface(e, handle):
    """the used part of the engine's surface, copied to the host"""
    used = 0
    for d in handle.descs:
        rows = e_rows(d)
        for p, (r, row) in enumerate(rows):
            used = max(used, int(d["offset"][p]) + (r - 1) * int(d["pitch"][p]) + row)
    assert 0 < used <= handle.nbytes
    e.synchronize()
    import torch

    class Surface(object):          # the engine's device memory, as torch reads foreign device buffers
        __cuda_array_interface__ = {"shape": (used,), "typestr": "|u1", "data": (handle.pixels, False), "version": 2}
    return torch.as_tensor(Surface(), device="cuda").cpu().numpy().copy()


def e_rows(d):
    from yolo_tensorflow_amd import hip
    return hip.frame_plane_rows(int(d["h"]), int(d["w"]), int(d["format"]))


def test_one_decode_of_a_mixed_batch_gives_a_frame_table(hiplib, decoded):
    e = _mini(hiplib, hiplib.BF16)
    files = [JH.path_of(n) for n in MIXED]
    handle = e.decode_jpegs(files)
    assert len(handle) == len(MIXED) and handle.descs.dtype == hiplib.FRAME_DTYPE and handle.pixels and handle.nbytes >= 1
    assert sorted(set(int(f) for f in handle.descs["format"])) == [16, 17, 18, 19, 20] and not handle.descs["matrix"].any()
    for name, d in zip(MIXED, handle.descs):
        info = hiplib.jpeg_info(JH.path_of(name))
        n = info["components"]
        assert (int(d["h"]), int(d["w"]), int(d["format"])) == (info["h"], info["w"], info["format"])
        assert [int(v) for v in d["pitch"][:n]] == [pw for _, pw in info["planes"]] and all(int(v) % 8 == 0 for v in d["offset"][:n])
    surface = _surface(e, handle)
    for i, name in enumerate(MIXED):
        # the planes on the device are the planes the restated IDCT makes of the same coefficients
        planes = [JH.idct_plane(c) for c in hiplib.jpeg_coefficients(JH.path_of(name))]
        d = handle.descs[i]
        for p, want in enumerate(planes):
            got = np.lib.stride_tricks.as_strided(surface[int(d["offset"][p]):], shape=e_rows(d)[p], strides=(int(d["pitch"][p]), 1))
            assert np.array_equal(got, want[:got.shape[0], :got.shape[1]]), (name, p)
        # ... and the frame operator over the entry reads the fixture
        assert np.array_equal(hiplib.frame_to_rgb((surface, handle.descs[i:i + 1]), device=0), decoded[name]), name
        assert np.array_equal(hiplib.frame_to_rgb((surface, handle.descs[i:i + 1])), decoded[name]), name
    # a second, smaller batch lands in the same surface
    again = e.decode_jpegs(files[3:5])
    assert (again.pixels, again.nbytes) == (handle.pixels, handle.nbytes) and len(again) == 2
    e.close()


# ---- 3: the fit, the records ----
@pytest.mark.parametrize("dtype", ["BF16", "FP32"])
@pytest.mark.parametrize("fit", ["FIT_STRETCH", "FIT_LETTERBOX", "FIT_CV2", "FIT_CENTER_CROP"])
def test_staged_input_of_forward_jpegs_equals_forward_images_of_the_reference_bytes(hiplib, decoded, fit, dtype):
    e = _mini(hiplib, getattr(hiplib, dtype))
    fit_id = getattr(hiplib, fit)
    names = MIXED[:10] + ["dog", "kite"]
    files = [_file(k) for k in names]
    n = len(names)
    h, w = e.input_hw
    e.forward_images([decoded[k] for k in names], fit=fit_id, want_detections=False)
    want = e.staged_input(n)
    e.forward(np.zeros((n, h, w, 3), np.uint8), want_detections=False)          # (so that nothing of `want` is left staged)
    e.forward_jpegs(files, fit=fit_id, want_detections=False)
    got = e.staged_input(n)
    assert want.shape[:3] == (n, h, w) and want[..., :3].any()
    for i in range(n):
        assert np.array_equal(got[i].view(np.uint8), want[i].view(np.uint8)), (fit, dtype, names[i])
    e.close()


@pytest.mark.parametrize("dtype", ["BF16", "FP32", "FP16", "FP8", "FP16X2"])
def test_records_of_detect_jpegs_equal_detect_images(hiplib, decoded, dtype):
    """the mini network in the four storage types it plans in.  Split-fp16 pairs refuse its 8-channel [route] when the cfg is planned -- that refusal is
    asserted, by its text -- and are compared on the YOLOv3 topology at 160 x 160 instead, as tests/test_gpu_frames.py does: no case goes uncompared"""
    thr = 0.05
    if dtype == "FP16X2":
        with pytest.raises(hiplib.YoloError, match=r"^yolo_create: layer \d+: \[route\] copies the 8 channels .* on split-fp16 pairs a copied source needs whole 32-channel groups"):
            _mini(hiplib, hiplib.FP16X2, max_batch=6)
        e, thr = _engine(hiplib, dtype=hiplib.FP16X2, max_batch=6), POST["score_thr"]
    else:
        e = _mini(hiplib, getattr(hiplib, dtype), max_batch=6)
    names = ["dog", "giraffe", "c50x35_420_std", "c33x31_440_opt", "g32x8", "person"]
    files = [_file(n) for n in names]
    kept = 0
    for kw in (dict(fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS, nms_mode=hiplib.NMS_TF),
               dict(fit=hiplib.FIT_LETTERBOX, units=hiplib.UNITS_SOURCE_PIXELS, nms_mode=hiplib.NMS_DARKNET)):
        want = e.detect_images([decoded[k] for k in names], score_thr=thr, iou_thr=0.45, max_out=30, **kw)
        got = e.detect_jpegs(files, score_thr=thr, iou_thr=0.45, max_out=30, **kw)
        assert len(got) == len(names)
        for i in range(len(names)):
            assert _recs_equal(got[i], want[i]), (dtype, kw["fit"], names[i])
            kept += len(want[i])
    if dtype in ("BF16", "FP16X2"):
        assert kept > 0
    e.close()


# ---- 4: graph ----
def test_graph_replays_over_two_decoded_batches(hiplib, decoded):
    """eager, capture, then replays: the table of each decode goes to yolo_detect_frames_graph with the surface's pointer and capacity, which both
    decodes share -- the captured step's key --, so the second batch is a replay; each call's records equal the eager detect_images of the
    reference's bytes."""
    import torch
    e = _engine(hiplib, max_batch=3)
    n, mo = 3, 30
    sets = [["dog", "c50x35_420_std", "kite"], ["person", "giraffe", "c33x31_422_rst1"]]
    files = [[_file(k) for k in s] for s in sets]
    boxes = torch.zeros(n * mo * 6, dtype=torch.int32, device="cuda"); counts = torch.zeros(n, dtype=torch.int32, device="cuda")
    kw = dict(fit=hiplib.FIT_STRETCH, units=hiplib.UNITS_SOURCE_PIXELS)
    want = [e.detect_images([decoded[k] for k in s], **kw, **POST) for s in sets]
    assert all(sum(len(r) for r in w) > 0 for w in want)
    surfaces = set()
    for step, k in enumerate([0, 0, 1, 0, 1]):          # call 1 eager, call 2 captures, then three replays
        handle = e.decode_jpegs(files[k])
        surfaces.add((handle.pixels, handle.nbytes))
        e.detect_frames_graph(handle.pixels, handle.descs, boxes, counts, nbytes=handle.nbytes, max_out=mo, score_thr=POST["score_thr"], iou_thr=POST["iou_thr"], **kw)
        e.synchronize()
        b = boxes.cpu().numpy().view(hiplib.BOX_DTYPE).reshape(n, mo); c = counts.cpu().numpy()
        for i in range(n):
            assert _recs_equal(b[i, :c[i]], want[k][i]), "call %d file %s" % (step + 1, sets[k][i])
    assert len(surfaces) == 1          # one buffer, one size: nothing in the key changed between the batches
    e.close()


# ---- 5: tiling ----
@pytest.mark.parametrize("photo", ["kite", "dog"])
def test_tiled_jpegs_equal_tiled_frames_of_the_reference_bytes(hiplib, decoded, photo):
    """windows of 321 x 323 pixels: the pulled-back last row and column of windows begin on an odd row and an odd column (kite: 579, 1029; dog: 255, 445), where
    the chroma upsampling of the 4:4:0 photograph (dog) depends on the position in the frame, not in the window"""
    e = _mini(hiplib, hiplib.BF16, max_batch=8)
    rgb = decoded[photo]
    wins = hiplib.tile_windows(rgb.shape[:2], (321, 323), 32)
    assert (wins[-1, 0] & 1) and (wins[-1, 1] & 1)
    frame = hiplib.Frame(rgb, rgb.shape[0], rgb.shape[1], hiplib.PIX_RGB24)
    kept = 0
    for kw in (dict(fit=hiplib.FIT_STRETCH, nms_mode=hiplib.NMS_TF, relative=False), dict(fit=hiplib.FIT_LETTERBOX, nms_mode=hiplib.NMS_DARKNET, relative=True)):
        want = e.detect_tiled_frames([frame], tile=(321, 323), overlap=32, score_thr=0.05, iou_thr=0.45, max_out=30, **kw)
        got = e.detect_tiled_jpegs([_photo(photo)], tile=(321, 323), overlap=32, score_thr=0.05, iou_thr=0.45, max_out=30, **kw)
        assert len(got) == 1 and _recs_equal(got[0], want[0]), (photo, kw["fit"])
        kept += len(want[0])
    assert kept > 0
    e.close()


# ---- 6: the detector class, the veneer ----
def test_detector_files_equal_detector_images_of_the_host_decodes(hiplib, decoded):
    from yolo_tensorflow_amd.detector import YOLOV3
    secs = IO.parse_cfg(IO.cfg_text("yolov3"))
    d = YOLOV3(None, weights=IO.synth_weights(secs, seed=7), max_batch=4)
    d.threshold = 0.3
    photos = ["dog", "eagle", "giraffe", "horses", "kite", "person"]
    paths = [_photo(p) for p in photos]
    kept = 0
    for large in (False, True):
        if large:          # six windows of the network's size per photograph; a threshold at which their candidates fit one NMS launch
            d.threshold = 0.9
            got, want = d.detect_from_large_files(paths[:2]), d.detect_from_large_images([decoded[p] for p in photos[:2]])
        else:
            got, want = d.detect_from_files(paths), d.detect_from_images([decoded[p] for p in photos])
        assert len(got) == len(want)
        for g, w in zip(got, want):
            for a, b in zip(g, w):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            kept += len(w[0])
    assert kept > 0
    d.engine.close()


def test_veneer_resizes_a_jpeg_as_it_resizes_a_ppm(hiplib, decoded, tmp_path):
    """load_image_color(dog.jpg, 416, 416) of libdarknet_hip.so equals its load_image_color of the PPM that holds the reference's decoded bytes
    (the same resize over the same pixels), and the compiled reference's where this checkout has built it (to the PPM path's tolerance)"""
    ven = C.CDLL(os.path.join(JH.ROOT, "yolo_tensorflow_amd", "libdarknet_hip.so"))
    ven.load_image_color.argtypes = [C.c_char_p, C.c_int, C.c_int]; ven.load_image_color.restype = JH._RefImage
    ven.free_image.argtypes = [JH._RefImage]; ven.free_image.restype = None
    rgb = decoded["dog"]
    ppm = str(tmp_path / "dog.ppm")
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]) + rgb.tobytes())
    a = ven.load_image_color(_photo("dog").encode(), 416, 416)
    b = ven.load_image_color(ppm.encode(), 416, 416)
    assert (a.w, a.h, a.c) == (416, 416, 3) and a.data and b.data
    x = np.ctypeslib.as_array(a.data, shape=(3, 416, 416)).copy()
    assert x.any() and np.array_equal(x, np.ctypeslib.as_array(b.data, shape=(3, 416, 416)))
    ven.free_image(a); ven.free_image(b)
    if os.path.exists(JH.REF_LIB):
        ref = C.CDLL(JH.REF_LIB)
        ref.load_image_color.argtypes = [C.c_char_p, C.c_int, C.c_int]; ref.load_image_color.restype = JH._RefImage
        ref.free_image.argtypes = [JH._RefImage]; ref.free_image.restype = None
        r = ref.load_image_color(_photo("dog").encode(), 416, 416)
        np.testing.assert_allclose(x, np.ctypeslib.as_array(r.data, shape=(3, 416, 416)), rtol=0, atol=2e-6)
        ref.free_image(r)


# ---- 7: refusals ----
def test_refusals_come_before_any_launch_and_name_the_file(hiplib, decoded):
    e = _mini(hiplib, hiplib.BF16, max_batch=4)
    good = [JH.path_of("c17x9_420_rst1"), JH.path_of("g23x19")]
    first = e.detect_jpegs(good, score_thr=0.05)
    staged = e.staged_input(2)
    with open(good[0], "rb") as f:
        data = f.read()
    for bad, code, words in (([good[0], JH.path_of("refused_progressive")], -6, ("file 1", "progressive")),
                             ([JH.path_of("refused_cmyk"), good[1]], -6, ("file 0", "4-component")),
                             ([good[0], good[1], data[:len(data) - 40]], -1, ("file 2", "offset")),
                             ([good[0], b"not a jpeg at all"], -1, ("file 1", "not a JPEG"))):
        for call in (e.decode_jpegs, e.forward_jpegs, e.detect_jpegs, lambda files: e.detect_tiled_jpegs(files, overlap=16)):
            with pytest.raises(hiplib.YoloError) as err:
                call(bad)
            assert "(%d)" % code in str(err.value) and all(w in str(err.value) for w in words), err.value
    # what the frames forms refuse, asked before the decode's launch: the batch size, the fit
    with pytest.raises(hiplib.YoloError, match=r"\(-1\).*batch 5"):
        e.detect_jpegs(good * 2 + good[:1])
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*YOLO_FIT_CV2_BGR"):
        e.forward_jpegs(good, fit=hiplib.FIT_CV2_BGR)
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*YOLO_FIT_CENTER_CROP"):
        e.detect_jpegs(good, fit=hiplib.FIT_CENTER_CROP)
    with pytest.raises(hiplib.YoloError, match=r"\(-6\).*yolo_detect_tiled_jpegs.*YOLO_NMS_PER_CLASS"):
        e.detect_tiled_jpegs(good, overlap=16, nms_mode=hiplib.NMS_PER_CLASS)
    with pytest.raises(hiplib.YoloError):
        e.detect_jpegs([])
    # no refused call launched anything: the staged input is still the last good call's, and the engine answers as before
    assert np.array_equal(e.staged_input(2), staged)
    again = e.detect_jpegs(good, score_thr=0.05)
    assert all(_recs_equal(x, y) for x, y in zip(first, again))
    e.close()
