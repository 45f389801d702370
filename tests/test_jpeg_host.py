"""JPEG files on the host: the host twin of the decode (yolo_jpeg_to_rgb_host) against what the compiled reference decodes
-- tests/golden/jpeg_cases.npz, written by tools/make_jpeg_cases.py from load_image of oracle/_ref, and load_image itself where oracle/_ref is built --
bit for bit; the JPEG frame formats against planes a numpy restatement of the IDCT makes from the library's coefficients; the headers; the refusals;
load_image_color of libdarknet_hip.so; and malformed input through a sanitizer build of the host stage.  No GPU.  tests/test_gpu_jpeg.py holds the
device to the same fixtures."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import sys
import numpy as np
import pytest
from conftest import golden
from yolo_tensorflow_amd import hip
import test_frames_host as FH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JPEG = os.path.join(ROOT, "tests", "golden", "jpeg")
IMAGES = os.path.join(ROOT, "tests", "golden", "images")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")
FORMATS = {"444": hip.PIX_JPEG_444, "422": hip.PIX_JPEG_422, "420": hip.PIX_JPEG_420, "440": hip.PIX_JPEG_440}
SAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}
INVALID, UNSUPPORTED = -1, -6          # YOLO_ERR_INVALID, YOLO_ERR_UNSUPPORTED (include/yolo_hip.h)


def cases():
    """jpeg_cases.npz; a missing fixture fails, it does not skip"""
    g = golden("jpeg_cases.npz")
    names = [str(n) for n in g["names"]]
    # the matrix the fixtures must hold: eight sizes x four samplings x three variants, a restart interval of three MCUs, both ends of the quality scale, grey
    for w, h in [(1, 1), (2, 2), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (50, 35)]:
        for sub in FORMATS:
            for var in ("std", "opt", "rst1"):
                assert "c%dx%d_%s_%s" % (w, h, sub, var) in names
    for need in ("c50x35_444_rst3", "c50x35_422_rst3", "c50x35_420_rst3", "c50x35_440_rst3", "c50x35_420_q10", "c33x31_422_q100", "g1x1", "g23x19", "g32x8"):
        assert need in names
    return g, names


def path_of(name):
    p = os.path.join(JPEG, name + ".jpg")
    assert os.path.exists(p), p
    return p


def name_geometry(name):
    """(w, h, sampling key or None for grey, restart interval) from a fixture's name"""
    m = re.match(r"^([cg])(\d+)x(\d+)(?:_(\d{3})_(\w+))?$", name)
    assert m, name
    var = m.group(5) or ""
    return int(m.group(2)), int(m.group(3)), m.group(4), 1 if var == "rst1" else 3 if var == "rst3" else 0


# ---- the IDCT restated: stb_image.h stbi__idct_block in int32 numpy, vectorised over blocks ----
def _idct_1d(s, bias, shift):
    """s: eight int32 arrays -> eight int32 arrays (the pass of kernels.h jpeg_idct_1d)"""
    i32 = np.int32
    p2, p3 = s[2], s[6]
    p1 = (p2 + p3) * i32(2217)
    t2 = p1 + p3 * i32(-7567); t3 = p1 + p2 * i32(3135)
    p2, p3 = s[0], s[4]
    t0 = (p2 + p3) * i32(4096); t1 = (p2 - p3) * i32(4096)
    x0 = t0 + t3 + i32(bias); x3 = t0 - t3 + i32(bias); x1 = t1 + t2 + i32(bias); x2 = t1 - t2 + i32(bias)
    t0, t1, t2, t3 = s[7], s[5], s[3], s[1]
    p3 = t0 + t2; p4 = t1 + t3; p1 = t0 + t3; p2 = t1 + t2
    p5 = (p3 + p4) * i32(4816)
    t0 = t0 * i32(1223); t1 = t1 * i32(8410); t2 = t2 * i32(12586); t3 = t3 * i32(6149)
    p1 = p5 + p1 * i32(-3685); p2 = p5 + p2 * i32(-10497); p3 = p3 * i32(-8034); p4 = p4 * i32(-1597)
    t3 = t3 + p1 + p4; t2 = t2 + p2 + p3; t1 = t1 + p2 + p4; t0 = t0 + p1 + p3
    out = [x0 + t3, x1 + t2, x2 + t1, x3 + t0, x3 - t0, x2 - t1, x1 - t2, x0 - t3]
    assert all(o.dtype == np.int32 for o in out)
    return [o >> shift for o in out]


def idct_plane(coef):
    """coef int16 [bh, bw, 8, 8] (natural order) -> the uint8 plane [8 bh, 8 bw]"""
    c = coef.astype(np.int32)
    cols = np.stack(_idct_1d([c[:, :, r, :] for r in range(8)], 512, 10), 2)                      # the column pass: over rows r, per column
    rows = np.stack(_idct_1d([cols[:, :, :, u] for u in range(8)], 65536 + (128 << 17), 17), 3)      # the row pass: over columns u, per row
    px = np.clip(rows, 0, 255).astype(np.uint8)
    bh, bw = coef.shape[:2]
    return np.ascontiguousarray(px.transpose(0, 2, 1, 3).reshape(8 * bh, 8 * bw))


def restated_frame(name, rng=None):
    """a fixture as a hip.Frame over planes the restated IDCT makes of the library's coefficients.  rng: at pitches above the row, planes in reverse
    order, 0xFF between them (FH.make_frame); None: the padded planes themselves, back to back"""
    info = hip.jpeg_info(path_of(name))
    planes = [idct_plane(c) for c in hip.jpeg_coefficients(path_of(name))]
    assert [p.shape for p in planes] == info["planes"]
    if rng is None:
        offsets = [int(o) for o in np.cumsum([0] + [p.size for p in planes[:-1]])]
        return hip.Frame(np.concatenate([p.reshape(-1) for p in planes]), info["h"], info["w"], info["format"], pitch=[p.shape[1] for p in planes], offsets=offsets)
    rows = hip.frame_plane_rows(info["h"], info["w"], info["format"])
    return FH.make_frame(rng, info["h"], info["w"], info["format"], 0, planes=[p[:r, :c] for p, (r, c) in zip(planes, rows)])


# ---- 1: the decode ----
def test_host_decode_equals_the_reference_on_every_fixture():
    g, names = cases()
    for name in names:
        want = g["rgb/" + name]
        got = hip.jpeg_to_rgb(path_of(name))
        assert got.shape == want.shape and np.array_equal(got, want), name
        with open(path_of(name), "rb") as f:          # bytes in place of a path
            assert np.array_equal(hip.jpeg_to_rgb(f.read()), want), name


def test_host_decode_matches_the_photographs():
    g, _ = cases()
    kinds = {}
    for name, sha, hw in zip(g["photos"], g["photo_sha256"], g["photo_hw"]):
        p = os.path.join(IMAGES, str(name) + ".jpg")
        got = hip.jpeg_to_rgb(p)
        assert got.shape == (int(hw[0]), int(hw[1]), 3)
        assert hashlib.sha256(got.tobytes()).hexdigest() == str(sha), name
        kinds[str(name)] = hip.jpeg_info(p)["format"]
    assert sorted(kinds) == ["dog", "eagle", "giraffe", "horses", "kite", "person"]
    # four are sampled 1 x 2 (4:4:0), two 1 x 1
    assert kinds == {"dog": hip.PIX_JPEG_440, "eagle": hip.PIX_JPEG_440, "horses": hip.PIX_JPEG_440, "person": hip.PIX_JPEG_440,
                     "giraffe": hip.PIX_JPEG_444, "kite": hip.PIX_JPEG_444}


class _RefImage(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


def _planar(rgb):
    """darknet's image of uint8 [h, w, 3]: CHW, (float)(byte / 255.)"""
    return (rgb.transpose(2, 0, 1).astype(np.float64) / 255.).astype(np.float32)


def test_host_decode_equals_load_image_where_the_reference_is_built():
    """the compiled reference called directly, when this checkout has built it; the committed decodes of jpeg_cases.npz hold either way"""
    if not os.path.exists(REF_LIB):
        return
    ref = C.CDLL(REF_LIB)
    ref.load_image.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]; ref.load_image.restype = _RefImage
    ref.free_image.argtypes = [_RefImage]; ref.free_image.restype = None
    _, names = cases()
    for p in [path_of(n) for n in names] + [os.path.join(IMAGES, n + ".jpg") for n in ("dog", "giraffe")]:
        im = ref.load_image(p.encode(), 0, 0, 3)
        want = np.ctypeslib.as_array(im.data, shape=(3, im.h, im.w)).copy()
        ref.free_image(im)
        assert np.array_equal(_planar(hip.jpeg_to_rgb(p)), want), p


# ---- 2: the frame formats ----
def test_frame_formats_read_restated_planes_as_the_decode():
    g, names = cases()
    rng = np.random.default_rng(41)
    seen = set()
    for name in names:
        want = g["rgb/" + name]
        packed = restated_frame(name)
        assert np.array_equal(hip.frame_to_rgb(packed), want), name
        f = restated_frame(name, rng)          # pitches above the row, planes reversed, every byte that is no sample 0xFF
        rows = hip.frame_plane_rows(f.h, f.w, f.format)
        assert all(p > row for p, (_, row) in zip(f.pitch, rows)) and f.offsets == sorted(f.offsets, reverse=True)
        assert np.array_equal(hip.frame_to_rgb(f), want), name
        seen.add((f.format, f.w <= 2, f.h & 1, f.w & 1))
    for fmt in FORMATS.values():          # every sampling with one chroma sample per row, and at odd sizes
        assert (fmt, True, 1, 1) in seen and (fmt, False, 1, 1) in seen


def test_frame_descriptor_rules_of_the_jpeg_formats():
    lib = hip.load_library()
    f = restated_frame("c17x9_420_std")
    out = np.full((17, 17, 3), 7, np.uint8)

    def rc(**kw):
        d = f.desc()
        for k, v in kw.items():
            if isinstance(v, tuple):
                d[k][0, v[0]] = v[1]
            else:
                d[k][0] = v
        out[...] = 7
        r = lib.yolo_frame_to_rgb_host(d.ctypes.data, f.data.ctypes.data, f.data.size, out.ctypes.data)
        assert r == 0 or (out == 7).all()
        return r, (lib.yolo_last_error(None) or b"").decode()
    assert rc()[0] == 0
    for fmt in (4, 5, 15, 21):          # 4 stays no format; so does everything between the two families and past the last
        r, msg = rc(format=fmt)
        assert r == INVALID and "format" in msg
    r, msg = rc(matrix=3)
    assert r == INVALID and "matrix" in msg
    for m in (1, 2):          # a JPEG format carries its rule: the matrix selects nothing and must be 0
        r, msg = rc(matrix=m)
        assert r == INVALID and "matrix" in msg and "JPEG" in msg
    # a chroma plane of ceil(h / 2) rows of ceil(w / 2) bytes is enough, at any pitch; one byte less is refused
    assert rc(pitch=(1, 9))[0] == 0 and rc(pitch=(1, 8))[0] == INVALID
    assert rc(h=16)[0] == 0 and rc(h=17)[0] == INVALID          # (the padded planes hold 16 x 32 luma, 8 x 16 chroma: 8 chroma rows lie inside the buffer, 9 end past it)
    # format 4 and matrix 3 on a video frame, as before
    v = FH.make_frame(np.random.default_rng(1), 6, 9, FH.NV12, reverse=False, gap=0)
    for kw in (dict(format=4), dict(matrix=3)):
        d = v.desc()
        for k, val in kw.items():
            d[k][0] = val
        assert lib.yolo_frame_to_rgb_host(d.ctypes.data, v.data.ctypes.data, v.data.size, np.zeros((6, 9, 3), np.uint8).ctypes.data) == INVALID


# ---- 3: headers and refusals ----
def test_info_geometry_of_every_fixture():
    _, names = cases()
    for name in names:
        w, h, sub, rst = name_geometry(name)
        info = hip.jpeg_info(path_of(name))
        hs, vs = SAMPLING[sub] if sub else (1, 1)
        mw, mh = -(-w // (8 * hs)), -(-h // (8 * vs))
        assert (info["w"], info["h"], info["hs"], info["vs"], info["restart_interval"], info["mcus"]) == (w, h, hs, vs, rst, (mw, mh)), name
        if sub:
            assert info["components"] == 3 and info["format"] == FORMATS[sub]
            assert info["planes"] == [(8 * mh * vs, 8 * mw * hs), (8 * mh, 8 * mw), (8 * mh, 8 * mw)] and info["blocks"] == [mw * hs * mh * vs, mw * mh, mw * mh], name
        else:
            assert info["components"] == 1 and info["format"] == hip.PIX_JPEG_GREY and info["planes"] == [(8 * mh, 8 * mw)] and info["blocks"] == [mw * mh], name
        # the planes hold the component's own samples
        for (ph, pw), (r, c) in zip(info["planes"], hip.frame_plane_rows(h, w, info["format"])):
            assert ph >= r and pw >= c


def test_refused_kinds_name_the_file_and_the_feature():
    g, _ = cases()
    assert sorted(str(n) for n in g["refused"]) == ["refused_cmyk", "refused_progressive"]
    lib = hip.load_library()
    for name, word in (("refused_progressive", "progressive"), ("refused_cmyk", "4-component")):
        with open(path_of(name), "rb") as f:
            data = f.read()
        for call in (hip.jpeg_info, hip.jpeg_to_rgb, hip.jpeg_coefficients):
            with pytest.raises(hip.YoloError, match=r"\(-6\): file 0: .*" + word):
                call(data)
        out = np.full(64 * 64 * 3, 7, np.uint8)
        assert lib.yolo_jpeg_to_rgb_host(data, len(data), out.ctypes.data, out.size) == UNSUPPORTED and (out == 7).all()


def test_malformed_files_are_invalid_with_the_offset():
    with open(path_of("c17x9_420_rst1"), "rb") as f:
        data = f.read()
    lib = hip.load_library()
    out = np.zeros(9 * 17 * 3, np.uint8)
    for bad, word in ((data[:len(data) // 2], "offset"), (data[:40], "truncated"), (b"\x89PNG\r\n\x1a\n" + data, "not a JPEG"), (data.replace(b"\xff\xd0", b"\x00\x00"), "restart marker")):
        assert lib.yolo_jpeg_to_rgb_host(bad, len(bad), out.ctypes.data, out.size) == INVALID
        msg = lib.yolo_last_error(None).decode()
        assert msg.startswith("file 0: ") and word in msg, msg
    assert lib.yolo_jpeg_to_rgb_host(data, len(data), out.ctypes.data, out.size - 1) == INVALID          # rgb_out too small


# ---- 4: libdarknet_hip.so ----
def test_veneer_load_image_color_reads_jpeg_as_the_reference():
    g, _ = cases()
    ven = C.CDLL(os.path.join(ROOT, "yolo_tensorflow_amd", "libdarknet_hip.so"))
    ven.load_image_color.argtypes = [C.c_char_p, C.c_int, C.c_int]; ven.load_image_color.restype = _RefImage
    ven.free_image.argtypes = [_RefImage]; ven.free_image.restype = None
    dog = os.path.join(IMAGES, "dog.jpg")
    im = ven.load_image_color(dog.encode(), 0, 0)
    assert (im.w, im.h, im.c) == (768, 576, 3) and im.data
    got = np.ctypeslib.as_array(im.data, shape=(3, 576, 768)).copy()
    ven.free_image(im)
    # the reference's bytes, by their digest, and its floats: (float)(byte / 255.)
    as_bytes = np.ascontiguousarray(np.rint(got.astype(np.float64) * 255.).astype(np.uint8).transpose(1, 2, 0))
    assert hashlib.sha256(as_bytes.tobytes()).hexdigest() == str(g["photo_sha256"][list(g["photos"]).index("dog")])
    assert np.array_equal(got, _planar(as_bytes))
    if os.path.exists(REF_LIB):
        ref = C.CDLL(REF_LIB)
        ref.load_image_color.argtypes = [C.c_char_p, C.c_int, C.c_int]; ref.load_image_color.restype = _RefImage
        ref.free_image.argtypes = [_RefImage]; ref.free_image.restype = None
        rim = ref.load_image_color(dog.encode(), 0, 0)
        assert np.array_equal(got, np.ctypeslib.as_array(rim.data, shape=(3, 576, 768)))
        ref.free_image(rim)
    for name in ("g23x19", "c33x31_422_opt"):          # a grey file: three equal planes
        im = ven.load_image_color(path_of(name).encode(), 0, 0)
        want = g["rgb/" + name]
        assert (im.h, im.w, im.c) == want.shape and np.array_equal(np.ctypeslib.as_array(im.data, shape=(3, im.h, im.w)), _planar(want)), name
        ven.free_image(im)
    bad = ven.load_image_color(path_of("refused_progressive").encode(), 0, 0)          # prints why, returns the empty image
    assert not bad.data and (bad.w, bad.h, bad.c) == (0, 0, 0)


# ---- 5: malformed input under the sanitizers ----
def test_malformed_input_sanitizer_run(tmp_path):
    """tests/c/jpeg_malformed.cpp built with yolo_jpeg.cpp under -fsanitize=address,undefined and run as a child process: every prefix and 2000 seeded
    single-byte corruptions of three fixtures; a clean status every time, no sanitizer report"""
    exe = str(tmp_path / "jpeg_malformed")
    # the sanitizers' runtimes are linked statically: the program needs nothing of the environment it is started in, which is passed on as it is
    # but for the two variables that would change what the sanitizers report
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + ROOT,
                            os.path.join(ROOT, "tests", "c", "jpeg_malformed.cpp"), os.path.join(ROOT, "yolo_tensorflow_amd", "csrc", "yolo_jpeg.cpp"),
                            "-pthread", "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    run = subprocess.run([exe] + [path_of(n) for n in ("c17x9_420_rst1", "c33x31_422_opt", "g23x19")], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.match(r"^ok (\d+) invalid (\d+) unsupported (\d+)$", run.stdout.strip())
    assert m and int(m.group(1)) >= 3 and int(m.group(2)) > 1000, run.stdout
    total = sum(os.path.getsize(path_of(n)) + 2001 for n in ("c17x9_420_rst1", "c33x31_422_opt", "g23x19"))
    assert sum(int(v) for v in m.groups()) == total
