"""Decoded video frames on the host: yolo_frame_to_rgb_host against a numpy restatement of the colour rule -- every
(Y, U, V) triple under all three matrices, odd sizes, pitches above the row, planes in any order --, pack_frames, the refusals of a
descriptor, the export list.  No GPU.  tests/test_gpu_frames.py holds the device to the same restatement (ref_rgb below)."""
import os
import re
import ctypes as C
import numpy as np
import pytest
from yolo_tensorflow_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NV12, I420, RGB24, BGR24 = hip.PIX_NV12, hip.PIX_I420, hip.PIX_RGB24, hip.PIX_BGR24
MATRICES = (hip.MATRIX_BT601, hip.MATRIX_BT709, hip.MATRIX_BT601_FULL)
#            yoff  CY       CVR      CUG     CVG     CUB
TABLE = {hip.MATRIX_BT601: (16, 1220542, 1673527, 409993, 852492, 2116026),
         hip.MATRIX_BT709: (16, 1220542, 1880097, 223347, 558891, 2214593),
         hip.MATRIX_BT601_FULL: (0, 1048576, 1470104, 360853, 748826, 1858077)}
LAYOUT_SIZES = [(1, 1), (1, 2), (2, 1), (3, 5), (5, 3), (16, 18)]


def ref_rgb(buf, offset, pitch, h, w, fmt, matrix):
    """The rule restated: integer numpy over the flat uint8 buffer -> [h, w, 3] uint8.  Chroma from (y >> 1, x >> 1); int32 throughout; `>>`
    arithmetic."""
    buf = np.asarray(buf).reshape(-1)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    if fmt in (RGB24, BGR24):
        p = offset[0] + y * pitch[0] + 3 * x
        rgb = np.stack([buf[p], buf[p + 1], buf[p + 2]], -1)
        return np.ascontiguousarray(rgb[..., ::-1] if fmt == BGR24 else rgb)
    Y = buf[offset[0] + y * pitch[0] + x].astype(np.int32)
    cy, cx = y >> 1, x >> 1
    if fmt == NV12:
        U = buf[offset[1] + cy * pitch[1] + 2 * cx].astype(np.int32); V = buf[offset[1] + cy * pitch[1] + 2 * cx + 1].astype(np.int32)
    else:
        U = buf[offset[1] + cy * pitch[1] + cx].astype(np.int32); V = buf[offset[2] + cy * pitch[2] + cx].astype(np.int32)
    yoff, CY, CVR, CUG, CVG, CUB = (np.int32(k) for k in TABLE[matrix])
    yp = np.maximum(np.int32(0), Y - yoff) * CY; u = U - np.int32(128); v = V - np.int32(128)
    half = np.int32(1 << 19)
    R = (yp + CVR * v + half) >> 20
    G = (yp - CUG * u - CVG * v + half) >> 20
    B = (yp + CUB * u + half) >> 20
    out = np.stack([R, G, B], -1)
    assert out.dtype == np.int32
    return np.clip(out, 0, 255).astype(np.uint8)


def ref_of(frame):
    return ref_rgb(frame.data, frame.offsets, frame.pitch, frame.h, frame.w, frame.format, frame.matrix)


def make_frame(rng, h, w, fmt, matrix=hip.MATRIX_BT601, y_extra=3, c_extra=5, reverse=True, gap=7, planes=None):
    """A frame of random (or given) plane contents at pitches above the row -- Y (and RGB / BGR) rows `y_extra` bytes wider, chroma rows
    `c_extra` --, the planes laid into the buffer in reverse order with `gap` bytes in front of each; everything that is no sample is 0xFF."""
    rows = hip.frame_plane_rows(h, w, fmt)
    pitch = [row + (y_extra if p == 0 else c_extra) for p, (_, row) in enumerate(rows)]
    order = list(range(len(rows)))[::-1] if reverse else list(range(len(rows)))
    offsets, off = [0] * len(rows), 0
    for p in order:
        off += gap
        offsets[p] = off
        off += rows[p][0] * pitch[p]
    buf = np.full(off + gap, 0xFF, dtype=np.uint8)
    for p, (r, row) in enumerate(rows):
        content = rng.integers(0, 256, (r, row), dtype=np.uint8) if planes is None else np.asarray(planes[p], dtype=np.uint8).reshape(r, row)
        view = np.lib.stride_tricks.as_strided(buf[offsets[p]:], shape=(r, row), strides=(pitch[p], 1))
        view[...] = content
    return hip.Frame(buf, h, w, fmt, matrix=matrix, pitch=pitch, offsets=offsets)


def exhaustive_planes(k, fmt):
    """frame k of 64, 512 x 512: U = x >> 1 and V = y >> 1 over every chroma pair, four Y values per 2 x 2 block: 4k + 2 (y & 1) + (x & 1)"""
    y, x = np.mgrid[0:512, 0:512]
    Y = (4 * k + 2 * (y & 1) + (x & 1)).astype(np.uint8)
    cy, cx = np.mgrid[0:256, 0:256]
    U, V = cx.astype(np.uint8), cy.astype(np.uint8)
    if fmt == NV12:
        return [Y, np.stack([U, V], -1).reshape(256, 512)]
    return [Y, U, V]


@pytest.mark.parametrize("fmt", [NV12, I420])
@pytest.mark.parametrize("matrix", MATRICES)
def test_every_yuv_triple_equals_the_restatement(fmt, matrix):
    seen = np.zeros(256, dtype=bool)
    for k in range(64):
        planes = exhaustive_planes(k, fmt)
        f = hip.Frame(np.concatenate([p.reshape(-1) for p in planes]), 512, 512, fmt, matrix=matrix)
        got = hip.frame_to_rgb(f)
        assert np.array_equal(got, ref_of(f)), "matrix %d format %d frame %d" % (matrix, fmt, k)
        seen[np.unique(planes[0])] = True
    assert seen.all()


def layout_frames(rng):
    """the layouts both the host and the device are held to: every size in NV12 and I420 under each matrix at pitches above the row, planes
    reversed with 0xFF between them; RGB24 and BGR24 at a pitch of 3w + 1"""
    out = []
    for i, (h, w) in enumerate(LAYOUT_SIZES):
        for j, fmt in enumerate((NV12, I420)):
            out.append(make_frame(rng, h, w, fmt, MATRICES[(i + j) % 3]))
        for fmt in (RGB24, BGR24):
            out.append(make_frame(rng, h, w, fmt, y_extra=1))
    return out


def test_layouts_pitches_and_plane_order():
    rng = np.random.default_rng(22)
    for f in layout_frames(rng):
        rows = hip.frame_plane_rows(f.h, f.w, f.format)
        assert all(p > row for p, (_, row) in zip(f.pitch, rows))
        if len(rows) > 1:
            assert f.offsets == sorted(f.offsets, reverse=True)
        got = hip.frame_to_rgb(f)
        assert got.shape == (f.h, f.w, 3) and np.array_equal(got, ref_of(f)), (f.h, f.w, f.format, f.matrix)
    # the RGB formats are the image's own bytes; BGR swaps channels 0 and 2
    img = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    assert np.array_equal(hip.frame_to_rgb(hip.Frame(img, 5, 3, RGB24)), img)
    assert np.array_equal(hip.frame_to_rgb(hip.Frame(img, 5, 3, BGR24)), img[..., ::-1])


def test_pack_frames_round_trips():
    rng = np.random.default_rng(23)
    frames = [make_frame(rng, 3, 5, NV12, hip.MATRIX_BT709), make_frame(rng, 16, 18, I420, hip.MATRIX_BT601_FULL), make_frame(rng, 5, 3, BGR24, y_extra=1),
              hip.Frame(rng.integers(0, 256, 4 * 6 * 3, dtype=np.uint8), 4, 6, RGB24)]
    buf, descs = hip.pack_frames(frames)
    assert descs.dtype == hip.FRAME_DTYPE and hip.FRAME_DTYPE.itemsize == 64 and buf.size == sum(f.data.size for f in frames)
    base = 0
    for i, f in enumerate(frames):
        d, n = descs[i], len(f.offsets)
        assert [int(v) for v in d["offset"][:n]] == [base + o for o in f.offsets] and [int(v) for v in d["pitch"][:n]] == f.pitch
        assert (int(d["h"]), int(d["w"]), int(d["format"]), int(d["matrix"])) == (f.h, f.w, f.format, f.matrix)
        assert np.array_equal(buf[base:base + f.data.size], f.data)
        # read back through the descriptor: the frame inside the packed buffer is the frame alone
        assert np.array_equal(hip.frame_to_rgb((buf, descs[i:i + 1])), hip.frame_to_rgb(f))
        back = hip.Frame(buf[base:base + f.data.size], int(d["h"]), int(d["w"]), int(d["format"]), matrix=int(d["matrix"]),
                         pitch=[int(v) for v in d["pitch"][:n]], offsets=[int(v) - base for v in d["offset"][:n]])
        assert np.array_equal(back.desc(base).view(np.uint8), descs[i:i + 1].view(np.uint8))
        base += f.data.size
    with pytest.raises(hip.YoloError):
        hip.pack_frames([])
    with pytest.raises(hip.YoloError):
        hip.pack_frames([np.zeros((4, 4, 3), np.uint8)])


def bad_descs(buf, d):
    """(descriptor, bytes, what) for everything a descriptor is refused for; `d` a valid NV12 FRAME_DTYPE record [1] inside `buf`"""
    def edit(**kw):
        e = d.copy()
        for k, v in kw.items():
            if isinstance(v, tuple):
                e[k][0, v[0]] = v[1]
            else:
                e[k][0] = v
        return e
    h, w = int(d["h"][0]), int(d["w"][0])
    yield edit(format=4), buf.size, "format"
    yield edit(format=-1), buf.size, "format"
    yield edit(matrix=3), buf.size, "matrix"
    yield edit(matrix=-1), buf.size, "matrix"
    yield edit(h=0), buf.size, "0 x"
    yield edit(w=-2), buf.size, "x -2"
    yield edit(pitch=(0, w - 1)), buf.size, "pitch"
    yield edit(pitch=(1, 2 * ((w + 1) // 2) - 1)), buf.size, "pitch"
    yield edit(pitch=(0, 2 ** 32)), buf.size, "32 bits"
    yield edit(pitch=(1, 2 ** 40)), buf.size, "32 bits"
    yield edit(offset=(1, 2 ** 32)), buf.size, "32 bits"
    yield edit(offset=(0, 2 ** 32 - 4)), buf.size, "32 bits"
    yield edit(offset=(0, int(d["offset"][0, 0]) + 1)), int(d["offset"][0, 0]) + (h - 1) * int(d["pitch"][0, 0]) + w, "past"
    yield d, int(d["offset"][0, 1]) + ((h + 1) // 2 - 1) * int(d["pitch"][0, 1]) + 2 * ((w + 1) // 2) - 1, "past"
    yield edit(h=h + 2), buf.size, "past"


def test_host_refuses_bad_descriptors():
    lib = hip.load_library()
    rng = np.random.default_rng(24)
    f = make_frame(rng, 6, 9, NV12, reverse=False, gap=0)
    d = f.desc()
    out = np.full((16, 16, 3), 7, np.uint8)
    assert lib.yolo_frame_to_rgb_host(d.ctypes.data, f.data.ctypes.data, f.data.size, out.ctypes.data) == 0
    # the bytes that are exactly enough are enough
    exact = int(d["offset"][0, 1]) + 2 * int(d["pitch"][0, 1]) + 10
    assert exact < f.data.size and lib.yolo_frame_to_rgb_host(d.ctypes.data, f.data.ctypes.data, exact, out.ctypes.data) == 0
    n = 0
    for e, nbytes, what in bad_descs(f.data, d):
        out[...] = 7
        e = np.ascontiguousarray(e)
        rc = lib.yolo_frame_to_rgb_host(e.ctypes.data, f.data.ctypes.data, nbytes, out.ctypes.data)
        msg = lib.yolo_last_error(None).decode()
        assert rc == -1 and "frame 0" in msg and what in msg, (what, rc, msg)
        assert (out == 7).all()
        n += 1
    assert n == 15
    # the planes a format does not have are not read: an RGB frame with wild plane 1 / 2 fields converts
    g = hip.Frame(rng.integers(0, 256, 12, dtype=np.uint8), 2, 2, RGB24).desc()
    g["offset"][0, 1:] = 2 ** 50; g["pitch"][0, 1:] = 0
    assert lib.yolo_frame_to_rgb_host(g.ctypes.data, f.data.ctypes.data, f.data.size, out.ctypes.data) == 0
    for args in [(None, f.data.ctypes.data, out.ctypes.data), (d.ctypes.data, None, out.ctypes.data), (d.ctypes.data, f.data.ctypes.data, None)]:
        assert lib.yolo_frame_to_rgb_host(args[0], args[1], f.data.size, args[2]) == -1


def test_new_entry_points_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(yolo_[a-z0-9_]+)\s*\(", text))
    new = {"yolo_frame_to_rgb_host", "yolo_op_frame_to_rgb", "yolo_forward_frames_u8", "yolo_detect_frames_u8", "yolo_detect_frames_graph",
           "yolo_detect_tiled_frames_u8"}
    lib = hip.load_library()
    assert new <= declared and new <= set(hip.EXPORTS)
    for name in new:
        assert hasattr(lib, name)
    assert "yolo_frame_desc" in text and "YOLO_PIX_NV12" in text and "YOLO_MATRIX_BT601_FULL" in text

    class FrameDesc(C.Structure):
        _fields_ = [("offset", C.c_uint64 * 3), ("pitch", C.c_uint64 * 3), ("h", C.c_int32), ("w", C.c_int32), ("format", C.c_int32), ("matrix", C.c_int32)]
    assert C.sizeof(FrameDesc) == hip.FRAME_DTYPE.itemsize == 64
    for name in ("offset", "pitch", "h", "w", "format", "matrix"):
        assert getattr(FrameDesc, name).offset == hip.FRAME_DTYPE.fields[name][1]
