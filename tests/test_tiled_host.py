"""Tiled detection, host side: the window grid of yolo_tile_windows (include/yolo_hip.h) against a pure-Python restatement of its rule and the
properties a cross-window merge relies on, the window record's layout as C sees it, and the exported entry points.  No device call is made."""
import ctypes
import os
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def axis_rule(L, T, O):
    """One axis of the rule, as the header states it -> [(start, extent)]."""
    assert L >= 1 and T >= 1 and 0 <= O < T
    if L <= T:
        return [(0, L)]
    S = T - O
    count = -(-(L - T) // S) + 1
    return [(min(k * S, L - T), T) for k in range(count)]


def grid_rule(img_hw, tile_hw, overlap_hw):
    ys = axis_rule(img_hw[0], tile_hw[0], overlap_hw[0]); xs = axis_rule(img_hw[1], tile_hw[1], overlap_hw[1])
    return np.array([(y0, x0, h, w) for y0, h in ys for x0, w in xs], dtype=np.int32).reshape(-1, 4)


def axis_cases():
    """(L, T, O): L < T, L == T, L == T + 1, (L - T) % S == 0 and its neighbours, O = 0, the largest overlap, one-pixel tiles."""
    out = []
    for T, O in [(1, 0), (2, 0), (2, 1), (5, 0), (5, 2), (5, 4), (7, 3), (16, 0), (16, 5), (16, 15), (96, 64), (416, 64)]:
        S = T - O
        Ls = {1, T - 1, T, T + 1, T + S - 1, T + S, T + S + 1, T + 3 * S - 1, T + 3 * S, T + 3 * S + 1, 2 * T, 2 * T + 1, 5 * T + 3}
        out += [(L, T, O) for L in sorted(Ls) if L >= 1]
    return out


AXES = axis_cases()


def test_axis_cases_cover_the_edges_named():
    assert any(L < T for L, T, O in AXES) and any(L == T for L, T, O in AXES) and any(L == T + 1 for L, T, O in AXES)
    assert any(L > T and (L - T) % (T - O) == 0 for L, T, O in AXES) and any(L > T and (L - T) % (T - O) == 1 for L, T, O in AXES)
    assert any(L > T + 1 and (L - T) % (T - O) == T - O - 1 for L, T, O in AXES) and any(O == 0 and L > T for L, T, O in AXES)


def test_windows_equal_the_rule_on_every_pair_of_axis_cases():
    from yolo_tensorflow_amd import hip
    # every case along y against a spread of cases along x (and the other way round): the two axes are independent in the rule
    some = AXES[::7]
    pairs = [(a, b) for a in AXES for b in some] + [(b, a) for a in AXES for b in some]
    for (Lh, Th, Oh), (Lw, Tw, Ow) in pairs:
        got = hip.tile_windows((Lh, Lw), (Th, Tw), (Oh, Ow))
        want = grid_rule((Lh, Lw), (Th, Tw), (Oh, Ow))
        assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), ((Lh, Lw), (Th, Tw), (Oh, Ow))


@pytest.mark.parametrize("other", [(1, 1, 0), (23, 7, 3)], ids=["x1", "x23"])
def test_grid_properties(other):
    """every window inside the image, every pixel covered, consecutive windows overlap by at least O, the count formula, row-major order"""
    from yolo_tensorflow_amd import hip
    Lw, Tw, Ow = other
    for L, T, O in AXES:
        w = hip.tile_windows((L, Lw), (T, Tw), (O, Ow)).astype(np.int64)
        ny = 1 if L <= T else -(-(L - T) // (T - O)) + 1
        nx = 1 if Lw <= Tw else -(-(Lw - Tw) // (Tw - Ow)) + 1
        assert len(w) == ny * nx, (L, T, O)
        assert (w[:, 0] >= 0).all() and (w[:, 1] >= 0).all() and (w[:, 2] >= 1).all() and (w[:, 3] >= 1).all()
        assert (w[:, 0] + w[:, 2] <= L).all() and (w[:, 1] + w[:, 3] <= Lw).all()
        assert (w[:, 2] == min(L, T)).all() and (w[:, 3] == min(Lw, Tw)).all()
        cover = np.zeros((L, Lw), dtype=bool)
        for y0, x0, h, ww in w:
            cover[y0:y0 + h, x0:x0 + ww] = True
        assert cover.all(), (L, T, O)
        grid = w.reshape(ny, nx, 4)
        assert (grid[:, :, 0] == grid[:, :1, 0]).all() and (grid[:, :, 1] == grid[:1, :, 1]).all()          # y outer, x inner
        assert (np.diff(grid[:, 0, 0]) > 0).all() and (np.diff(grid[0, :, 1]) > 0).all()                      # strictly ascending: row-major, no window twice
        if ny > 1:
            assert (grid[:-1, 0, 0] + T - grid[1:, 0, 0] >= O).all(), (L, T, O)
        if nx > 1:
            assert (grid[0, :-1, 1] + Tw - grid[0, 1:, 1] >= Ow).all()


def test_kite_at_416_with_overlap_64_is_four_by_three():
    from yolo_tensorflow_amd import hip
    w = hip.tile_windows((900, 1352), (416, 416), (64, 64))
    assert w.shape == (12, 4)
    assert sorted(set(w[:, 0].tolist())) == [0, 352, 484] and sorted(set(w[:, 1].tolist())) == [0, 352, 704, 936]
    assert np.array_equal(hip.tile_windows((900, 1352), 416, 64), w)          # an int means both axes


def test_count_only_and_capped_calls():
    from yolo_tensorflow_amd import hip
    lib = hip.load_library()
    n = ctypes.c_int(-7)
    assert lib.yolo_tile_windows(900, 1352, 416, 416, 64, 64, None, 0, ctypes.byref(n)) == 0 and n.value == 12
    out = np.full((5, 4), -1, dtype=np.int32)
    n = ctypes.c_int(-7)
    assert lib.yolo_tile_windows(900, 1352, 416, 416, 64, 64, out.ctypes.data, 3, ctypes.byref(n)) == 0 and n.value == 12
    assert np.array_equal(out[:3], grid_rule((900, 1352), (416, 416), (64, 64))[:3]) and (out[3:] == -1).all()


def test_bad_arguments_are_invalid_and_still_write_the_count():
    from yolo_tensorflow_amd import hip
    lib = hip.load_library()
    out = np.zeros((4, 4), dtype=np.int32)
    bad = [(0, 10, 4, 4, 0, 0), (10, -1, 4, 4, 0, 0), (10, 10, 0, 4, 0, 0), (10, 10, 4, -3, 0, 0), (10, 10, 4, 4, -1, 0), (10, 10, 4, 4, 0, -1),
           (10, 10, 4, 4, 4, 0), (10, 10, 4, 4, 0, 4), (10, 10, 4, 4, 9, 0)]
    for a in bad:
        n = ctypes.c_int(-7)
        assert lib.yolo_tile_windows(*a, out.ctypes.data, 4, ctypes.byref(n)) == INVALID, a
        assert n.value == 0 and not out.any(), a
        with pytest.raises(hip.YoloError, match=r"\(-1\)"):
            hip.tile_windows(a[:2], a[2:4], a[4:])
    assert lib.yolo_tile_windows(10, 10, 4, 4, 0, 0, out.ctypes.data, 4, None) == INVALID
    n = ctypes.c_int(-7)
    assert lib.yolo_tile_windows(10, 10, 4, 4, 0, 0, None, 4, ctypes.byref(n)) == INVALID and n.value == 0      # cap > 0 needs somewhere to write
    # extents near the top of an int neither overflow nor loop: 2^31 - 1 pixels at stride 1 is a count the int cannot hold, at stride 2^30 it is 2
    n = ctypes.c_int(-7)
    assert lib.yolo_tile_windows(2 ** 31 - 1, 2 ** 31 - 1, 2, 2, 1, 1, None, 0, ctypes.byref(n)) == INVALID and n.value == 0
    assert lib.yolo_tile_windows(2 ** 31 - 1, 1, 2 ** 30, 1, 0, 0, out.ctypes.data, 4, ctypes.byref(n)) == 0 and n.value == 2
    assert out[:2].tolist() == [[0, 0, 2 ** 30, 1], [2 ** 30 - 1, 0, 2 ** 30, 1]]


def test_entry_points_are_exported_and_bound():
    from yolo_tensorflow_amd import hip
    from yolo_tensorflow_amd.detector import _Detector
    lib = hip.load_library()
    for name in ("yolo_tile_windows", "yolo_detect_tiled_u8"):
        assert name in hip.EXPORTS and hasattr(lib, name), name
    assert callable(hip.Engine.detect_tiled) and callable(_Detector.detect_from_large_images)
    assert lib.yolo_detect_tiled_u8(None, None, 0, None, 0, 0, 0, 0, 0, 0, 0, 0.5, 0.5, 1, 0, 0, 0, None, None, 0) == INVALID      # no context: refused, no device touched


def test_window_record_layout_as_c_sees_it(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "yolo_hip.h"\n'
                   'int main(void) { printf("%u %u %u %u %u\\n", (unsigned)sizeof(yolo_tile_window), (unsigned)offsetof(yolo_tile_window, y0), '
                   '(unsigned)offsetof(yolo_tile_window, x0), (unsigned)offsetof(yolo_tile_window, h), (unsigned)offsetof(yolo_tile_window, w)); return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O0", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split() == ["16", "0", "4", "8", "12"]
