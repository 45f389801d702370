"""Ragged batches of native-size images, host side: the packing of the batch, the descriptor's layout as C sees it, the exported
entry points, and the u8 -> float step of the letterbox fit against darknet's loader expression.  No device call is made."""
import ctypes
import os
import subprocess
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ["yolo_forward_images_u8", "yolo_detect_images_u8", "yolo_detect_images_graph", "yolo_fit_unit_value", "yolo_darknet_boxes_at"]

# a C consumer of the header: the descriptor's size and field offsets, and darknet's `(float)data[i]/255.` (DN/image.c load_image_stb)
# for every byte value, as bit patterns
_C_PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "yolo_hip.h"
int main(void)
{
    int p;
    printf("%u %u %u %u\n", (unsigned)sizeof(yolo_image_desc), (unsigned)offsetof(yolo_image_desc, offset),
           (unsigned)offsetof(yolo_image_desc, h), (unsigned)offsetof(yolo_image_desc, w));
    printf("%d %d %d %d %d %d\n", YOLO_FIT_STRETCH, YOLO_FIT_LETTERBOX, YOLO_FIT_CV2, YOLO_FIT_CV2_BGR, YOLO_UNITS_NETWORK, YOLO_UNITS_SOURCE_PIXELS);
    for (p = 0; p < 256; ++p) {
        unsigned char data = (unsigned char)p;
        float v = (float)data/255.;
        unsigned bits;
        memcpy(&bits, &v, 4);
        printf("%u\n", bits);
    }
    return 0;
}
"""


def _probe(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(_C_PROBE)
    exe = str(tmp_path / "probe")
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-O0", "-I" + os.path.join(ROOT, "include"),
                         str(src), "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    return run.stdout.split("\n")


def test_pack_images_offsets_and_layout():
    from yolo_tensorflow_amd import hip
    rng = np.random.default_rng(0)
    shapes = [(1, 1), (3, 5), (1, 7), (9, 2), (4, 4)]
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    imgs[2] = np.asfortranarray(imgs[2])                     # any memory order in, C order packed
    buf, descs = hip.pack_images(imgs)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size == sum(h * w * 3 for h, w in shapes)
    assert descs.dtype == hip.DESC_DTYPE and descs.dtype.itemsize == 16 and len(descs) == len(shapes)
    off = 0
    for im, d, (h, w) in zip(imgs, descs, shapes):
        assert (int(d["offset"]), int(d["h"]), int(d["w"])) == (off, h, w)
        assert np.array_equal(buf[off:off + h * w * 3].reshape(h, w, 3), im)
        off += h * w * 3
    for bad in ([], [np.zeros((2, 2), np.uint8)], [np.zeros((2, 2, 3), np.float32)], [np.zeros((0, 2, 3), np.uint8)]):
        try:
            hip.pack_images(bad)
        except hip.YoloError:
            continue
        raise AssertionError("pack_images accepted %r" % (bad,))


def test_descriptor_layout_matches_the_header(tmp_path):
    from yolo_tensorflow_amd import hip
    out = _probe(tmp_path)
    size, o_off, o_h, o_w = (int(x) for x in out[0].split())
    assert size == 16 == ctypes.sizeof(hip.ImageDesc) == hip.DESC_DTYPE.itemsize
    assert (o_off, o_h, o_w) == (hip.ImageDesc.offset.offset, hip.ImageDesc.h.offset, hip.ImageDesc.w.offset) == (0, 8, 12)
    assert [hip.DESC_DTYPE.fields[k][1] for k in ("offset", "h", "w")] == [0, 8, 12]
    assert [int(x) for x in out[1].split()] == [hip.FIT_STRETCH, hip.FIT_LETTERBOX, hip.FIT_CV2, hip.FIT_CV2_BGR,
                                                hip.UNITS_NETWORK, hip.UNITS_SOURCE_PIXELS]


def test_new_entry_points_are_exported():
    from yolo_tensorflow_amd import hip
    lib = hip.load_library()
    for name in NEW_SYMBOLS:
        assert name in hip.EXPORTS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "yolo_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name


def test_letterbox_u8_to_float_is_darknets_for_all_256_values(tmp_path):
    """The letterbox fit reads a byte as darknet's loader stores it: (float)p/255., a double division rounded once to float.  The
    library's expression (host evaluation of what the kernel evaluates) against the same expression compiled as plain C."""
    from yolo_tensorflow_amd import hip
    want = np.array([int(x) for x in _probe(tmp_path)[2:258]], dtype=np.uint32).view(np.float32)
    got = np.array([hip.fit_unit_value(hip.FIT_LETTERBOX, p) for p in range(256)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(want, (np.arange(256, dtype=np.float64) / 255.).astype(np.float32))
    stretch = np.array([hip.fit_unit_value(hip.FIT_STRETCH, p) for p in range(256)], dtype=np.float32)
    assert np.array_equal(stretch, np.arange(256, dtype=np.float32) / np.float32(255))
    assert [hip.fit_unit_value(hip.FIT_CV2, p) for p in (0, 7, 255)] == [0.0, 7.0, 255.0]
    assert np.isnan(hip.fit_unit_value(9, 0)) and np.isnan(hip.fit_unit_value(hip.FIT_STRETCH, 256))
