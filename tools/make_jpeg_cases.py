#!/usr/bin/env python3
"""Writes the JPEG fixtures (tests/golden/jpeg/*.jpg) and what the compiled reference decodes them to (tests/golden/jpeg_cases.npz).

    python tools/make_jpeg_cases.py

The pictures are crops of tests/golden/images/dog.jpg with seeded noise added (in int, clipped), so that chroma edges matter, written by
PIL in every kind of file the library serves -- and two kinds it refuses.  The expected bytes come from the reference itself:
load_image(path, 0, 0, 3) of oracle/_ref/libdarknet_ref.so, times 255 (exact: the loader divides the byte by 255. in double).  This tool
reads the compiled reference; the tests read only what it wrote.  For the six photographs of tests/golden/images the file keeps the
sha-256 of the reference's decoded bytes, not the bytes.
"""
import ctypes as C
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")
NPZ = os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")
IMAGES = os.path.join(ROOT, "tests", "golden", "images")
REF = os.path.join(ROOT, "oracle", "_ref", "libdarknet_ref.so")

SIZES = [(1, 1), (2, 2), (7, 5), (8, 8), (16, 16), (17, 9), (33, 31), (50, 35)]          # (w, h)
SUBSAMPLING = {"444": 0, "422": 1, "420": 2}
VARIANTS = {"std": {}, "opt": {"optimize": True}, "rst1": {"restart_marker_blocks": 1}}
GREY = [(1, 1), (23, 19), (32, 8)]
PHOTOS = ["dog", "eagle", "giraffe", "horses", "kite", "person"]


class RefImage(C.Structure):
    _fields_ = [("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("data", C.POINTER(C.c_float))]


def reference():
    lib = C.CDLL(REF)
    lib.load_image.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_int]
    lib.load_image.restype = RefImage
    lib.free_image.argtypes = [RefImage]
    lib.free_image.restype = None
    return lib


def ref_decode(lib, path):
    """the reference's image of a file as uint8 [h, w, 3]"""
    im = lib.load_image(path.encode(), 0, 0, 3)
    chw = np.ctypeslib.as_array(im.data, shape=(im.c, im.h, im.w)).astype(np.float64) * 255.0
    out = np.rint(chw).astype(np.uint8)
    if not np.array_equal(out.astype(np.float64), chw.round(3)):
        raise SystemExit("%s: the reference's floats are not bytes / 255" % path)
    lib.free_image(im)
    return np.ascontiguousarray(out.transpose(1, 2, 0))


def picture(dog, rng, w, h, i):
    """a w x h crop of the dog photograph around its coloured parts, with noise of +-24 levels"""
    y0 = 120 + (37 * i) % 200
    x0 = 130 + (53 * i) % 300
    crop = dog[y0:y0 + h, x0:x0 + w].astype(np.int32)
    return np.clip(crop + rng.integers(-24, 25, crop.shape), 0, 255).astype(np.uint8)


def as_440(data):
    """A 4:2:2 file of W x H -> a 4:4:0 file of H x W (luma sampled 1 x 2: what four of the six photographs are, and what PIL cannot write).  Both
    kinds code four blocks per MCU -- Y, Y, Cb, Cr -- and a W x H 4:2:2 frame has as many MCUs as an H x W 4:4:0 one, so swapping the two sizes and
    the luma sampling factors in the frame header leaves a valid file.  Its picture is the original's blocks rearranged; it is a picture all the same,
    and the reference's decode of it is the fixture."""
    at = data.index(b"\xff\xc0")
    head = bytearray(data[at:at + 19])
    if head[9] != 3 or head[11] != 0x21:
        raise SystemExit("as_440: not a 3-component 4:2:2 baseline file")
    head[5:7], head[7:9] = data[at + 7:at + 9], data[at + 5:at + 7]
    head[11] = 0x12
    return data[:at] + bytes(head) + data[at + 19:]


def main():
    if not os.path.exists(REF):
        raise SystemExit("%s is missing: build the reference first (make -C oracle)" % REF)
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(23)
    dog = np.asarray(Image.open(os.path.join(IMAGES, "dog.jpg")).convert("RGB"))
    files = []
    i = 0
    for w, h in SIZES:
        for sub, code in SUBSAMPLING.items():
            for var, kw in VARIANTS.items():
                name = "c%dx%d_%s_%s" % (w, h, sub, var)
                Image.fromarray(picture(dog, rng, w, h, i)).save(os.path.join(OUT, name + ".jpg"), quality=85, subsampling=code, **kw)
                files.append(name)
                i += 1
    for sub, code in SUBSAMPLING.items():
        name = "c50x35_%s_rst3" % sub
        Image.fromarray(picture(dog, rng, 50, 35, i)).save(os.path.join(OUT, name + ".jpg"), quality=85, subsampling=code, restart_marker_blocks=3)
        files.append(name)
        i += 1
    for w, h in SIZES:
        for var, kw in list(VARIANTS.items()) + ([("rst3", {"restart_marker_blocks": 3})] if (w, h) == (50, 35) else []):
            name = "c%dx%d_440_%s" % (w, h, var)
            buf = io.BytesIO()
            Image.fromarray(picture(dog, rng, h, w, i)).save(buf, "JPEG", quality=85, subsampling=1, **kw)
            with open(os.path.join(OUT, name + ".jpg"), "wb") as fh:
                fh.write(as_440(buf.getvalue()))
            files.append(name)
            i += 1
    for name, q, code in (("c50x35_420_q10", 10, 2), ("c33x31_422_q100", 100, 1)):
        w, h = (50, 35) if "50x35" in name else (33, 31)
        Image.fromarray(picture(dog, rng, w, h, i)).save(os.path.join(OUT, name + ".jpg"), quality=q, subsampling=code)
        files.append(name)
        i += 1
    for w, h in GREY:
        name = "g%dx%d" % (w, h)
        Image.fromarray(picture(dog, rng, w, h, i)).convert("L").save(os.path.join(OUT, name + ".jpg"), quality=85)
        files.append(name)
        i += 1
    refused = ["refused_progressive", "refused_cmyk"]
    Image.fromarray(picture(dog, rng, 33, 31, i)).save(os.path.join(OUT, refused[0] + ".jpg"), quality=85, progressive=True)
    Image.fromarray(picture(dog, rng, 17, 9, i + 1)).convert("CMYK").save(os.path.join(OUT, refused[1] + ".jpg"), quality=85)

    lib = reference()
    out = {"names": np.array(files), "refused": np.array(refused), "photos": np.array(PHOTOS)}
    for name in files:
        path = os.path.join(OUT, name + ".jpg")
        if os.path.getsize(path) > 64 * 1024:
            raise SystemExit("%s: %d bytes, too large for a fixture" % (path, os.path.getsize(path)))
        out["rgb/" + name] = ref_decode(lib, path)
    sha, shape = [], []
    for name in PHOTOS:
        rgb = ref_decode(lib, os.path.join(IMAGES, name + ".jpg"))
        sha.append(hashlib.sha256(rgb.tobytes()).hexdigest())
        shape.append(rgb.shape[:2])
    out["photo_sha256"] = np.array(sha)
    out["photo_hw"] = np.array(shape, dtype=np.int32)
    np.savez_compressed(NPZ, **out)
    total = sum(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT))
    print("%d served + %d refused fixtures, %d bytes in %s; %s: %d bytes" % (len(files), len(refused), total, OUT, NPZ, os.path.getsize(NPZ)))


if __name__ == "__main__":
    sys.exit(main())
