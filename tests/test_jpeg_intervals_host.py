"""The entropy stage over restart intervals, host side: the interval scan (yolo_jpeg_intervals) on every fixture and photograph, the library's
exports, and tests/c/jpeg_intervals.cpp -- the interval decoder the device runs per lane, built for the host under the sanitizers and held to the host decoder on every
prefix and 2000 corruptions of each of the 36 fixtures with a restart interval.  No GPU."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from yolo_tensorflow_amd import hip
import test_jpeg_host as JH

# restart interval in MCUs and the number of intervals of the photographs of tests/golden/images (giraffe has no DRI segment)
PHOTOS = {"dog": (96, 36), "eagle": (97, 32), "horses": (97, 32), "person": (80, 27), "kite": (169, 113)}
EXPORTS = ["yolo_set_jpeg_entropy", "yolo_jpeg_entropy", "yolo_jpeg_entropy_times", "yolo_jpeg_intervals", "yolo_op_jpeg_entropy"]


def _names():
    return JH.cases()[1]


def dri_fixtures():
    return [n for n in _names() if JH.name_geometry(n)[3]]


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _check_intervals(data, iv, mcus, restart):
    assert iv.shape == (-(-mcus // restart), 2) and iv.dtype == np.uint32
    for i, (b, e) in enumerate(iv):
        b, e = int(b), int(e)
        assert b <= e <= len(data)
        if i:          # every begin follows an RSTm, and the interval before it ends at that marker (or at the fill bytes in front of it)
            assert data[b - 2] == 0xFF and 0xD0 <= data[b - 1] <= 0xD7, i
            assert int(iv[i - 1, 1]) <= b - 2 and set(data[int(iv[i - 1, 1]):b - 2]) <= {0xFF}
        # inside an interval every 0xFF is a stuffed one; at its end stands a marker or the file's end
        body = data[b:e]
        assert all(body[k + 1] == 0 for k in range(len(body) - 1) if body[k] == 0xFF) and (not body or body[-1] != 0xFF)
        assert e == len(data) or (data[e] == 0xFF and (e + 1 == len(data) or data[e + 1] != 0))


def test_exports_exist_in_the_library():
    lib = C.CDLL(os.path.join(JH.ROOT, "yolo_tensorflow_amd", "libyolo_hip.so"))
    for name in EXPORTS:
        assert hasattr(lib, name), name
        assert name in hip.EXPORTS
    assert (hip.JPEG_ENTROPY_HOST, hip.JPEG_ENTROPY_AUTO) == (0, 1)


def test_interval_count_and_marker_positions_on_every_dri_fixture():
    names = dri_fixtures()
    assert len(names) == 36 and sum(JH.name_geometry(n)[3] == 1 for n in names) == 32 and sum(JH.name_geometry(n)[3] == 3 for n in names) == 4
    for name in names:
        data = _read(JH.path_of(name))
        info = hip.jpeg_info(data)
        restart = JH.name_geometry(name)[3]
        assert info["restart_interval"] == restart
        iv = hip.jpeg_intervals(data)
        _check_intervals(data, iv, info["mcus"][0] * info["mcus"][1], restart)
        assert int(iv[0, 0]) > 0 and data[int(iv[-1, 1]):int(iv[-1, 1]) + 2] == b"\xff\xd9", name          # from the scan header to EOI


def test_interval_count_on_the_photographs():
    for photo, (restart, count) in PHOTOS.items():
        data = _read(os.path.join(JH.IMAGES, photo + ".jpg"))
        info = hip.jpeg_info(data)
        assert info["restart_interval"] == restart == info["mcus"][0], photo          # one MCU row
        iv = hip.jpeg_intervals(data)
        assert len(iv) == count == info["mcus"][1]
        _check_intervals(data, iv, info["mcus"][0] * info["mcus"][1], restart)
    giraffe = _read(os.path.join(JH.IMAGES, "giraffe.jpg"))
    assert hip.jpeg_info(giraffe)["restart_interval"] == 0 and hip.jpeg_intervals(giraffe).shape == (0, 2)


def test_files_without_dri_are_not_eligible():
    every = sorted(f[:-4] for f in os.listdir(JH.JPEG) if f.endswith(".jpg"))
    plain = [n for n in every if n not in dri_fixtures()]
    assert len(every) == 107 and len(plain) == 71
    for name in plain:
        if name.startswith("refused_"):          # a kind whose headers are refused: the scan passes that refusal on
            with pytest.raises(hip.YoloError, match=r"\(-6\)"):
                hip.jpeg_intervals(JH.path_of(name))
            continue
        assert hip.jpeg_info(JH.path_of(name))["restart_interval"] == 0
        assert hip.jpeg_intervals(JH.path_of(name)).shape == (0, 2), name


def test_a_marker_missing_or_out_of_place_makes_a_file_not_eligible():
    data = bytearray(_read(JH.path_of("c50x35_444_rst1")))
    iv = hip.jpeg_intervals(bytes(data))
    assert len(iv) == 35
    at = int(iv[10, 1])          # the marker behind interval 10
    assert data[at] == 0xFF and 0xD0 <= data[at + 1] <= 0xD7
    assert len(hip.jpeg_intervals(bytes(data[:at] + data[at + 2:]))) == 0                  # deleted: one marker too few
    assert len(hip.jpeg_intervals(bytes(data[:at] + b"\xff\xd9" + data[at + 2:]))) == 0    # EOI in its place
    assert len(hip.jpeg_intervals(bytes(data[:at] + b"\xff" + data[at:]))) == 35           # a fill byte in front of it: skipped
    junk = hip.jpeg_intervals(bytes(data[:at] + b"\x5a" + data[at:]))                      # a data byte in front of it: part of interval 10
    assert len(junk) == 35 and int(junk[10, 1]) == at + 1
    last = int(iv[-1, 1])
    assert len(hip.jpeg_intervals(bytes(data[:last] + b"\xff\xd3" + data[last:]))) == 0    # one marker too many
    with pytest.raises(hip.YoloError, match=r"\(-1\).*not a JPEG"):
        hip.jpeg_intervals(b"not a jpeg at all")


def test_interval_decoder_sanitizer_run(tmp_path):
    """tests/c/jpeg_intervals.cpp built with yolo_jpeg.cpp under -fsanitize=address,undefined and run as a child process over the 36 fixtures with a restart
    interval: the contract of DESIGN.md 3.25 on every input, no sanitizer report"""
    exe = str(tmp_path / "jpeg_intervals")
    build = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + JH.ROOT,
                            os.path.join(JH.ROOT, "tests", "c", "jpeg_intervals.cpp"), os.path.join(JH.ROOT, "yolo_tensorflow_amd", "csrc", "yolo_jpeg.cpp"),
                            "-pthread", "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    names = dri_fixtures()
    run = subprocess.run([exe] + [JH.path_of(n) for n in names], capture_output=True, text=True, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr
    m = re.match(r"^not_eligible (\d+) clean (\d+) handed_back (\d+) host_refused (\d+)$", run.stdout.strip())
    assert m, run.stdout
    not_eligible, clean, handed_back, host_refused = (int(v) for v in m.groups())
    assert not_eligible + clean + handed_back == sum(os.path.getsize(JH.path_of(n)) + 2001 for n in names)
    # every intact file is clean; the corruptions reach both other outcomes; whatever the host refuses was handed back to it
    assert clean >= len(names) and not_eligible > 1000 and handed_back >= host_refused > 1000
