"""Classifiers and segmenters over decoded video frames and JPEG files, host side: the six entry points are declared, exported and
bound, the Python wrappers carry the stated signatures, and yolo_view_table is what it was.  No GPU.  tests/test_gpu_classify_frames.py holds the
device to the image path over the restated RGB."""
import inspect
import os
import re
from yolo_tensorflow_amd import hip
from yolo_tensorflow_amd.classifier import Classifier
from yolo_tensorflow_amd.segmenter import Segmenter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("yolo_classify_frames_u8", "yolo_classify_views_frames_u8", "yolo_segment_frames_u8", "yolo_classify_jpegs", "yolo_classify_views_jpegs", "yolo_segment_jpegs")


def _signature(fn):
    """[(name, default or inspect.Parameter.empty)] without self"""
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values() if p.name != "self"]


def test_the_six_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "yolo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(yolo_[a-z0-9_]+)\s*\(", text))
    lib = hip.load_library()
    for name in NEW:
        assert name in declared and name in hip.EXPORTS and hasattr(lib, name), name
    # the frame forms follow their image forms argument for argument, yolo_frame_desc in the place of yolo_image_desc
    protos = {m.group(1): re.sub(r"\s+", " ", m.group(2)) for m in re.finditer(r"\bint (yolo_[a-z0-9_]+)\s*\(([^)]*)\)", text)}
    for frame_form, image_form in (("yolo_classify_frames_u8", "yolo_classify_images_u8"), ("yolo_classify_views_frames_u8", "yolo_classify_views_u8")):
        assert protos[frame_form] == protos[image_form].replace("yolo_image_desc", "yolo_frame_desc"), frame_form
        assert getattr(lib, frame_form).argtypes == getattr(lib, image_form).argtypes
    assert protos["yolo_segment_frames_u8"] == ("yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc, float thresh, "
                                                "uint8_t *labels_u8, const uint64_t *label_offsets")
    # the JPEG forms: (files, bytes, n) for (pixels, bytes, descs, n), no loc
    assert protos["yolo_classify_jpegs"] == "yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, int fit, int top_k, int32_t *classes_out, float *probs_out, int out_loc"
    assert protos["yolo_classify_views_jpegs"] == ("yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n_images, int views, int fit, int shift, float scale, "
                                                   "int top_k, int32_t *classes_out, float *probs_out, int out_loc")
    assert protos["yolo_segment_jpegs"] == ("yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, int fit, float thresh, uint8_t *labels_u8, "
                                            "const uint64_t *label_offsets")
    assert len(lib.yolo_segment_frames_u8.argtypes) == 10 and len(lib.yolo_classify_jpegs.argtypes) == 9
    assert len(lib.yolo_classify_views_jpegs.argtypes) == 12 and len(lib.yolo_segment_jpegs.argtypes) == 8


def test_the_python_wrappers_have_the_stated_signatures():
    E, empty = hip.Engine, inspect.Parameter.empty
    assert _signature(E.classify_frames) == [("frames", empty), ("fit", hip.FIT_STRETCH), ("top_k", 5)]
    assert _signature(E.classify_views_frames) == [("frames", empty), ("views", empty), ("fit", hip.FIT_STRETCH), ("shift", 32), ("scale", 1.0), ("top_k", 0)]
    assert _signature(E.segment_frames) == [("frames", empty), ("fit", hip.FIT_LETTERBOX), ("thresh", 0.5)]
    assert _signature(E.classify_jpegs) == [("files", empty), ("fit", hip.FIT_STRETCH), ("top_k", 5)]
    assert _signature(E.classify_views_jpegs) == [("files", empty), ("views", empty), ("fit", hip.FIT_STRETCH), ("shift", 32), ("scale", 1.0), ("top_k", 0)]
    assert _signature(E.segment_jpegs) == [("files", empty), ("fit", hip.FIT_LETTERBOX), ("thresh", 0.5)]
    # the frame forms take what their image forms take
    assert _signature(E.classify_frames)[1:] == _signature(E.classify_images)[1:]
    assert _signature(E.classify_views_frames)[1:] == _signature(E.classify_views)[1:]
    assert _signature(E.segment_frames)[1:] == _signature(E.segment_images)[1:]
    for fn, first in ((Classifier.classify_from_files, "paths"), (Classifier.classify_from_frames, "frames")):
        assert _signature(fn) == [(first, empty), ("top", 5), ("views", None), ("shift", 32)]
        assert _signature(fn)[1:] == _signature(Classifier.classify_from_images)[1:]
    assert _signature(Segmenter.segment_from_files) == [("paths", empty), ("thresh", 0.5)]
    assert _signature(Segmenter.segment_from_frames) == [("frames", empty), ("thresh", 0.5)]


def test_view_table_is_unchanged():
    assert [tuple(int(x) for x in v) for v in hip.view_table(hip.VIEWS_FLIP)] == [(0, 0, 0, 0), (0, 0, 1, 0)]
    for s in (0, 5, 32):
        want = [(-s, -s, 0, 0), (-s, s, 0, 0), (0, 0, 0, 0), (s, -s, 0, 0), (s, s, 0, 0)]
        want = want + [(dy, dx, 1, 0) for dy, dx, _, _ in want]
        assert [tuple(int(x) for x in v) for v in hip.view_table(hip.VIEWS_TEN_CROP, s)] == want, s
    assert hip.VIEW_DTYPE.itemsize == 16 and (hip.VIEWS_FLIP, hip.VIEWS_TEN_CROP) == (1, 2)
