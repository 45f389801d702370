"""ctypes shim over libyolo_hip.so (the C ABI in include/yolo_hip.h).

This is the only module that talks to the device.  It replaces the reference's `tf.Session.run`
boundary (V3/YOLO_V3_inference.py:106-107) and plays the role D2T/darknet.py:48-115 plays for
libdarknet.so.  There is deliberately **no CPU fallback**: if the library is missing or no HIP
device is visible every entry point raises.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# YOLO_HIP_LIB: another build of the SAME library (A/B probes, tools/probe/ab) -- selected, never copied over the in-tree file, whose
# sources buildinfo.source_hash() stamps the profiles with; a line measured through it says so (bench.py: "lib_override")
LIB_OVERRIDE = os.environ.get("YOLO_HIP_LIB") or None
LIB_PATH = LIB_OVERRIDE or os.path.join(_HERE, "libyolo_hip.so")

BF16, FP32, FP8, FP16, FP16X2 = 0, 1, 2, 3, 4
SEM_TF, SEM_DARKNET = 0, 1
DECODE_RATIO, DECODE_PIXEL = 0, 1
HOST, DEVICE = 0, 1
IMG_U8, IMG_F32, IMG_F32_CHW = 0, 1, 2
NMS_TF, NMS_PER_CLASS, NMS_DARKNET, NMS_NUMPY_V3, NMS_TF_V1 = 0, 1, 2, 3, 4
SELECT_GT, SELECT_GE = 0, 1
FIT_STRETCH, FIT_LETTERBOX, FIT_CV2, FIT_CV2_BGR, FIT_CENTER_CROP = 0, 1, 2, 3, 4
UNITS_NETWORK, UNITS_SOURCE_PIXELS = 0, 1
VIEWS_FLIP, VIEWS_TEN_CROP = 1, 2
PIX_NV12, PIX_I420, PIX_RGB24, PIX_BGR24 = 0, 1, 2, 3
PIX_JPEG_GREY, PIX_JPEG_444, PIX_JPEG_422, PIX_JPEG_420, PIX_JPEG_440 = 16, 17, 18, 19, 20      # the component planes of a decoded JPEG file
MATRIX_BT601, MATRIX_BT709, MATRIX_BT601_FULL = 0, 1, 2

BOX_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("x1", "<f4"), ("y1", "<f4"), ("score", "<f4"), ("cls", "<i4")])
# yolo_image_desc: one image of a ragged batch, a uint8 RGB [h][w][3] image at byte `offset` of one packed buffer
DESC_DTYPE = np.dtype([("offset", "<u8"), ("h", "<i4"), ("w", "<i4")])
# yolo_frame_desc: one decoded video frame, every plane at its own byte offset of one packed buffer and its own row pitch
FRAME_DTYPE = np.dtype([("offset", "<u8", (3,)), ("pitch", "<u8", (3,)), ("h", "<i4"), ("w", "<i4"), ("format", "<i4"), ("matrix", "<i4")])
# yolo_view: one view of multi-view classification, the crop offsets in pixels and whether the image is mirrored
VIEW_DTYPE = np.dtype([("dy", "<i4"), ("dx", "<i4"), ("flip", "<i4"), ("pad", "<i4")])


class ImageDesc(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("h", C.c_int32), ("w", C.c_int32)]

EXPORTS = [
    "yolo_create", "yolo_destroy", "yolo_last_error", "yolo_load_darknet_weights", "yolo_set_weights",
    "yolo_weights_count", "yolo_set_act_scales", "yolo_export", "yolo_create_from_file", "yolo_input_size", "yolo_num_rows", "yolo_num_attrs", "yolo_num_layers", "yolo_head_geometry", "yolo_head_geometry_hw", "yolo_op_decode_hw", "yolo_op_resize_u8_hw",
    "yolo_conv_flops", "yolo_conv_bytes", "yolo_forward", "yolo_forward_image_u8", "yolo_postprocess",
    "yolo_detect", "yolo_detect_graph", "yolo_synchronize", "yolo_layer_output", "yolo_staged_input", "yolo_time_forward", "yolo_time_layers",
    "yolo_autotune", "yolo_get_tile_configs", "yolo_set_tile_configs", "yolo_resolved_tile_configs", "yolo_op_conv2d", "yolo_op_conv_num_cfgs", "yolo_op_upsample2x", "yolo_op_reorg",
    "yolo_darknet_boxes", "yolo_last_layer_size", "yolo_last_layer_output", "yolo_op_letterbox",
    "yolo_op_maxpool", "yolo_op_resize_u8", "yolo_op_detections_boxes", "yolo_op_nms_detections", "yolo_forward_letterbox_chw", "yolo_op_decode", "yolo_op_postprocess",
    "yolo_postprocess_rows", "yolo_op_postprocess_rows", "yolo_last_layer_output_batch", "yolo_head_raw", "yolo_calibrate", "yolo_calibrate_copy", "yolo_op_resize_cv2",
    "yolo_forward_images_u8", "yolo_detect_images_u8", "yolo_detect_images_graph", "yolo_fit_unit_value", "yolo_darknet_boxes_at",
    "yolo_num_classes", "yolo_classify", "yolo_classify_images_u8", "yolo_op_avgpool", "yolo_op_softmax",
    "yolo_set_hier_thresh", "yolo_set_hierarchy_mode", "yolo_darknet_boxes_map", "yolo_tree_geometry", "yolo_tree_read", "yolo_plan_check", "yolo_plan_table", "yolo_plan_dump",
    "yolo_op_tree_softmax", "yolo_op_tree_top", "yolo_activation_code", "yolo_op_activate", "yolo_op_shortcut",
    "yolo_output_map_geometry", "yolo_output_map", "yolo_label_map", "yolo_segment_images_u8", "yolo_op_deconv2d", "yolo_op_l2norm", "yolo_op_upsample", "yolo_op_label_map",
    "yolo_op_conv2d_grouped", "yolo_op_conv2d_xnor", "yolo_op_conv2d_pad", "yolo_op_lrn",
    "yolo_num_state_tensors", "yolo_state_geometry", "yolo_get_state", "yolo_set_state", "yolo_reset_state",
    "yolo_tile_windows", "yolo_detect_tiled_u8",
    "yolo_vector_inputs", "yolo_forward_vectors", "yolo_sequence", "yolo_set_temperature", "yolo_reset_temperature", "yolo_op_sample",
    "yolo_set_frame_average", "yolo_frame_average",
    "yolo_view_table", "yolo_classify_views_u8", "yolo_op_view_reduce",
    "yolo_frame_to_rgb_host", "yolo_op_frame_to_rgb", "yolo_forward_frames_u8", "yolo_detect_frames_u8", "yolo_detect_frames_graph", "yolo_detect_tiled_frames_u8",
    "yolo_jpeg_info", "yolo_jpeg_coefficients", "yolo_jpeg_to_rgb_host", "yolo_op_jpeg_to_rgb", "yolo_decode_jpegs", "yolo_jpeg_decode_times", "yolo_forward_jpegs", "yolo_detect_jpegs", "yolo_detect_tiled_jpegs",
    "yolo_classify_frames_u8", "yolo_classify_views_frames_u8", "yolo_segment_frames_u8", "yolo_classify_jpegs", "yolo_classify_views_jpegs", "yolo_segment_jpegs",
    "yolo_set_jpeg_entropy", "yolo_jpeg_entropy", "yolo_jpeg_entropy_times", "yolo_jpeg_intervals", "yolo_op_jpeg_entropy",
]
HIER_CONDITIONAL, HIER_ABSOLUTE, HIER_LEAVES = 0, 1, 2
_HIER_MODES = {None: HIER_CONDITIONAL, "conditional": HIER_CONDITIONAL, "absolute": HIER_ABSOLUTE, "leaves": HIER_LEAVES}
# include/yolo_dist.h: the image-sharded detect step
DIST_EXPORTS = ["yolo_shard_bounds", "yolo_dist_flat_words", "yolo_dist_split_records", "yolo_dist_unique_id", "yolo_dist_create",
                "yolo_dist_detect", "yolo_dist_detect_async", "yolo_dist_destroy"]


class YoloError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cfg_text", C.c_char_p), ("max_batch", C.c_int32),
                ("dtype", C.c_int32), ("semantics", C.c_int32), ("decode", C.c_int32), ("device", C.c_int32),
                ("keep_layers", C.c_int32), ("stream", C.c_void_p)]


_lib = None


def load_library():
    """dlopen libyolo_hip.so and declare every prototype; raises YoloError when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YoloError("%s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(or `make -C yolo_tensorflow_amd/csrc`); there is no CPU fallback" % LIB_PATH)
    l = C.CDLL(LIB_PATH)
    P, I, F, D = C.c_void_p, C.c_int, C.c_float, C.c_double
    FP = C.POINTER(C.c_float)
    l.yolo_create.argtypes = [C.POINTER(_Config), C.c_char_p, C.c_size_t]; l.yolo_create.restype = P
    l.yolo_destroy.argtypes = [P]; l.yolo_destroy.restype = None
    l.yolo_last_error.argtypes = [P]; l.yolo_last_error.restype = C.c_char_p
    l.yolo_load_darknet_weights.argtypes = [P, C.c_char_p, I]
    l.yolo_set_weights.argtypes = [P, FP, C.c_size_t]
    l.yolo_weights_count.argtypes = [P]; l.yolo_weights_count.restype = C.c_size_t
    l.yolo_set_act_scales.argtypes = [P, P, I]
    l.yolo_head_geometry.argtypes = [P, I, P, P, P, P]
    l.yolo_head_geometry_hw.argtypes = [P, I, P, P, P, P, P]
    l.yolo_export.argtypes = [P, C.c_char_p]
    l.yolo_create_from_file.argtypes = [C.c_char_p, I, I, P, I, C.c_char_p, C.c_size_t]; l.yolo_create_from_file.restype = P
    l.yolo_input_size.argtypes = [P, C.POINTER(I), C.POINTER(I), C.POINTER(I)]
    for n in ("yolo_num_rows", "yolo_num_attrs", "yolo_num_layers", "yolo_synchronize", "yolo_num_classes"):
        getattr(l, n).argtypes = [P]
    l.yolo_conv_flops.argtypes = [P]; l.yolo_conv_flops.restype = D
    l.yolo_conv_bytes.argtypes = [P, I]; l.yolo_conv_bytes.restype = D
    l.yolo_forward.argtypes = [P, P, I, I, I, F, P, I]
    l.yolo_forward_image_u8.argtypes = [P, P, I, I, I, P, I]
    l.yolo_postprocess.argtypes = [P, I, F, F, I, I, I, P, P, I]
    l.yolo_detect.argtypes = [P, P, I, I, I, F, F, F, I, I, I, P, P, I]
    l.yolo_detect_graph.argtypes = [P, P, I, I, F, F, F, I, I, I, P, P]
    l.yolo_layer_output.argtypes = [P, I, I, P, C.c_size_t, C.POINTER(I)]
    l.yolo_staged_input.argtypes = [P, I, P, C.c_size_t, C.POINTER(I)]
    l.yolo_time_forward.argtypes = [P, I, I, FP, FP]
    l.yolo_time_layers.argtypes = [P, I, I, FP]
    l.yolo_autotune.argtypes = [P, I, I]
    l.yolo_get_tile_configs.argtypes = [P, P]
    l.yolo_set_tile_configs.argtypes = [P, P]
    l.yolo_resolved_tile_configs.argtypes = [P, I, P]
    l.yolo_op_conv2d.argtypes = [P, I, I, I, I, P, P, I, I, I, I, P, P, I, I, I]
    l.yolo_op_conv2d_pad.argtypes = [P, I, I, I, I, P, P, I, I, I, I, I, P, P, I, I, I]
    l.yolo_op_conv_num_cfgs.argtypes = []
    l.yolo_op_upsample2x.argtypes = [P, I, I, I, I, I, P, I]
    l.yolo_op_reorg.argtypes = [P, I, I, I, I, I, I, P, I]
    l.yolo_op_maxpool.argtypes = [P, I, I, I, I, I, I, P, I]
    l.yolo_op_resize_u8.argtypes = [P, I, I, I, F, P, I]
    l.yolo_op_resize_u8_hw.argtypes = [P, I, I, I, I, F, P, I]
    l.yolo_op_detections_boxes.argtypes = [P, I, I, I, P, I]
    l.yolo_op_nms_detections.argtypes = [P, P, P, I, I, F, I, I]
    l.yolo_forward_letterbox_chw.argtypes = [P, P, I, I, I, P, I]
    l.yolo_op_decode.argtypes = [P, I, I, I, I, P, I, I, I, P, I]
    l.yolo_op_decode_hw.argtypes = [P, I, I, I, I, I, P, I, I, I, I, P, I]
    l.yolo_darknet_boxes.argtypes = [P, I, I, F, I, P, I, P]
    l.yolo_last_layer_size.argtypes = [P]; l.yolo_last_layer_size.restype = C.c_size_t
    l.yolo_last_layer_output.argtypes = [P, P, C.c_size_t]
    l.yolo_op_letterbox.argtypes = [P, I, I, I, I, I, P, I]
    l.yolo_op_postprocess.argtypes = [P, I, I, I, F, F, I, I, I, P, P, I]
    l.yolo_op_postprocess_rows.argtypes = [P, I, I, I, F, F, I, I, I, P, P, P, I]
    l.yolo_postprocess_rows.argtypes = [P, I, F, F, I, I, I, P, P, P, I]
    l.yolo_last_layer_output_batch.argtypes = [P, I, P, C.c_size_t]
    l.yolo_head_raw.argtypes = [P, I, I, P, C.c_size_t]
    l.yolo_calibrate.argtypes = [I, P, I, C.c_double, FP, FP]
    l.yolo_calibrate_copy.argtypes = [I, P, C.c_double, FP]
    l.yolo_op_resize_cv2.argtypes = [P, I, I, I, I, I, F, P, I]
    SZ = C.c_size_t
    l.yolo_forward_images_u8.argtypes = [P, P, SZ, P, I, I, I, P, I]
    l.yolo_detect_images_u8.argtypes = [P, P, SZ, P, I, I, I, F, F, I, I, I, I, P, P, I]
    l.yolo_detect_images_graph.argtypes = [P, P, SZ, P, I, I, F, F, I, I, I, I, P, P]
    l.yolo_fit_unit_value.argtypes = [I, I]; l.yolo_fit_unit_value.restype = F
    l.yolo_darknet_boxes_at.argtypes = [P, I, I, I, F, I, P, I, P]
    l.yolo_classify.argtypes = [P, P, I, I, I, F, I, P, P, I]
    l.yolo_classify_images_u8.argtypes = [P, P, SZ, P, I, I, I, I, P, P, I]
    l.yolo_op_avgpool.argtypes = [P, I, I, I, I, I, P, I]
    l.yolo_op_softmax.argtypes = [P, I, I, I, F, I, P, P, P, I]
    l.yolo_set_hier_thresh.argtypes = [P, F]
    l.yolo_set_hierarchy_mode.argtypes = [P, I]
    l.yolo_darknet_boxes_map.argtypes = [P, I, I, I, F, I, P, P, I, P]
    l.yolo_tree_geometry.argtypes = [P, P, P, P, P, P, P, P]
    l.yolo_tree_read.argtypes = [C.c_char_p, P, P, P, P, P, P, P, C.c_char_p, SZ]
    l.yolo_plan_check.argtypes = [C.c_char_p, I, C.c_char_p, SZ]
    l.yolo_plan_table.argtypes = [C.c_char_p, I, I, I, C.c_char_p, SZ, C.c_char_p, SZ]
    l.yolo_plan_dump.argtypes = [C.c_char_p, I, I, I, C.c_char_p, SZ, C.c_char_p, SZ]
    l.yolo_op_tree_softmax.argtypes = [P, I, I, C.c_char_p, F, I, P, I]
    l.yolo_op_tree_top.argtypes = [P, I, C.c_char_p, F, P, I]
    l.yolo_activation_code.argtypes = [C.c_char_p]
    l.yolo_op_activate.argtypes = [P, I, I, I, I, I, I, P, I]
    l.yolo_op_shortcut.argtypes = [P, I, I, I, I, P, I, I, I, I, I, P, I]
    l.yolo_output_map_geometry.argtypes = [P, C.POINTER(I), C.POINTER(I), C.POINTER(I)]
    l.yolo_output_map.argtypes = [P, I, P, SZ]
    l.yolo_label_map.argtypes = [P, I, F, P]
    l.yolo_segment_images_u8.argtypes = [P, P, P, I, I, F, P, P]
    l.yolo_op_deconv2d.argtypes = [P, I, I, I, I, P, P, I, I, I, I, I, I, I, P, I]
    l.yolo_op_conv2d_grouped.argtypes = [P, I, I, I, I, P, P, I, I, I, I, I, I, I, I, P, I]
    l.yolo_op_conv2d_xnor.argtypes = [P, I, I, I, I, P, P, I, I, I, I, I, I, I, P, I]
    l.yolo_op_l2norm.argtypes = [P, I, I, I, I, I, P, I]
    l.yolo_op_lrn.argtypes = [P, I, I, I, I, I, C.c_float, C.c_float, C.c_float, I, P, I]
    l.yolo_op_upsample.argtypes = [P, I, I, I, I, I, F, I, P, I]
    l.yolo_op_label_map.argtypes = [P, I, I, I, I, F, P, I]
    l.yolo_num_state_tensors.argtypes = [P]
    l.yolo_state_geometry.argtypes = [P, I, C.POINTER(I), C.POINTER(SZ)]
    l.yolo_get_state.argtypes = [P, I, I, P, SZ]
    l.yolo_set_state.argtypes = [P, I, I, P, SZ]
    l.yolo_reset_state.argtypes = [P, I]
    l.yolo_set_frame_average.argtypes = [P, I]
    l.yolo_frame_average.argtypes = [P]
    l.yolo_tile_windows.argtypes = [I, I, I, I, I, I, P, I, C.POINTER(I)]
    l.yolo_detect_tiled_u8.argtypes = [P, P, SZ, P, I, I, I, I, I, I, I, F, F, I, I, I, I, P, P, I]
    l.yolo_view_table.argtypes = [I, I, P, I, C.POINTER(I)]
    l.yolo_classify_views_u8.argtypes = [P, P, SZ, P, I, I, I, I, I, F, I, P, P, I]
    l.yolo_op_view_reduce.argtypes = [P, I, I, I, F, I, P, P, P, I]
    l.yolo_frame_to_rgb_host.argtypes = [P, P, SZ, P]
    l.yolo_op_frame_to_rgb.argtypes = [P, P, SZ, P, I]
    l.yolo_forward_frames_u8.argtypes = l.yolo_forward_images_u8.argtypes
    l.yolo_detect_frames_u8.argtypes = l.yolo_detect_images_u8.argtypes
    l.yolo_detect_frames_graph.argtypes = l.yolo_detect_images_graph.argtypes
    l.yolo_detect_tiled_frames_u8.argtypes = l.yolo_detect_tiled_u8.argtypes
    l.yolo_jpeg_info.argtypes = [P, SZ, P]
    l.yolo_jpeg_to_rgb_host.argtypes = [P, SZ, P, SZ]
    l.yolo_jpeg_coefficients.argtypes = [P, SZ, P, SZ]
    l.yolo_op_jpeg_to_rgb.argtypes = [P, SZ, P, I]
    l.yolo_decode_jpegs.argtypes = [P, P, P, I, P, C.POINTER(P), C.POINTER(SZ)]
    l.yolo_jpeg_decode_times.argtypes = [P, C.POINTER(D), C.POINTER(D), C.POINTER(D), C.POINTER(SZ)]
    l.yolo_set_jpeg_entropy.argtypes = [P, I]
    l.yolo_jpeg_entropy.argtypes = [P]
    l.yolo_jpeg_entropy_times.argtypes = [P, C.POINTER(I), C.POINTER(I), C.POINTER(I), C.POINTER(D), C.POINTER(D), C.POINTER(SZ)]
    l.yolo_jpeg_intervals.argtypes = [P, SZ, P, P, SZ, C.POINTER(SZ)]
    l.yolo_op_jpeg_entropy.argtypes = [P, SZ, P, SZ, I]
    l.yolo_forward_jpegs.argtypes = [P, P, P, I, I, P, I]
    l.yolo_detect_jpegs.argtypes = [P, P, P, I, I, F, F, I, I, I, I, P, P, I]
    l.yolo_detect_tiled_jpegs.argtypes = [P, P, P, I, I, I, I, I, I, F, F, I, I, I, I, P, P, I]
    l.yolo_classify_frames_u8.argtypes = l.yolo_classify_images_u8.argtypes
    l.yolo_classify_views_frames_u8.argtypes = l.yolo_classify_views_u8.argtypes
    l.yolo_segment_frames_u8.argtypes = [P, P, SZ, P, I, I, I, F, P, P]
    l.yolo_classify_jpegs.argtypes = [P, P, P, I, I, I, P, P, I]
    l.yolo_classify_views_jpegs.argtypes = [P, P, P, I, I, I, I, F, I, P, P, I]
    l.yolo_segment_jpegs.argtypes = [P, P, P, I, I, F, P, P]
    l.yolo_vector_inputs.argtypes = [P]
    l.yolo_forward_vectors.argtypes = [P, P, I, I, P, SZ]
    l.yolo_sequence.argtypes = [P, I, I, P, I, P, F, P, P, I]
    l.yolo_set_temperature.argtypes = [P, F]
    l.yolo_reset_temperature.argtypes = [P]
    l.yolo_op_sample.argtypes = [P, I, I, P, F, P, I]
    l.yolo_shard_bounds.argtypes = [I, I, I, C.POINTER(I), C.POINTER(I)]
    l.yolo_dist_flat_words.argtypes = [I, I]; l.yolo_dist_flat_words.restype = C.c_size_t
    l.yolo_dist_split_records.argtypes = [P, I, I, I, P, P]
    l.yolo_dist_unique_id.argtypes = [P]
    l.yolo_dist_create.argtypes = [P, I, I, P, P, I, I, C.c_char_p, C.c_size_t]; l.yolo_dist_create.restype = P
    l.yolo_dist_detect.argtypes = [P, P, I, F, F, F, I, I, P, P]
    l.yolo_dist_detect_async.argtypes = [P, P, I, F, F, F, I, I, C.POINTER(P)]
    l.yolo_dist_destroy.argtypes = [P]; l.yolo_dist_destroy.restype = None
    _lib = l
    return l


def _ptr(a):
    """host numpy array / torch tensor (host or device) / raw int pointer -> (void*, location)."""
    if a is None:
        return None, HOST
    if isinstance(a, int):
        return C.c_void_p(a), DEVICE
    if isinstance(a, np.ndarray):
        if not a.flags["C_CONTIGUOUS"]:
            raise YoloError("array must be C-contiguous")
        return C.c_void_p(a.ctypes.data), HOST
    if hasattr(a, "data_ptr"):   # torch tensor, no torch import needed
        if not a.is_contiguous():
            raise YoloError("tensor must be contiguous")
        return C.c_void_p(a.data_ptr()), (DEVICE if a.is_cuda else HOST)
    raise YoloError("unsupported buffer type %r" % type(a))


def _op_check(rc, what):
    if rc != 0:
        msg = load_library().yolo_last_error(None)
        raise YoloError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))


_warned_legacy = False
HIP_STREAM_LEGACY = 1     # hipStreamLegacy: the explicit handle of the legacy NULL stream (hip_runtime_api.h)


class ChannelError(YoloError, ValueError):
    """An image whose channel count is not the network's."""


def pack_images(images, channels=3):
    """A list of uint8 [h, w, channels] arrays of any sizes (RGB by default; a [h, w] array is one plane) -> (packed uint8 buffer,
    DESC_DTYPE descriptors): the images back to back in list order, each C-contiguous, offset = bytes of the images before it.  Pure
    host code; what yolo_*_images_* read.  ChannelError (a ValueError) for an image of another channel count."""
    arrs = []
    for i, im in enumerate(images):
        a = np.ascontiguousarray(im)
        if a.ndim == 2 and channels != 3:
            a = a[:, :, None]
        if a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] != channels and channels != 3:
            raise ChannelError("image %d: %d channels, the network reads %d" % (i, a.shape[2], channels))
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != channels or a.shape[0] < 1 or a.shape[1] < 1:
            raise YoloError("image %d: need a uint8 [h, w, %d] array, got %s %s" % (i, channels, a.dtype, a.shape))
        arrs.append(a)
    if not arrs:
        raise YoloError("pack_images: no images")
    descs = np.zeros(len(arrs), dtype=DESC_DTYPE)
    off = 0
    for i, a in enumerate(arrs):
        descs[i] = (off, a.shape[0], a.shape[1])
        off += a.size
    buf = np.empty(off, dtype=np.uint8)
    for a, d in zip(arrs, descs):
        buf[int(d["offset"]):int(d["offset"]) + a.size] = a.reshape(-1)
    return buf, descs


def _descs(descs):
    d = np.ascontiguousarray(descs)
    if d.dtype != DESC_DTYPE:
        d = np.ascontiguousarray(np.asarray(descs), dtype=DESC_DTYPE)
    return d


def frame_plane_rows(h, w, format):
    """(rows, bytes per row) of every plane a frame of `format` has, in plane order"""
    ch, cw = (int(h) + 1) // 2, (int(w) + 1) // 2
    if format == PIX_NV12:
        return [(int(h), int(w)), (ch, 2 * cw)]
    if format == PIX_I420:
        return [(int(h), int(w)), (ch, cw), (ch, cw)]
    if format in (PIX_RGB24, PIX_BGR24):
        return [(int(h), 3 * int(w))]
    if format == PIX_JPEG_GREY:
        return [(int(h), int(w))]
    if format in (PIX_JPEG_444, PIX_JPEG_422, PIX_JPEG_420, PIX_JPEG_440):
        rows = ch if format in (PIX_JPEG_420, PIX_JPEG_440) else int(h)
        cols = cw if format in (PIX_JPEG_422, PIX_JPEG_420) else int(w)
        return [(int(h), int(w)), (rows, cols), (rows, cols)]
    raise YoloError("unknown pixel format %r" % (format,))


class Frame(object):
    """One decoded video frame as a decoder or a capture leaves it (yolo_frame_desc): `data` a uint8 buffer (host numpy array of any shape,
    read flat) that holds the planes of an h x w frame in `format` (PIX_NV12, PIX_I420, PIX_RGB24, PIX_BGR24), plane p beginning at byte
    offsets[p] of it with rows pitch[p] bytes apart.  pitch: one int for every plane or one per plane; None: the rows' own bytes.  offsets:
    None: the planes back to back in plane order, each rows * pitch bytes.  matrix: MATRIX_BT601 / MATRIX_BT709 (limited range) or
    MATRIX_BT601_FULL (JFIF); not read for the RGB formats.  The PIX_JPEG_* formats -- the component planes of a decoded JPEG file, what
    Engine.decode_jpegs describes -- carry their own rule: their matrix must be 0 (the default)."""

    def __init__(self, data, h, w, format, matrix=MATRIX_BT601, pitch=None, offsets=None):
        self.data = np.ascontiguousarray(data).reshape(-1)
        if self.data.dtype != np.uint8:
            raise YoloError("Frame: need uint8 data, got %s" % self.data.dtype)
        self.h, self.w, self.format, self.matrix = int(h), int(w), int(format), int(matrix)
        planes = frame_plane_rows(h, w, self.format)
        if pitch is None:
            pitch = [row for _, row in planes]
        elif np.ndim(pitch) == 0:
            pitch = [int(pitch)] * len(planes)
        if offsets is None:
            offsets, off = [], 0
            for (rows, _), pt in zip(planes, pitch):
                offsets.append(off)
                off += rows * int(pt)
        if len(pitch) != len(planes) or len(offsets) != len(planes):
            raise YoloError("Frame: format %d has %d planes, got %d pitches and %d offsets" % (self.format, len(planes), len(pitch), len(offsets)))
        self.pitch = [int(p) for p in pitch]
        self.offsets = [int(o) for o in offsets]

    def desc(self, base=0):
        """the FRAME_DTYPE record of this frame with its data at byte `base` of a packed buffer"""
        d = np.zeros(1, dtype=FRAME_DTYPE)
        n = len(self.offsets)
        d["offset"][0, :n] = [base + o for o in self.offsets]
        d["pitch"][0, :n] = self.pitch
        d["h"], d["w"], d["format"], d["matrix"] = self.h, self.w, self.format, self.matrix
        return d


def pack_frames(frames):
    """A list of Frame -> (packed uint8 buffer, FRAME_DTYPE descriptors): every frame's data back to back in list order, its plane offsets
    moved by the bytes in front of it; pitches, sizes, formats and matrices as the frames state them.  Pure host code; what
    yolo_*_frames_* read."""
    frames = list(frames)
    if not frames:
        raise YoloError("pack_frames: no frames")
    for i, f in enumerate(frames):
        if not isinstance(f, Frame):
            raise YoloError("pack_frames: frame %d is %r, not a hip.Frame" % (i, type(f)))
    descs = np.zeros(len(frames), dtype=FRAME_DTYPE)
    off = 0
    for i, f in enumerate(frames):
        descs[i] = f.desc(off)[0]
        off += f.data.size
    return np.concatenate([f.data for f in frames]), descs


def _frame_descs(descs):
    d = np.ascontiguousarray(descs)
    if d.dtype != FRAME_DTYPE:
        raise YoloError("frame descriptors: need a FRAME_DTYPE array (pack_frames), got %s" % d.dtype)
    return d.reshape(-1)


def frame_to_rgb(frame, device=None):
    """The uint8 [h, w, 3] RGB image the colour rule yields for a frame (a Frame, or a (buffer, FRAME_DTYPE record) pair): on the host
    (yolo_frame_to_rgb_host; no device is touched) or, with `device` an ordinal, by the device operator (yolo_op_frame_to_rgb).  The two
    agree bit for bit; every fit reads a frame as this image."""
    l = load_library()
    if isinstance(frame, Frame):
        buf, d = frame.data, frame.desc()
    else:
        buf, d = frame
        buf = np.ascontiguousarray(buf).reshape(-1)
        d = _frame_descs(d)[:1].copy()
    out = np.zeros((max(int(d["h"][0]), 0), max(int(d["w"][0]), 0), 3), dtype=np.uint8)
    if device is None:
        _op_check(l.yolo_frame_to_rgb_host(d.ctypes.data, buf.ctypes.data, buf.size, out.ctypes.data), "yolo_frame_to_rgb_host")
    else:
        _op_check(l.yolo_op_frame_to_rgb(d.ctypes.data, buf.ctypes.data, buf.size, out.ctypes.data, int(device)), "yolo_op_frame_to_rgb")
    return out


# ---- JPEG files (include/yolo_hip.h "JPEG files"): host entropy decode, IDCT and colour on the device; bit-equal to darknet's load_image ----
class _JpegInfo(C.Structure):
    _fields_ = [("h", C.c_int32), ("w", C.c_int32), ("components", C.c_int32), ("hs", C.c_int32), ("vs", C.c_int32), ("format", C.c_int32),
                ("restart_interval", C.c_int32), ("mcus_w", C.c_int32), ("mcus_h", C.c_int32), ("plane_w", C.c_int32 * 3), ("plane_h", C.c_int32 * 3),
                ("blocks", C.c_int32 * 3)]


def _jpeg_bytes(f):
    """one file as a bytes object: bytes-like as they are, anything else is a path"""
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    with open(os.fspath(f), "rb") as fh:
        return fh.read()


class _JpegFiles(object):
    """files (bytes objects or paths) as the (files, bytes, n) triple of the C entry points; holds the buffers alive"""

    def __init__(self, files):
        if isinstance(files, (bytes, bytearray, memoryview, str)) or hasattr(files, "__fspath__"):
            raise YoloError("JPEG files: need a list of bytes objects or paths, got one %s" % type(files).__name__)
        self.data = [_jpeg_bytes(f) for f in files]
        self.n = len(self.data)
        if not self.n:
            raise YoloError("JPEG files: no files")
        self.ptrs = (C.c_char_p * self.n)(*self.data)
        self.sizes = (C.c_size_t * self.n)(*[len(d) for d in self.data])


def jpeg_info(file):
    """The headers of one JPEG file (bytes or a path) as a dict (yolo_jpeg_info): h, w, components, the luma sampling hs x vs, the PIX_JPEG_* format of
    its frame, restart_interval, mcus (w, h), the padded component planes and their blocks.  Host only.  A file of a kind that is not served
    (progressive, CMYK, ...) or a malformed one raises YoloError with the library's text: code -6 (unsupported) or -1 (invalid)."""
    data = _jpeg_bytes(file)
    info = _JpegInfo()
    _op_check(load_library().yolo_jpeg_info(data, len(data), C.byref(info)), "yolo_jpeg_info")
    n = info.components
    return {"h": info.h, "w": info.w, "components": n, "hs": info.hs, "vs": info.vs, "format": info.format, "restart_interval": info.restart_interval,
            "mcus": (info.mcus_w, info.mcus_h), "planes": [(info.plane_h[p], info.plane_w[p]) for p in range(n)], "blocks": [info.blocks[p] for p in range(n)]}


def jpeg_coefficients(file):
    """The host stage by itself (yolo_jpeg_coefficients): the dequantised coefficient blocks of a JPEG file, one int16 array
    [blocks down, blocks across, 8, 8] per component plane (natural order: [..., v, u] is row v, column u of the block)."""
    data = _jpeg_bytes(file)
    l = load_library()
    info = _JpegInfo()
    _op_check(l.yolo_jpeg_info(data, len(data), C.byref(info)), "yolo_jpeg_info")
    n = info.components
    coef = np.zeros((sum(info.blocks[p] for p in range(n)), 8, 8), dtype=np.int16)
    _op_check(l.yolo_jpeg_coefficients(data, len(data), coef.ctypes.data, coef.shape[0]), "yolo_jpeg_coefficients")
    out, at = [], 0
    for p in range(n):
        out.append(coef[at:at + info.blocks[p]].reshape(info.plane_h[p] // 8, info.plane_w[p] // 8, 8, 8))
        at += info.blocks[p]
    return out


JPEG_ENTROPY_HOST, JPEG_ENTROPY_AUTO = 0, 1          # YOLO_JPEG_ENTROPY_*: who Huffman-decodes the files of a batch (Engine.set_jpeg_entropy)
_JPEG_ENTROPY = {"host": JPEG_ENTROPY_HOST, "auto": JPEG_ENTROPY_AUTO}


def jpeg_intervals(file):
    """The restart intervals of a JPEG file (bytes or a path) that the device's entropy stage would decode (yolo_jpeg_intervals): a uint32 array [n, 2],
    interval i the bytes [i, 0] .. [i, 1] - 1 of the file.  Empty for a file that is not eligible -- no DRI segment, or a marker missing or out of place --:
    such a file is the host stage's.  Host only."""
    data = _jpeg_bytes(file)
    l = load_library()
    n = C.c_size_t()
    _op_check(l.yolo_jpeg_intervals(data, len(data), None, None, 0, C.byref(n)), "yolo_jpeg_intervals")
    begin, end = np.zeros(n.value, dtype=np.uint32), np.zeros(n.value, dtype=np.uint32)
    if n.value:
        _op_check(l.yolo_jpeg_intervals(data, len(data), begin.ctypes.data, end.ctypes.data, n.value, C.byref(n)), "yolo_jpeg_intervals")
    return np.stack([begin, end], axis=1)


def jpeg_coefficients_device(file, device=0):
    """jpeg_coefficients through the device's entropy stage (yolo_op_jpeg_entropy): scan, upload, k_jpeg_entropy, read-back; the same arrays, bit for bit.
    A file without a restart interval raises YoloError (-6); one the device hands back is decoded, or refused, by the host stage."""
    data = _jpeg_bytes(file)
    l = load_library()
    info = _JpegInfo()
    _op_check(l.yolo_jpeg_info(data, len(data), C.byref(info)), "yolo_jpeg_info")
    n = info.components
    coef = np.zeros((sum(info.blocks[p] for p in range(n)), 8, 8), dtype=np.int16)
    _op_check(l.yolo_op_jpeg_entropy(data, len(data), coef.ctypes.data, coef.shape[0], int(device)), "yolo_op_jpeg_entropy")
    out, at = [], 0
    for p in range(n):
        out.append(coef[at:at + info.blocks[p]].reshape(info.plane_h[p] // 8, info.plane_w[p] // 8, 8, 8))
        at += info.blocks[p]
    return out


def jpeg_to_rgb(file, device=None):
    """The uint8 [h, w, 3] image of a JPEG file (bytes or a path), bit-equal to what darknet's load_image reads: wholly on the host
    (yolo_jpeg_to_rgb_host; no device is touched) or, with `device` an ordinal, entropy stage on the host and IDCT, upsampling and colour by the
    device kernels (yolo_op_jpeg_to_rgb)."""
    data = _jpeg_bytes(file)
    l = load_library()
    info = _JpegInfo()
    _op_check(l.yolo_jpeg_info(data, len(data), C.byref(info)), "yolo_jpeg_info")
    out = np.zeros((info.h, info.w, 3), dtype=np.uint8)
    if device is None:
        _op_check(l.yolo_jpeg_to_rgb_host(data, len(data), out.ctypes.data, out.size), "yolo_jpeg_to_rgb_host")
    else:
        _op_check(l.yolo_op_jpeg_to_rgb(data, len(data), out.ctypes.data, int(device)), "yolo_op_jpeg_to_rgb")
    return out


class JpegFrames(object):
    """What Engine.decode_jpegs returns: the frame table (`descs`, FRAME_DTYPE) of a decoded batch over the engine's surface -- `pixels`, a raw device
    pointer, `nbytes` its capacity.  Pass it wherever frames are taken (forward_frames, detect_frames, detect_tiled_frames, classify_frames, classify_views_frames, segment_frames; detect_frames_graph:
    pixels_dev=handle.pixels, descs=handle.descs, nbytes=handle.nbytes).  Valid until the engine's next decode."""

    def __init__(self, pixels, nbytes, descs):
        self.pixels, self.nbytes, self.descs = int(pixels), int(nbytes), descs

    def __len__(self):
        return len(self.descs)


def fit_unit_value(fit, value):
    """What one source byte contributes to a fit's arithmetic before interpolation (yolo_fit_unit_value): host evaluation of the
    expression the fit kernel evaluates."""
    return load_library().yolo_fit_unit_value(fit, value)


def _pair(v, what):
    """an int, or an (h, w) pair -> (h, w) ints"""
    if np.ndim(v) == 0:
        return int(v), int(v)
    if len(v) != 2:
        raise YoloError("%s: an int or an (h, w) pair, got %r" % (what, v))
    return int(v[0]), int(v[1])


def tile_windows(img_hw, tile_hw, overlap_hw):
    """yolo_tile_windows: the window grid an image of img_hw = (h, w) is cut into by tiles of tile_hw with overlap_hw pixels of overlap
    (each an int or an (h, w) pair) -> int32 [count, 4] rows (y0, x0, h, w), row-major.  Per axis: an image no larger than the tile is
    one window of its own extent; otherwise stride = tile - overlap, ceil((L - tile) / stride) + 1 windows of the tile's extent, the last
    pulled back to the image's edge.  Host code: no device."""
    l = load_library()
    (ih, iw), (th, tw), (oh, ow) = _pair(img_hw, "img_hw"), _pair(tile_hw, "tile_hw"), _pair(overlap_hw, "overlap_hw")
    n = C.c_int(0)
    _op_check(l.yolo_tile_windows(ih, iw, th, tw, oh, ow, None, 0, C.byref(n)), "yolo_tile_windows")
    out = np.zeros((n.value, 4), dtype=np.int32)
    _op_check(l.yolo_tile_windows(ih, iw, th, tw, oh, ow, out.ctypes.data, n.value, C.byref(n)), "yolo_tile_windows")
    return out


def view_table(views, shift=32):
    """yolo_view_table: the views of VIEWS_FLIP (the image and its mirror) or VIEWS_TEN_CROP (darknet's `classifier valid10`: five crop_image
    windows of the image resized to network + shift, then the same five of its mirror) -> VIEW_DTYPE [K] in view order.  Host code: no device."""
    l = load_library()
    n = C.c_int(0)
    _op_check(l.yolo_view_table(int(views), int(shift), None, 0, C.byref(n)), "yolo_view_table")
    out = np.zeros(n.value, dtype=VIEW_DTYPE)
    _op_check(l.yolo_view_table(int(views), int(shift), out.ctypes.data, n.value, C.byref(n)), "yolo_view_table")
    return out


def _stream_handle(stream):
    """None: the engine creates a stream of its own.  An integer handle: the caller's stream -- and a handle of 0, which is what
    torch.cuda.current_stream().cuda_stream reads on torch's DEFAULT stream, means that stream, not "none": it is passed on as
    hipStreamLegacy, so that everything stays stream-ordered (NULL at the C boundary would mean "create one").  The legacy stream cannot
    be captured: detect_graph then launches the step eagerly (same device time, ~0.17 ms of host time per step; a one-time
    RuntimeWarning says so).  The legacy stream orders itself against torch's default stream and every BLOCKING stream; a tensor produced
    on a NON-blocking side stream (torch.cuda.Stream() is one) must be ordered by the caller (event / synchronize) before it is handed
    over -- unlike stream=None, where the engine waits on the host for the producer stream."""
    if stream is None:
        return None
    if int(stream) == 0:
        global _warned_legacy
        if not _warned_legacy:
            _warned_legacy = True
            import warnings
            warnings.warn("stream handle 0 is torch's default (legacy NULL) stream: the engine runs on hipStreamLegacy, detect_graph launches "
                          "eagerly (the legacy stream cannot be captured) and tensors from non-blocking side streams are not ordered "
                          "against it; pass stream=None for an engine-owned stream or a created stream's handle", RuntimeWarning, stacklevel=3)
        return HIP_STREAM_LEGACY
    return int(stream)


class Engine:
    """One planned network on one GPU (a `yolo_ctx`)."""

    def __init__(self, cfg_text, max_batch=1, dtype=BF16, semantics=SEM_TF, decode=DECODE_RATIO, device=0,
                 keep_layers=False, stream=None):
        self.lib = load_library()
        self._cfg_bytes = cfg_text.encode()
        stream = _stream_handle(stream)
        conf = _Config(C.sizeof(_Config), self._cfg_bytes, max_batch, dtype, semantics, decode, device,
                       1 if keep_layers else 0, C.c_void_p(stream) if stream else None)
        err = C.create_string_buffer(512)
        self.ctx = self.lib.yolo_create(C.byref(conf), err, 512)
        if not self.ctx:
            raise YoloError("yolo_create: " + err.value.decode())
        h, w, ch = C.c_int(), C.c_int(), C.c_int()
        self.lib.yolo_input_size(self.ctx, C.byref(h), C.byref(w), C.byref(ch))
        self.size = h.value                        # the input's height; input_hw: both sides
        self.input_hw = (h.value, w.value)
        self.input_channels = ch.value             # 3, or the N of [net] yolo_input=planes (a vector-input network: its inputs=)
        self.rows = self.lib.yolo_num_rows(self.ctx)
        self.attrs = self.lib.yolo_num_attrs(self.ctx)
        self.num_layers = self.lib.yolo_num_layers(self.ctx)
        self.max_batch = max_batch
        self.dtype = dtype
        self._own_stream = not stream

    @classmethod
    def from_file(cls, path, max_batch=1, device=0, keep_layers=False, stream=None):
        """Load an export artifact written by `export` (cfg + run configuration + packed parameters + tile plan)."""
        self = cls.__new__(cls)
        self.lib = load_library()
        stream = _stream_handle(stream)
        err = C.create_string_buffer(512)
        self.ctx = self.lib.yolo_create_from_file(os.fsencode(path), max_batch, device, C.c_void_p(stream) if stream else None,
                                                  1 if keep_layers else 0, err, 512)
        if not self.ctx:
            raise YoloError("yolo_create_from_file: " + err.value.decode())
        h, w, ch = C.c_int(), C.c_int(), C.c_int()
        self.lib.yolo_input_size(self.ctx, C.byref(h), C.byref(w), C.byref(ch))
        self.size = h.value
        self.input_hw = (h.value, w.value)
        self.input_channels = ch.value
        self.rows = self.lib.yolo_num_rows(self.ctx); self.attrs = self.lib.yolo_num_attrs(self.ctx)
        self.num_layers = self.lib.yolo_num_layers(self.ctx); self.max_batch = max_batch; self.dtype = None
        self._own_stream = not stream
        return self

    def export(self, path):
        self._check(self.lib.yolo_export(self.ctx, os.fsencode(path)), "yolo_export")

    def _check(self, rc, what):
        if rc != 0:
            raise YoloError("%s failed (%d): %s" % (what, rc, self.lib.yolo_last_error(self.ctx).decode()))

    def _order_after_producer(self, *tensors):
        """Stream ordering for device tensors.  An engine created with stream=None runs on a stream of its own, which
        nothing orders against the torch stream that produced `tensors`: wait (on the host) for that stream first.  The
        engine's own device outputs are valid after `synchronize()`.  With an explicit stream (the `.cuda_stream` of a torch.cuda.Stream
        made current, what bench.py passes; or torch's default stream, handle 0, passed on as hipStreamLegacy) everything is
        stream-ordered and nothing is waited for."""
        if not self._own_stream:
            return
        for t in tensors:
            if hasattr(t, "is_cuda") and t.is_cuda:
                import torch
                torch.cuda.current_stream(t.device).synchronize()
                return

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.yolo_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights ----
    def weights_count(self):
        return self.lib.yolo_weights_count(self.ctx)

    def set_act_scales(self, scales):
        """FP8 engines: one activation scale per cfg layer (code = e4m3(value / scale)); call before loading weights."""
        sc = np.ascontiguousarray(scales, dtype=np.float32)
        self._check(self.lib.yolo_set_act_scales(self.ctx, sc.ctypes.data, sc.size), "yolo_set_act_scales")

    def load_weights(self, path, header_ints=0):
        self._check(self.lib.yolo_load_darknet_weights(self.ctx, os.fsencode(path), header_ints), "yolo_load_darknet_weights")

    def set_weights(self, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        self._check(self.lib.yolo_set_weights(self.ctx, flat.ctypes.data_as(C.POINTER(C.c_float)), flat.size), "yolo_set_weights")

    # ---- hot path ----
    def _check_channels(self, images, fmt=None):
        """[n, H, W, C] (IMG_F32_CHW: [n, C, H, W]) arrays of a network of another channel count: ChannelError, naming both counts"""
        shape = getattr(images, "shape", None)
        if shape is None or len(shape) != 4 or self.vector_inputs:          # (a vector-input network: the library refuses the call by name)
            return
        got = int(shape[1] if fmt == IMG_F32_CHW else shape[3])
        if got != self.input_channels:
            raise ChannelError("images of %d channels, the network reads %d" % (got, self.input_channels))

    def _image_channels(self):
        return 3 if self.vector_inputs else self.input_channels

    def forward(self, images, scale=1.0 / 255.0, want_detections=True, n=None, fmt=None, out=None):
        """images: uint8 or float32 [n,in_h,in_w,C] (input_hw, input_channels; numpy, torch host/device tensor, or raw device pointer with
        n and fmt given).  Returns the decoded tensor [n, rows, attrs] (numpy) unless out/want_detections say otherwise."""
        self._check_channels(images, fmt)
        p, loc = _ptr(images)
        # a device uint8 image may be read IN PLACE by the fused stem, also by a later time_forward / time_layers / autotune pass
        # (yolo_hip.h, yolo_forward): keep it alive until the next image replaces it
        self._last_image = images if loc == DEVICE else None
        self._order_after_producer(images, out)
        if n is None:
            n = int(images.shape[0])
        if fmt is None:
            fmt = IMG_U8 if str(images.dtype).endswith("uint8") else IMG_F32
        det = None
        dp, dloc = None, HOST
        if out is not None:
            dp, dloc = _ptr(out)
        elif want_detections:
            det = np.empty((n, self.rows, self.attrs), dtype=np.float32)
            dp, dloc = _ptr(det)
        self._check(self.lib.yolo_forward(self.ctx, p, n, fmt, loc, scale, dp, dloc), "yolo_forward")
        return det

    def forward_image(self, image_u8):
        """One uint8 image of any size, [h, w, input_channels] (RGB; one plane: [h, w] too): /255 + legacy bilinear stretch on the device, then forward."""
        image_u8 = np.ascontiguousarray(image_u8, dtype=np.uint8)
        if image_u8.ndim == 2 and self._image_channels() != 3:
            image_u8 = image_u8[:, :, None]
        if image_u8.ndim != 3 or image_u8.shape[2] != self._image_channels():
            raise ChannelError("forward_image: an image of shape %s, the network reads %d channels" % (image_u8.shape, self.input_channels))
        det = np.empty((1, self.rows, self.attrs), dtype=np.float32)
        self._check(self.lib.yolo_forward_image_u8(self.ctx, image_u8.ctypes.data, image_u8.shape[0], image_u8.shape[1],
                                                   HOST, det.ctypes.data, HOST), "yolo_forward_image_u8")
        return det

    def postprocess(self, n, score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=NMS_TF, select_mode=SELECT_GT,
                    boxes_out=None, counts_out=None, rows_out=None, return_rows=False):
        """-> list of structured arrays (BOX_DTYPE) per image, or writes into the given device buffers.
        return_rows=True: -> (records, rows) where rows[i] holds, for every kept record of image i, the row of the decoded tensor
        it was formed from (yolo_postprocess_rows); rows_out: the same into a device int32 buffer [n * max_out]."""
        if boxes_out is not None:
            bp, bloc = _ptr(boxes_out); cp, _ = _ptr(counts_out); rp, _ = _ptr(rows_out)
            self._order_after_producer(boxes_out, counts_out, rows_out)
            self._check(self.lib.yolo_postprocess_rows(self.ctx, n, score_thr, iou_thr, max_out, nms_mode, select_mode, bp, cp, rp, bloc), "yolo_postprocess")
            return None
        boxes = np.zeros((n, max_out), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
        rows = np.full((n, max_out), -1, dtype=np.int32) if return_rows else None
        self._check(self.lib.yolo_postprocess_rows(self.ctx, n, score_thr, iou_thr, max_out, nms_mode, select_mode,
                                                   boxes.ctypes.data, counts.ctypes.data, rows.ctypes.data if return_rows else None, HOST), "yolo_postprocess")
        recs = [boxes[i, :counts[i]].copy() for i in range(n)]
        if return_rows:
            return recs, [rows[i, :counts[i]].copy() for i in range(n)]
        return recs

    def head_geometry(self, head):
        """Detection head `head` (cfg order) -> dict(kind, grid_h, grid_w, anchors, row_offset) (yolo_head_geometry_hw): kind 0 [yolo],
        1 [region], 2 [detection]; rows of the decoded tensor are cell-major (cell = row * grid_w + col), the anchor inner."""
        kind, gh, gw, na, off = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.yolo_head_geometry_hw(self.ctx, head, C.byref(kind), C.byref(gh), C.byref(gw), C.byref(na), C.byref(off)), "yolo_head_geometry_hw")
        return {"kind": kind.value, "grid_h": gh.value, "grid_w": gw.value, "anchors": na.value, "row_offset": off.value}

    def head_raw(self, head, n):
        """Raw fp32 tensor [n, grid_h, grid_w, anchors * (5 + classes)] that detection head `head` decodes (yolo_head_raw)."""
        g = self.head_geometry(head)
        out = np.empty((n, g["grid_h"], g["grid_w"], g["anchors"] * self.attrs), dtype=np.float32)
        self._check(self.lib.yolo_head_raw(self.ctx, head, n, out.ctypes.data, out.size), "yolo_head_raw")
        return out

    def last_layer_output(self, n=1):
        """darknet's net->output (DN/network.c:497-508) of images 0..n-1 of the last forward: [n, yolo_last_layer_size()] float32."""
        self.lib.yolo_last_layer_size.restype = C.c_size_t
        per = self.lib.yolo_last_layer_size(self.ctx)
        out = np.empty((n, per), dtype=np.float32)
        self._check(self.lib.yolo_last_layer_output_batch(self.ctx, n, out.ctypes.data, out.size), "yolo_last_layer_output_batch")
        return out

    # ---- softmax trees (a [region] or [softmax] section with tree=) ----
    def set_hier_thresh(self, hier_thresh):
        """hier_thresh of postprocess / detect* / darknet_boxes on a network with a tree head (yolo_set_hier_thresh; default 0.5)."""
        self._check(self.lib.yolo_set_hier_thresh(self.ctx, float(hier_thresh)), "yolo_set_hier_thresh")

    def set_hierarchy_mode(self, mode):
        """What classify* returns for a tree classifier: None / "conditional", "absolute" or "leaves" (yolo_set_hierarchy_mode)."""
        self._check(self.lib.yolo_set_hierarchy_mode(self.ctx, _HIER_MODES[mode] if mode in _HIER_MODES else int(mode)), "yolo_set_hierarchy_mode")

    def tree_geometry(self):
        """The network's softmax tree -> dict(n, groups, parent, child, group_offset, group_size, leaf), or None without one."""
        n, g = C.c_int32(0), C.c_int32(0)
        self._check(self.lib.yolo_tree_geometry(self.ctx, C.byref(n), C.byref(g), None, None, None, None, None), "yolo_tree_geometry")
        if n.value == 0:
            return None
        a = {k: np.zeros(n.value if k in ("parent", "child", "leaf") else g.value, dtype=np.int32) for k in ("parent", "child", "group_offset", "group_size", "leaf")}
        self._check(self.lib.yolo_tree_geometry(self.ctx, None, None, a["parent"].ctypes.data, a["child"].ctypes.data, a["group_offset"].ctypes.data,
                                                a["group_size"].ctypes.data, a["leaf"].ctypes.data), "yolo_tree_geometry")
        a.update(n=n.value, groups=g.value)
        return a

    def detect(self, images, scale=1.0 / 255.0, hier_thresh=None, **kw):
        """forward, then postprocess(**kw).  hier_thresh (networks with a tree head): None leaves the context's value alone."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        self.forward(images, scale=scale, want_detections=False)
        return self.postprocess(int(images.shape[0]), **kw)

    def detect_fused(self, images, scale=1.0 / 255.0, hier_thresh=None, **kw):
        """yolo_detect: forward + threshold + NMS as one call that never materialises the decoded tensor (the lean decode of [yolo]
        heads, the descent form of a tree head); records to the host.  Keywords as for postprocess."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        p, loc = _ptr(images)
        self._last_image = images if loc == DEVICE else None
        self._order_after_producer(images)
        n = int(images.shape[0])
        fmt = IMG_U8 if str(images.dtype).endswith("uint8") else IMG_F32
        a = dict(score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=NMS_TF, select_mode=SELECT_GT); a.update(kw)
        boxes = np.zeros((n, a["max_out"]), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
        self._check(self.lib.yolo_detect(self.ctx, p, n, fmt, loc, scale, a["score_thr"], a["iou_thr"], a["max_out"], a["nms_mode"], a["select_mode"],
                                         boxes.ctypes.data, counts.ctypes.data, HOST), "yolo_detect")
        return [boxes[i, :counts[i]].copy() for i in range(n)]

    def detect_graph(self, images, boxes_out, counts_out, scale=1.0 / 255.0, score_thr=0.5, iou_thr=0.5, max_out=20,
                     nms_mode=NMS_TF, select_mode=SELECT_GT, hier_thresh=None):
        """Device-resident detect replayed from a HIP graph (images / boxes_out / counts_out: device tensors)."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        p, loc = _ptr(images); bp, bl = _ptr(boxes_out); cp, cl = _ptr(counts_out)
        if loc != DEVICE or bl != DEVICE or cl != DEVICE:
            raise YoloError("detect_graph needs device-resident buffers")
        self._last_image = images                   # (see forward)
        self._order_after_producer(images, boxes_out, counts_out)
        fmt = IMG_U8 if str(images.dtype).endswith("uint8") else IMG_F32
        self._check(self.lib.yolo_detect_graph(self.ctx, p, int(images.shape[0]), fmt, scale, score_thr, iou_thr, max_out,
                                               nms_mode, select_mode, bp, cp), "yolo_detect_graph")

    # ---- ragged batches of native-size images ----
    def _packed(self, images):
        if isinstance(images, tuple):
            buf, descs = images
        else:
            buf, descs = pack_images(images, self._image_channels())
        descs = _descs(descs)
        p, loc = _ptr(buf)
        nbytes = int(buf.numel()) if hasattr(buf, "numel") else int(buf.nbytes)
        return buf, descs, p, loc, nbytes

    def forward_images(self, images, fit=FIT_STRETCH, want_detections=True):
        """A list of uint8 RGB [h, w, 3] images of any sizes -- a network of planes ([net] yolo_input=planes): [h, w, input_channels], one plane also
        [h, w]; ChannelError for another count -- (or a (buffer, descs) pair from pack_images, the buffer on the host or
        the device) -> fitted on the device in one launch (`fit`), then forward.  Returns the decoded tensor [n, rows, attrs]."""
        buf, descs, p, loc, nbytes = self._packed(images)
        n = len(descs)
        self._order_after_producer(buf)
        det = np.empty((n, self.rows, self.attrs), dtype=np.float32) if want_detections else None
        self._check(self.lib.yolo_forward_images_u8(self.ctx, p, nbytes, descs.ctypes.data, n, fit, loc,
                                                    det.ctypes.data if det is not None else None, HOST), "yolo_forward_images_u8")
        return det

    def detect_images(self, images, fit=FIT_STRETCH, units=UNITS_NETWORK, score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=NMS_TF,
                      select_mode=SELECT_GT, hier_thresh=None):
        """forward_images + threshold + NMS with each image's own geometry (yolo_detect_images_u8) -> list of BOX_DTYPE arrays."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        buf, descs, p, loc, nbytes = self._packed(images)
        n = len(descs)
        self._order_after_producer(buf)
        boxes = np.zeros((n, max_out), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
        self._check(self.lib.yolo_detect_images_u8(self.ctx, p, nbytes, descs.ctypes.data, n, fit, loc, score_thr, iou_thr, max_out,
                                                   nms_mode, select_mode, units, boxes.ctypes.data, counts.ctypes.data, HOST),
                    "yolo_detect_images_u8")
        return [boxes[i, :counts[i]].copy() for i in range(n)]

    def detect_tiled(self, images, tile=None, overlap=(64, 64), fit=FIT_STRETCH, relative=False, score_thr=0.5, iou_thr=0.5, max_out=20,
                     nms_mode=NMS_TF, select_mode=SELECT_GT):
        """Detection in images larger than the network input (yolo_detect_tiled_u8): every image (a list of uint8 RGB [h, w, 3] arrays of any
        sizes and any number, or a (buffer, descs) pair from pack_images) is cut into overlapping windows of `tile` (None: the network's
        input size; an int or (h, w)) -- tile_windows states the grid --, the windows run max_batch at a time, their candidates are merged
        per image in source-image pixels and ONE NMS per image suppresses duplicates across windows.  -> list of BOX_DTYPE arrays, at most
        max_out records per image, in the image's pixels, or divided by its width and height with relative=True; NMS_DARKNET records hold
        (cx, cy, w, h) as detect_images reports them.  fit: FIT_STRETCH or FIT_LETTERBOX; nms_mode: NMS_TF or NMS_DARKNET."""
        buf, descs, p, loc, nbytes = self._packed(images)
        n = len(descs)
        th, tw = (0, 0) if tile is None else _pair(tile, "tile")
        oh, ow = _pair(overlap, "overlap")
        self._order_after_producer(buf)
        boxes = np.zeros((n, max_out), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
        self._check(self.lib.yolo_detect_tiled_u8(self.ctx, p, nbytes, descs.ctypes.data, n, th, tw, oh, ow, fit, loc, score_thr, iou_thr, max_out,
                                                  nms_mode, select_mode, 1 if relative else 0, boxes.ctypes.data, counts.ctypes.data, HOST),
                    "yolo_detect_tiled_u8")
        return [boxes[i, :counts[i]].copy() for i in range(n)]

    def detect_images_graph(self, pixels_dev, descs, boxes_out, counts_out, fit=FIT_STRETCH, units=UNITS_NETWORK, score_thr=0.5,
                            iou_thr=0.5, max_out=20, nms_mode=NMS_TF, select_mode=SELECT_GT, nbytes=None, hier_thresh=None):
        """yolo_detect_images_graph: pixels_dev a device uint8 tensor holding the packed images, descs (host) where each one lies this
        call; boxes_out / counts_out device tensors.  One captured graph serves every call with the same buffers and modes, whatever
        the image sizes."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        p, loc = _ptr(pixels_dev); bp, bl = _ptr(boxes_out); cp, cl = _ptr(counts_out)
        if loc != DEVICE or bl != DEVICE or cl != DEVICE:
            raise YoloError("detect_images_graph needs device-resident buffers")
        descs = _descs(descs)
        if nbytes is None:
            nbytes = int(pixels_dev.numel())
        self._order_after_producer(pixels_dev, boxes_out, counts_out)
        self._check(self.lib.yolo_detect_images_graph(self.ctx, p, nbytes, descs.ctypes.data, len(descs), fit, score_thr, iou_thr,
                                                      max_out, nms_mode, select_mode, units, bp, cp), "yolo_detect_images_graph")

    # ---- decoded video frames: NV12 / I420 / pitched RGB / BGR surfaces, converted while they are fitted ----
    def _packed_frames(self, frames):
        if isinstance(frames, JpegFrames):          # a decoded batch of JPEG files: the engine's own surface
            return frames.pixels, _frame_descs(frames.descs), C.c_void_p(frames.pixels), DEVICE, frames.nbytes
        if isinstance(frames, tuple):
            buf, descs = frames
        else:
            buf, descs = pack_frames(frames)
        descs = _frame_descs(descs)
        p, loc = _ptr(buf)
        nbytes = int(buf.numel()) if hasattr(buf, "numel") else int(buf.nbytes)
        return buf, descs, p, loc, nbytes

    def forward_frames(self, frames, fit=FIT_STRETCH, want_detections=True):
        """forward_images over a list of Frame (or a (buffer, descs) pair from pack_frames, the buffer on the host or the device): one
        launch converts and fits every frame (`fit`: any but FIT_CV2_BGR), then forward.  One batch may mix formats and matrices.  Returns the
        decoded tensor [n, rows, attrs]."""
        buf, descs, p, loc, nbytes = self._packed_frames(frames)
        n = len(descs)
        self._order_after_producer(buf)
        det = np.empty((n, self.rows, self.attrs), dtype=np.float32) if want_detections else None
        self._check(self.lib.yolo_forward_frames_u8(self.ctx, p, nbytes, descs.ctypes.data, n, fit, loc,
                                                    det.ctypes.data if det is not None else None, HOST), "yolo_forward_frames_u8")
        return det

    def detect_frames(self, frames, fit=FIT_STRETCH, units=UNITS_NETWORK, score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=NMS_TF,
                      select_mode=SELECT_GT, hier_thresh=None):
        """detect_images over frames (yolo_detect_frames_u8) -> list of BOX_DTYPE arrays; UNITS_SOURCE_PIXELS: in the frame's own pixels."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        buf, descs, p, loc, nbytes = self._packed_frames(frames)
        n = len(descs)
        self._order_after_producer(buf)
        boxes = np.zeros((n, max_out), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
        self._check(self.lib.yolo_detect_frames_u8(self.ctx, p, nbytes, descs.ctypes.data, n, fit, loc, score_thr, iou_thr, max_out,
                                                   nms_mode, select_mode, units, boxes.ctypes.data, counts.ctypes.data, HOST),
                    "yolo_detect_frames_u8")
        return [boxes[i, :counts[i]].copy() for i in range(n)]

    def detect_tiled_frames(self, frames, tile=None, overlap=(64, 64), fit=FIT_STRETCH, relative=False, score_thr=0.5, iou_thr=0.5, max_out=20,
                            nms_mode=NMS_TF, select_mode=SELECT_GT):
        """detect_tiled over frames (yolo_detect_tiled_frames_u8): every window is converted and fitted straight from the frame it lies in,
        chroma indexed by the pixel's position in the frame.  Arguments and records as detect_tiled."""
        buf, descs, p, loc, nbytes = self._packed_frames(frames)
        n = len(descs)
        th, tw = (0, 0) if tile is None else _pair(tile, "tile")
        oh, ow = _pair(overlap, "overlap")
        self._order_after_producer(buf)
        boxes = np.zeros((n, max_out), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
        self._check(self.lib.yolo_detect_tiled_frames_u8(self.ctx, p, nbytes, descs.ctypes.data, n, th, tw, oh, ow, fit, loc, score_thr, iou_thr,
                                                         max_out, nms_mode, select_mode, 1 if relative else 0, boxes.ctypes.data,
                                                         counts.ctypes.data, HOST), "yolo_detect_tiled_frames_u8")
        return [boxes[i, :counts[i]].copy() for i in range(n)]

    def detect_frames_graph(self, pixels_dev, descs, boxes_out, counts_out, fit=FIT_STRETCH, units=UNITS_NETWORK, score_thr=0.5,
                            iou_thr=0.5, max_out=20, nms_mode=NMS_TF, select_mode=SELECT_GT, nbytes=None, hier_thresh=None):
        """yolo_detect_frames_graph: detect_images_graph over frames -- pixels_dev a device uint8 tensor holding the surfaces, descs (host,
        FRAME_DTYPE) where each frame's planes lie this call.  One captured graph, kept apart from detect_images_graph's, serves every
        call with the same buffers and modes, whatever the frames' sizes, formats and pitches."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        p, loc = _ptr(pixels_dev); bp, bl = _ptr(boxes_out); cp, cl = _ptr(counts_out)
        if loc != DEVICE or bl != DEVICE or cl != DEVICE:
            raise YoloError("detect_frames_graph needs device-resident buffers")
        descs = _frame_descs(descs)
        if nbytes is None:
            nbytes = int(pixels_dev.numel())
        self._order_after_producer(pixels_dev, boxes_out, counts_out)
        self._check(self.lib.yolo_detect_frames_graph(self.ctx, p, nbytes, descs.ctypes.data, len(descs), fit, score_thr, iou_thr,
                                                      max_out, nms_mode, select_mode, units, bp, cp), "yolo_detect_frames_graph")

    # ---- JPEG files: entropy-decoded on the host, IDCT on the device, read as frames (chroma upsampling and colour inside the fit launch) ----
    def decode_jpegs(self, files):
        """files: a list of JPEG files, each a bytes object or a path -> a JpegFrames handle over this engine's surface (yolo_decode_jpegs): one
        upload and one IDCT launch for the batch.  The handle goes wherever frames go; it is valid until the next decode on this engine."""
        f = _JpegFiles(files)
        descs = np.zeros(f.n, dtype=FRAME_DTYPE)
        pixels, nbytes = C.c_void_p(), C.c_size_t()
        self._check(self.lib.yolo_decode_jpegs(self.ctx, f.ptrs, f.sizes, f.n, descs.ctypes.data, C.byref(pixels), C.byref(nbytes)), "yolo_decode_jpegs")
        return JpegFrames(pixels.value, nbytes.value, descs)

    def jpeg_decode_times(self):
        """What this engine's last decode cost (yolo_jpeg_decode_times): {"entropy_ms": host wall time of the entropy stage, "upload_ms" and
        "idct_ms": device time of the upload and of the IDCT launch, "upload_bytes"}.  Waits for the IDCT."""
        e, u, i, b = C.c_double(), C.c_double(), C.c_double(), C.c_size_t()
        self._check(self.lib.yolo_jpeg_decode_times(self.ctx, C.byref(e), C.byref(u), C.byref(i), C.byref(b)), "yolo_jpeg_decode_times")
        return {"entropy_ms": e.value, "upload_ms": u.value, "idct_ms": i.value, "upload_bytes": b.value}

    def set_jpeg_entropy(self, mode):
        """Who Huffman-decodes the files of decode_jpegs and every *_jpegs method (yolo_set_jpeg_entropy): "host" (the default) -- host threads, every file --
        or "auto" -- files with restart intervals on the device, one lane per interval, the others on the host, in one call.  Same results, same refusals."""
        if mode not in _JPEG_ENTROPY and mode not in _JPEG_ENTROPY.values():
            raise YoloError("set_jpeg_entropy: mode %r (\"host\" or \"auto\")" % (mode,))
        self._check(self.lib.yolo_set_jpeg_entropy(self.ctx, _JPEG_ENTROPY.get(mode, mode)), "yolo_set_jpeg_entropy")

    @property
    def jpeg_entropy(self):
        """"host" or "auto": the mode set_jpeg_entropy set"""
        return "auto" if self.lib.yolo_jpeg_entropy(self.ctx) == JPEG_ENTROPY_AUTO else "host"

    def jpeg_entropy_times(self):
        """What the entropy stage of this engine's last decode did (yolo_jpeg_entropy_times): {"device_files", "host_files", "intervals" decoded on the
        device, "scan_ms": host wall time of the interval scan, "device_ms": device time of k_jpeg_entropy, "stream_bytes": file bytes uploaded}."""
        d, h, i, s, k, b = C.c_int(), C.c_int(), C.c_int(), C.c_double(), C.c_double(), C.c_size_t()
        self._check(self.lib.yolo_jpeg_entropy_times(self.ctx, C.byref(d), C.byref(h), C.byref(i), C.byref(s), C.byref(k), C.byref(b)), "yolo_jpeg_entropy_times")
        return {"device_files": d.value, "host_files": h.value, "intervals": i.value, "scan_ms": s.value, "device_ms": k.value, "stream_bytes": b.value}

    def forward_jpegs(self, files, fit=FIT_STRETCH, want_detections=True):
        """forward_frames over JPEG files (yolo_forward_jpegs): decode, fit, forward.  Returns the decoded tensor [n, rows, attrs]."""
        f = _JpegFiles(files)
        det = np.empty((f.n, self.rows, self.attrs), dtype=np.float32) if want_detections else None
        self._check(self.lib.yolo_forward_jpegs(self.ctx, f.ptrs, f.sizes, f.n, fit, det.ctypes.data if det is not None else None, HOST), "yolo_forward_jpegs")
        return det

    def detect_jpegs(self, files, fit=FIT_STRETCH, units=UNITS_NETWORK, score_thr=0.5, iou_thr=0.5, max_out=20, nms_mode=NMS_TF, select_mode=SELECT_GT,
                     hier_thresh=None):
        """detect_frames over JPEG files (yolo_detect_jpegs) -> list of BOX_DTYPE arrays; UNITS_SOURCE_PIXELS: in the picture's own pixels."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        f = _JpegFiles(files)
        boxes = np.zeros((f.n, max_out), dtype=BOX_DTYPE); counts = np.zeros(f.n, dtype=np.int32)
        self._check(self.lib.yolo_detect_jpegs(self.ctx, f.ptrs, f.sizes, f.n, fit, score_thr, iou_thr, max_out, nms_mode, select_mode, units,
                                               boxes.ctypes.data, counts.ctypes.data, HOST), "yolo_detect_jpegs")
        return [boxes[i, :counts[i]].copy() for i in range(f.n)]

    def detect_tiled_jpegs(self, files, tile=None, overlap=(64, 64), fit=FIT_STRETCH, relative=False, score_thr=0.5, iou_thr=0.5, max_out=20,
                           nms_mode=NMS_TF, select_mode=SELECT_GT):
        """detect_tiled_frames over JPEG files (yolo_detect_tiled_jpegs).  Arguments and records as detect_tiled."""
        f = _JpegFiles(files)
        th, tw = (0, 0) if tile is None else _pair(tile, "tile")
        oh, ow = _pair(overlap, "overlap")
        boxes = np.zeros((f.n, max_out), dtype=BOX_DTYPE); counts = np.zeros(f.n, dtype=np.int32)
        self._check(self.lib.yolo_detect_tiled_jpegs(self.ctx, f.ptrs, f.sizes, f.n, th, tw, oh, ow, fit, score_thr, iou_thr, max_out, nms_mode,
                                                     select_mode, 1 if relative else 0, boxes.ctypes.data, counts.ctypes.data, HOST), "yolo_detect_tiled_jpegs")
        return [boxes[i, :counts[i]].copy() for i in range(f.n)]

    # ---- classifier networks (a cfg whose output layer is a [softmax]) ----
    @property
    def num_classes(self):
        """Outputs of the [softmax] layer of a classifier; for a detector, attrs - 5 (yolo_num_classes)."""
        return self.lib.yolo_num_classes(self.ctx)

    def _classify_result(self, n, top_k):
        if top_k:
            return np.full((n, top_k), -1, dtype=np.int32), np.zeros((n, top_k), dtype=np.float32)
        return None, np.zeros((n, max(self.num_classes, 0)), dtype=np.float32)

    def classify(self, images, top_k=5, scale=1.0 / 255.0):
        """images as for `forward`.  top_k > 0: -> (classes int32 [n, top_k], probs float32 [n, top_k]), probability descending, equal
        probabilities by ascending class -- selected on the device, only these records are copied; top_k == 0: -> the whole
        probability matrix float32 [n, num_classes]."""
        self._check_channels(images)
        p, loc = _ptr(images)
        self._last_image = images if loc == DEVICE else None
        self._order_after_producer(images)
        n = int(images.shape[0])
        fmt = IMG_U8 if str(images.dtype).endswith("uint8") else IMG_F32
        cls, probs = self._classify_result(n, top_k)
        self._check(self.lib.yolo_classify(self.ctx, p, n, fmt, loc, scale, top_k, cls.ctypes.data if top_k else None, probs.ctypes.data, HOST),
                    "yolo_classify")
        return (cls, probs) if top_k else probs

    def classify_images(self, images, fit=FIT_STRETCH, top_k=5):
        """`classify` over a list of uint8 [h, w, input_channels] images of any sizes, RGB unless the cfg says otherwise (or a (buffer, descs) pair from pack_images), fitted on
        the device in one launch (yolo_classify_images_u8)."""
        buf, descs, p, loc, nbytes = self._packed(images)
        n = len(descs)
        self._order_after_producer(buf)
        cls, probs = self._classify_result(n, top_k)
        self._check(self.lib.yolo_classify_images_u8(self.ctx, p, nbytes, descs.ctypes.data, n, fit, loc, top_k,
                                                     cls.ctypes.data if top_k else None, probs.ctypes.data, HOST), "yolo_classify_images_u8")
        return (cls, probs) if top_k else probs

    def classify_views(self, images, views, fit=FIT_STRETCH, shift=32, scale=1.0, top_k=0):
        """yolo_classify_views_u8: every image (a list of uint8 [h, w, input_channels] arrays of any sizes and any number, or a (buffer, descs) pair
        from pack_images) is predicted over the views of `views` -- VIEWS_FLIP: the image fitted by `fit` and its mirror; VIEWS_TEN_CROP: darknet's ten
        crops of the image resized to network + shift (view_table states them; `fit` is not read) --, the slots image * K + view run max_batch at a
        time, and one launch adds each image's rows in view order, multiplies by `scale` (1 / K: the mean) and selects.  top_k == 0: -> the sums
        float32 [n, num_classes]; top_k > 0: -> (classes int32 [n, top_k], sums float32 [n, top_k]), value descending, equal values by ascending class."""
        buf, descs, p, loc, nbytes = self._packed(images)
        n = len(descs)
        self._order_after_producer(buf)
        cls, probs = self._classify_result(n, max(int(top_k), 0))          # (a negative top_k: the library refuses it)
        self._check(self.lib.yolo_classify_views_u8(self.ctx, p, nbytes, descs.ctypes.data, n, int(views), int(fit), int(shift), loc, float(scale), int(top_k),
                                                    cls.ctypes.data if cls is not None else None, probs.ctypes.data, HOST), "yolo_classify_views_u8")
        return (cls, probs) if top_k else probs

    # ---- classifiers over decoded video frames and JPEG files: the frame fit, no RGB copy of a frame anywhere ----
    def classify_frames(self, frames, fit=FIT_STRETCH, top_k=5):
        """`classify_images` over a list of Frame (or a (buffer, descs) pair from pack_frames, the buffer on the host or the device; or a decode_jpegs
        handle): one launch converts and fits every frame (`fit`: any but FIT_CV2_BGR), then the classifier tail (yolo_classify_frames_u8).  Bit-equal
        to classify_images over frame_to_rgb of the frames."""
        buf, descs, p, loc, nbytes = self._packed_frames(frames)
        n = len(descs)
        self._order_after_producer(buf)
        cls, probs = self._classify_result(n, top_k)
        self._check(self.lib.yolo_classify_frames_u8(self.ctx, p, nbytes, descs.ctypes.data, n, fit, loc, top_k,
                                                     cls.ctypes.data if top_k else None, probs.ctypes.data, HOST), "yolo_classify_frames_u8")
        return (cls, probs) if top_k else probs

    def classify_views_frames(self, frames, views, fit=FIT_STRETCH, shift=32, scale=1.0, top_k=0):
        """`classify_views` over frames (yolo_classify_views_frames_u8): any number of them; every view is fitted straight from its frame's planes, chroma
        indexed by the pixel's position in the frame.  Arguments and results as classify_views."""
        buf, descs, p, loc, nbytes = self._packed_frames(frames)
        n = len(descs)
        self._order_after_producer(buf)
        cls, probs = self._classify_result(n, max(int(top_k), 0))          # (a negative top_k: the library refuses it)
        self._check(self.lib.yolo_classify_views_frames_u8(self.ctx, p, nbytes, descs.ctypes.data, n, int(views), int(fit), int(shift), loc, float(scale), int(top_k),
                                                           cls.ctypes.data if cls is not None else None, probs.ctypes.data, HOST), "yolo_classify_views_frames_u8")
        return (cls, probs) if top_k else probs

    def classify_jpegs(self, files, fit=FIT_STRETCH, top_k=5):
        """classify_frames over JPEG files (bytes objects or paths; yolo_classify_jpegs): decode, fit, classify.  fit=FIT_CENTER_CROP: darknet's
        `classifier predict` from a file."""
        f = _JpegFiles(files)
        cls, probs = self._classify_result(f.n, top_k)
        self._check(self.lib.yolo_classify_jpegs(self.ctx, f.ptrs, f.sizes, f.n, fit, top_k, cls.ctypes.data if top_k else None, probs.ctypes.data, HOST),
                    "yolo_classify_jpegs")
        return (cls, probs) if top_k else probs

    def classify_views_jpegs(self, files, views, fit=FIT_STRETCH, shift=32, scale=1.0, top_k=0):
        """classify_views_frames over JPEG files (yolo_classify_views_jpegs): one decode batch for all the files -- darknet's `classifier valid10` over files."""
        f = _JpegFiles(files)
        cls, probs = self._classify_result(f.n, max(int(top_k), 0))
        self._check(self.lib.yolo_classify_views_jpegs(self.ctx, f.ptrs, f.sizes, f.n, int(views), int(fit), int(shift), float(scale), int(top_k),
                                                       cls.ctypes.data if cls is not None else None, probs.ctypes.data, HOST), "yolo_classify_views_jpegs")
        return (cls, probs) if top_k else probs

    # ---- map networks ([net] yolo_output=map): segmentation masks, heat maps ----
    def map_geometry(self):
        """(h, w, c) of the output map (yolo_output_map_geometry); YoloError on a detector or a classifier."""
        h, w, ch = C.c_int(), C.c_int(), C.c_int()
        self._check(self.lib.yolo_output_map_geometry(self.ctx, C.byref(h), C.byref(w), C.byref(ch)), "yolo_output_map_geometry")
        return h.value, w.value, ch.value

    def output_map(self, n):
        """The map of images 0..n-1 of the last forward (forward / forward_images with want_detections=False): [n, h, w, c] float32."""
        out = np.empty((n,) + self.map_geometry(), dtype=np.float32)
        self._check(self.lib.yolo_output_map(self.ctx, n, out.ctypes.data, out.size), "yolo_output_map")
        return out

    def label_map(self, n, thresh=0.5):
        """Per map pixel of those images the arg-max over the channels (the lowest index wins a tie), 255 where the maximum is below
        thresh: [n, h, w] uint8 (yolo_label_map)."""
        h, w, _ = self.map_geometry()
        out = np.empty((n, h, w), dtype=np.uint8)
        self._check(self.lib.yolo_label_map(self.ctx, n, float(thresh), out.ctypes.data), "yolo_label_map")
        return out

    def segment_images(self, images, fit=FIT_LETTERBOX, thresh=0.5):
        """images: a list of uint8 RGB [h_i, w_i, 3] arrays of any sizes -> a list of [h_i, w_i] uint8 label arrays, each at its image's own
        size: one fit launch, one forward, one label kernel (yolo_segment_images_u8; include/yolo_hip.h states the pixel mapping)."""
        buf, descs = pack_images(images, self._image_channels())
        d = _descs(descs)
        sizes = [int(q["h"]) * int(q["w"]) for q in d]
        labels = np.empty(sum(sizes), dtype=np.uint8)
        self._check(self.lib.yolo_segment_images_u8(self.ctx, buf.ctypes.data, d.ctypes.data, len(d), fit, float(thresh), labels.ctypes.data, None), "yolo_segment_images_u8")
        out, lo = [], 0
        for q, sz in zip(d, sizes):
            out.append(labels[lo:lo + sz].reshape(int(q["h"]), int(q["w"])).copy()); lo += sz
        return out

    @staticmethod
    def _split_labels(labels, hw):
        out, lo = [], 0
        for h, w in hw:
            out.append(labels[lo:lo + h * w].reshape(h, w).copy()); lo += h * w
        return out

    def segment_frames(self, frames, fit=FIT_LETTERBOX, thresh=0.5):
        """segment_images over frames (a list of Frame, a (buffer, descs) pair with the buffer on the host or the device, or a decode_jpegs handle) -> a
        list of [h_i, w_i] uint8 label arrays, each at its frame's own size (yolo_segment_frames_u8)."""
        buf, descs, p, loc, nbytes = self._packed_frames(frames)
        hw = [(max(int(q["h"]), 0), max(int(q["w"]), 0)) for q in descs]
        self._order_after_producer(buf)
        labels = np.empty(sum(h * w for h, w in hw), dtype=np.uint8)
        self._check(self.lib.yolo_segment_frames_u8(self.ctx, p, nbytes, descs.ctypes.data, len(descs), fit, loc, float(thresh), labels.ctypes.data, None),
                    "yolo_segment_frames_u8")
        return self._split_labels(labels, hw)

    def segment_jpegs(self, files, fit=FIT_LETTERBOX, thresh=0.5):
        """segment_frames over JPEG files (bytes objects or paths; yolo_segment_jpegs): labels at each picture's own size."""
        f = _JpegFiles(files)
        hw = []
        for d in f.data:
            info = _JpegInfo()
            ok = self.lib.yolo_jpeg_info(d, len(d), C.byref(info)) == 0          # (a file that is not served: the entry point refuses it, by its index)
            hw.append((info.h, info.w) if ok else (0, 0))
        labels = np.empty(sum(h * w for h, w in hw), dtype=np.uint8)
        self._check(self.lib.yolo_segment_jpegs(self.ctx, f.ptrs, f.sizes, f.n, fit, float(thresh), labels.ctypes.data, None), "yolo_segment_jpegs")
        return self._split_labels(labels, hw)

    def darknet_boxes(self, image, w, h, thresh=0.5, relative=1, cap=None, hier_thresh=None, map200=None):
        """darknet's get_network_boxes over image `image` of the last forward (yolo_darknet_boxes_at) -> records [count, 5 + classes]
        (x, y, w, h, objectness, prob[classes]), un-letterboxed for a w x h source image.  A tree head: hier_thresh (None: the
        context's), map200 the 200 class indices of the `map` form (yolo_darknet_boxes_map)."""
        if hier_thresh is not None:
            self.set_hier_thresh(hier_thresh)
        m = None if map200 is None else np.ascontiguousarray(map200, dtype=np.int32)
        if m is not None and m.size != 200:
            raise YoloError("map200 needs exactly 200 entries")
        mp = None if m is None else m.ctypes.data
        cnt = C.c_int(0)
        self._check(self.lib.yolo_darknet_boxes_map(self.ctx, image, w, h, thresh, relative, mp, None, 0, C.byref(cnt)), "yolo_darknet_boxes_at")
        cap = cnt.value if cap is None else cap
        rec = np.zeros((max(cap, 1), self.attrs), dtype=np.float32)
        self._check(self.lib.yolo_darknet_boxes_map(self.ctx, image, w, h, thresh, relative, mp, rec.ctypes.data, cap, C.byref(cnt)),
                    "yolo_darknet_boxes_at")
        return rec[:min(cnt.value, cap)]

    def synchronize(self):
        self._check(self.lib.yolo_synchronize(self.ctx), "yolo_synchronize")

    # ---- recurrent networks ([rnn] / [gru] / [lstm]): one call is one time step, batch index b is stream b (include/yolo_hip.h) ----
    @property
    def num_state_tensors(self):
        return self.lib.yolo_num_state_tensors(self.ctx)

    def state_geometry(self, k):
        """(layer index, floats per stream) of state tensor k"""
        layer, n = C.c_int(0), C.c_size_t(0)
        self._check(self.lib.yolo_state_geometry(self.ctx, k, C.byref(layer), C.byref(n)), "yolo_state_geometry")
        return layer.value, n.value

    def state(self, k, stream):
        out = np.empty(self.state_geometry(k)[1], dtype=np.float32)
        self._check(self.lib.yolo_get_state(self.ctx, k, stream, out.ctypes.data, out.size), "yolo_get_state")
        return out

    def set_state(self, k, stream, values):
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        self._check(self.lib.yolo_set_state(self.ctx, k, stream, v.ctypes.data, v.size), "yolo_set_state")

    def reset_state(self, stream=None):
        """zero the states of one stream, or of every stream (darknet's reset_network_state)"""
        self._check(self.lib.yolo_reset_state(self.ctx, -1 if stream is None else int(stream)), "yolo_reset_state")

    # ---- frame-averaged detection on video streams (darknet's `detector demo`; include/yolo_hip.h) ----
    def set_frame_average(self, frames):
        """frames = K in 1 .. 8 (1: off).  With K >= 2 every forward* / detect* call with n images is one time step of the streams 0 .. n-1:
        the boxes are decoded from the mean of the heads' activated outputs over the stream's last K steps.  The slots start as zeros (and
        again after reset_state), so a stream's first K-1 results are attenuated, as in darknet's demo."""
        self._check(self.lib.yolo_set_frame_average(self.ctx, int(frames)), "yolo_set_frame_average")

    def frame_average(self):
        """the current K (1: off)"""
        return self.lib.yolo_frame_average(self.ctx)

    # ---- vector-input networks ([net] yolo_input=vector, inputs=N: char-rnn; include/yolo_hip.h) ----
    @property
    def vector_inputs(self):
        """N of a vector-input network, 0 for an image network"""
        return self.lib.yolo_vector_inputs(self.ctx)

    def forward_vectors(self, x):
        """one step of streams 0 .. n-1 over x, float32 [n, N] -> the output layer's probabilities [n, classes]"""
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.vector_inputs:
            raise YoloError("forward_vectors: need a float32 [n, %d] array, got %s" % (self.vector_inputs, x.shape))
        out = np.empty((x.shape[0], self.lib.yolo_num_classes(self.ctx)), dtype=np.float32)
        self._check(self.lib.yolo_forward_vectors(self.ctx, x.ctypes.data, x.shape[0], HOST, out.ctypes.data, out.size), "yolo_forward_vectors")
        return out

    def sequence(self, tokens, steps, uniforms=None, clip=1e-4, want_probs=False):
        """yolo_sequence over host arrays.  tokens: int32 [forced, n] (or [forced]: one stream), fed at the steps 0 .. forced-1; uniforms: float32
        [steps - forced + 1, n] (or one-dimensional for one stream), or None with steps == forced (teacher forcing: nothing is sampled).
        -> sampled tokens int32 [steps - forced + 1, n] (None without uniforms), or (tokens, probs float32 [steps, n, N]) with want_probs.
        clip: probabilities below it (p < clip, in floats) are not drawn.  The default is the float 1e-4; darknet's rnn.c:291 compares with the
        DOUBLE .0001, which also removes p == 1e-4f: char_rnn.CharRNN.CLIP is the float bound that reproduces darknet exactly."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        if tok.ndim == 1:
            tok = tok.reshape(-1, 1)
        forced, n = tok.shape if tok.ndim == 2 else (0, 0)
        uni = out = probs = None
        if uniforms is not None:
            uni = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1, max(n, 1))
            if uni.shape[0] != steps - forced + 1:
                raise YoloError("sequence: %d steps with %d forced tokens need uniforms [%d, %d], got %s" % (steps, forced, steps - forced + 1, n, uni.shape))
            out = np.full(uni.shape, -1, dtype=np.int32)
        if want_probs:
            probs = np.empty((max(steps, 0), n, self.vector_inputs), dtype=np.float32)
        self._check(self.lib.yolo_sequence(self.ctx, n, steps, tok.ctypes.data, forced, uni.ctypes.data if uni is not None else None, float(clip),
                                           out.ctypes.data if out is not None else None, probs.ctypes.data if probs is not None else None, HOST), "yolo_sequence")
        return (out, probs) if want_probs else out

    def set_temperature(self, t):
        """the temperature of every [softmax] layer (darknet's rnn.c:261), until it is set again or reset_temperature is called"""
        self._check(self.lib.yolo_set_temperature(self.ctx, float(t)), "yolo_set_temperature")

    def reset_temperature(self):
        """every [softmax] layer back to the temperature its cfg section names"""
        self._check(self.lib.yolo_reset_temperature(self.ctx), "yolo_reset_temperature")

    # ---- introspection / measurement ----
    def layer_output(self, index, n):
        dims = (C.c_int * 3)()
        self._check(self.lib.yolo_layer_output(self.ctx, index, n, None, 0, dims), "yolo_layer_output")
        out = np.empty((n, dims[0], dims[1], dims[2]), dtype=np.float32)
        self._check(self.lib.yolo_layer_output(self.ctx, index, n, out.ctypes.data, out.size, dims), "yolo_layer_output")
        return out

    def staged_input(self, n):
        """The staged network input of images 0..n-1 of the last forward, every stored channel of a pixel: [n, H, W, S] float32, S = 8 for an
        RGB network, roundup(input_channels, 8) for a network of planes (yolo_staged_input)."""
        dims = (C.c_int * 3)()
        self._check(self.lib.yolo_staged_input(self.ctx, n, None, 0, dims), "yolo_staged_input")
        out = np.empty((n, dims[0], dims[1], dims[2]), dtype=np.float32)
        self._check(self.lib.yolo_staged_input(self.ctx, n, out.ctypes.data, out.size, dims), "yolo_staged_input")
        return out

    def conv_flops(self):
        return self.lib.yolo_conv_flops(self.ctx)

    def conv_bytes(self, n):
        return self.lib.yolo_conv_bytes(self.ctx, n)

    def time_forward(self, n, iters, conv=True):
        t, c = C.c_float(0), C.c_float(0)
        self._check(self.lib.yolo_time_forward(self.ctx, n, iters, C.byref(t), C.byref(c) if conv else None), "yolo_time_forward")
        return t.value, (c.value if conv else None)

    def time_layers(self, n, iters):
        ms = np.zeros(self.num_layers, dtype=np.float32)
        self._check(self.lib.yolo_time_layers(self.ctx, n, iters, ms.ctypes.data_as(C.POINTER(C.c_float))), "yolo_time_layers")
        return ms

    def autotune(self, n, iters=3):
        self._check(self.lib.yolo_autotune(self.ctx, n, iters), "yolo_autotune")

    def get_tile_configs(self):
        cfgs = np.full(self.num_layers, -1, dtype=np.int32)
        self._check(self.lib.yolo_get_tile_configs(self.ctx, cfgs.ctypes.data), "yolo_get_tile_configs")
        return cfgs

    def set_tile_configs(self, cfgs):
        cfgs = np.ascontiguousarray(cfgs, dtype=np.int32)
        if cfgs.size != self.num_layers:
            raise YoloError("need %d tile configs, got %d" % (self.num_layers, cfgs.size))
        self._check(self.lib.yolo_set_tile_configs(self.ctx, cfgs.ctypes.data), "yolo_set_tile_configs")

    def resolved_tile_configs(self, n):
        """the id every layer would launch at batch n under the current plan (-1: not a tunable conv layer); see include/yolo_hip.h"""
        out = np.full(self.num_layers, -1, dtype=np.int32)
        self._check(self.lib.yolo_resolved_tile_configs(self.ctx, n, out.ctypes.data), "yolo_resolved_tile_configs")
        return out


# ---- single operators (host buffers in, host buffers out; production kernels underneath) ----------
def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def op_conv2d(x, w_hwio, bias=None, stride=1, act=0, residual=None, dtype=BF16, tile_cfg=-1, device=0, padding=None):
    """the dense conv on host tensors: x [n, h, w, cin], w_hwio [k, k, cin, cout], k 1..11.  padding=None: k // 2 (darknet's pad=1); an
    explicit padding, or a k other than 1 and 3, goes through yolo_op_conv2d_pad"""
    l = load_library()
    x = _f32(x); w = _f32(w_hwio)
    n, h, wd, cin = x.shape
    k, _, _, cout = w.shape
    pad = k // 2 if padding is None else int(padding)
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    if ho < 1 or wo < 1 or pad < 0:
        raise YoloError("op_conv2d: a %d x %d filter with padding %d over a %d x %d input leaves no output pixel" % (k, k, pad, wd, h))
    out = np.empty((n, ho, wo, cout), dtype=np.float32)
    b = _f32(bias) if bias is not None else None
    r = _f32(residual) if residual is not None else None
    if padding is not None or k not in (1, 3):
        rc = l.yolo_op_conv2d_pad(x.ctypes.data, n, h, wd, cin, w.ctypes.data, b.ctypes.data if b is not None else None, k, stride, pad,
                                  cout, act, r.ctypes.data if r is not None else None, out.ctypes.data, dtype, tile_cfg, device)
        _op_check(rc, "yolo_op_conv2d_pad")
        return out
    rc = l.yolo_op_conv2d(x.ctypes.data, n, h, wd, cin, w.ctypes.data, b.ctypes.data if b is not None else None, k, stride,
                          cout, act, r.ctypes.data if r is not None else None, out.ctypes.data, dtype, tile_cfg, device)
    _op_check(rc, "yolo_op_conv2d")
    return out


def op_conv_num_cfgs():
    return load_library().yolo_op_conv_num_cfgs()


def calibrate(seconds=0.4, f16=False, device=0, stream=None):
    """yolo_calibrate: (TFLOP/s, GHz) this chip sustains on a register-resident MFMA loop (bf16, or fp16 with f16=True) -- the yardstick
    bench.py prints next to its roofline fraction so that lines measured on different boxes can be normalised."""
    t, g = C.c_float(0), C.c_float(0)
    _op_check(load_library().yolo_calibrate(device, _stream_handle(stream), 1 if f16 else 0, float(seconds), C.byref(t), C.byref(g)), "yolo_calibrate")
    return float(t.value), float(g.value)


def calibrate_copy(seconds=0.2, device=0, stream=None):
    """yolo_calibrate_copy: GB/s (read + written) of a streaming 1 GiB -> 1 GiB device copy -- the memory side of the box's yardstick."""
    g = C.c_float(0)
    _op_check(load_library().yolo_calibrate_copy(device, _stream_handle(stream), float(seconds), C.byref(g)), "yolo_calibrate_copy")
    return float(g.value)


def op_upsample2x(x, semantics=SEM_TF, device=0):
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty((n, 2 * h, 2 * w, c), dtype=np.float32)
    _op_check(load_library().yolo_op_upsample2x(x.ctypes.data, n, h, w, c, semantics, out.ctypes.data, device), "yolo_op_upsample2x")
    return out


def op_reorg(x, stride=2, semantics=SEM_TF, device=0):
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty((n, h // stride, w // stride, c * stride * stride), dtype=np.float32)
    _op_check(load_library().yolo_op_reorg(x.ctypes.data, n, h, w, c, stride, semantics, out.ctypes.data, device), "yolo_op_reorg")
    return out


def op_maxpool(x, size=2, stride=2, device=0):
    x = _f32(x); n, h, w, c = x.shape
    pad = (size - 1) // 2
    out = np.empty((n, (h + 2 * pad) // stride, (w + 2 * pad) // stride, c), dtype=np.float32)
    _op_check(load_library().yolo_op_maxpool(x.ctypes.data, n, h, w, c, size, stride, out.ctypes.data, device), "yolo_op_maxpool")
    return out


def op_avgpool(x, dtype=FP32, device=0):
    """darknet's (global) [avgpool] of x [n, h, w, c], stored as `dtype` first -> [n, c] float32."""
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty((n, c), dtype=np.float32)
    _op_check(load_library().yolo_op_avgpool(x.ctypes.data, n, h, w, c, dtype, out.ctypes.data, device), "yolo_op_avgpool")
    return out


ACTIVATIONS = ("linear", "leaky", "relu", "relie", "logistic", "loggy", "elu", "ramp", "tanh", "plse", "stair", "hardtan", "lhtan")


def activation_code(name):
    """The library's code of a darknet activation name (yolo_activation_code, the planner's mapping); YoloError for a name darknet does
    not know.  An int passes through."""
    if isinstance(name, (int, np.integer)):
        return int(name)
    code = load_library().yolo_activation_code(str(name).encode())
    if code < 0:
        raise YoloError("unknown activation '%s'" % name)
    return code


def op_activate(x, activation, dtype=FP32, device=0):
    """act(x) of x [n, h, w, c] by the kernel behind a layer whose activation is outside the conv epilogues' slope family (k_activate);
    x is stored as `dtype` first and the result is rounded to it -> float32 [n, h, w, c]."""
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty_like(x)
    _op_check(load_library().yolo_op_activate(x.ctypes.data, n, h, w, c, activation_code(activation), dtype, out.ctypes.data, device), "yolo_op_activate")
    return out


def op_shortcut(x, frm, activation="linear", dtype=FP32, device=0):
    """darknet's [shortcut]: act(x + gather(frm)), x [n, h2, w2, c2] the layer's input, frm [n, h1, w1, c1] the `from` tensor (the first
    min(c1, c2) channels, stride w1 // w2 or sample w2 // w1 as shortcut_cpu computes them), stored as `dtype` first -> float32 like x."""
    x = _f32(x); frm = _f32(frm); n, h2, w2, c2 = x.shape; n1, h1, w1, c1 = frm.shape
    if n1 != n:
        raise ValueError("op_shortcut: batch sizes differ")
    out = np.empty_like(x)
    _op_check(load_library().yolo_op_shortcut(x.ctypes.data, n, h2, w2, c2, frm.ctypes.data, h1, w1, c1, activation_code(activation), dtype,
                                              out.ctypes.data, device), "yolo_op_shortcut")
    return out


def _op_side_conv(entry, x, filters, bias, cout, geometry, out_hw, activation, dtype, out_f32, device):
    """The call behind op_deconv2d / op_conv2d_grouped / op_conv2d_xnor: C entry point `entry` over x [n, h, w, cin] and checked float32 filters of `cout`
    filters [., ., size, size]; `geometry`: the integers between `size` and the activation; out_hw: the output's height and width."""
    n, h, w, cin = x.shape
    b = _f32(bias) if bias is not None else None
    out = np.empty((n, max(out_hw[0], 0), max(out_hw[1], 0), cout), dtype=np.float32)
    _op_check(getattr(load_library(), entry)(x.ctypes.data, n, h, w, cin, filters.ctypes.data, b.ctypes.data if b is not None else None, filters.shape[2], *geometry,
                                             activation_code(activation), dtype, 1 if out_f32 else 0, out.ctypes.data, device), entry)
    return out


def op_deconv2d(x, w_iohw, bias=None, stride=1, padding=0, activation="linear", dtype=BF16, out_f32=False, device=0):
    """darknet's [deconvolutional] (yolo_op_deconv2d): x [n, h, w, cin], w_iohw [cin, cout, size, size] (the weight file's order) ->
    [n, (h - 1) stride + size - 2 padding, ..., cout] float32.  out_f32: the fp32 store of a 16-bit kernel."""
    x = _f32(x); w_iohw = _f32(w_iohw)
    n, h, w, cin = x.shape
    if w_iohw.ndim != 4 or w_iohw.shape[0] != cin or w_iohw.shape[2] != w_iohw.shape[3]:
        raise YoloError("op_deconv2d: filters must be [cin, cout, size, size]")
    cout, size = w_iohw.shape[1], w_iohw.shape[2]
    return _op_side_conv("yolo_op_deconv2d", x, w_iohw, bias, cout, (stride, padding, cout), [(d - 1) * stride + size - 2 * padding for d in (h, w)],
                         activation, dtype, out_f32, device)


def op_conv2d_grouped(x, w_oihw, bias=None, groups=1, stride=1, padding=0, activation="linear", dtype=BF16, out_f32=False, device=0):
    """darknet's [convolutional] with groups= (yolo_op_conv2d_grouped): x [n, h, w, cin], w_oihw [cout, cin / groups, size, size] (the
    weight file's order) -> [n, (h + 2 padding - size) // stride + 1, ..., cout] float32.  out_f32: the fp32 store of a 16-bit kernel."""
    x = _f32(x); w_oihw = _f32(w_oihw)
    n, h, w, cin = x.shape
    if w_oihw.ndim != 4 or groups < 1 or cin % groups or w_oihw.shape[1] != cin // groups or w_oihw.shape[2] != w_oihw.shape[3]:
        raise YoloError("op_conv2d_grouped: filters must be [cout, cin / groups, size, size]")
    cout, size = w_oihw.shape[0], w_oihw.shape[2]
    return _op_side_conv("yolo_op_conv2d_grouped", x, w_oihw, bias, cout, (stride, padding, cout, groups), [(d + 2 * padding - size) // stride + 1 for d in (h, w)],
                         activation, dtype, out_f32, device)


def op_conv2d_xnor(x, w_oihw, bias=None, stride=1, padding=0, activation="linear", dtype=BF16, out_f32=False, device=0):
    """darknet's [convolutional] with xnor=1 (yolo_op_conv2d_xnor): x [n, h, w, cin], rounded to `dtype` before its sign is taken (+1 where
    > 0, else -1; a tap outside the image: 0), w_oihw [cout, cin, size, size] (the weight file's order), used as mean|w_f| * sign(w) ->
    [n, (h + 2 padding - size) // stride + 1, ..., cout] float32.  out_f32: the fp32 store of a 16-bit configuration."""
    x = _f32(x); w_oihw = _f32(w_oihw)
    n, h, w, cin = x.shape
    if w_oihw.ndim != 4 or w_oihw.shape[1] != cin or w_oihw.shape[2] != w_oihw.shape[3]:
        raise YoloError("op_conv2d_xnor: filters must be [cout, cin, size, size]")
    cout, size = w_oihw.shape[0], w_oihw.shape[2]
    return _op_side_conv("yolo_op_conv2d_xnor", x, w_oihw, bias, cout, (stride, padding, cout), [(d + 2 * padding - size) // stride + 1 for d in (h, w)],
                         activation, dtype, out_f32, device)


def op_l2norm(x, dtype=FP32, device=0):
    """[l2norm]: per pixel x / sqrt(sum over the channels of x^2) (yolo_op_l2norm)."""
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty_like(x)
    _op_check(load_library().yolo_op_l2norm(x.ctypes.data, n, h, w, c, dtype, out.ctypes.data, device), "yolo_op_l2norm")
    return out


def op_lrn(x, size=5, alpha=1e-4, beta=0.75, kappa=1.0, dtype=FP32, device=0):
    """[normalization] / [lrn] over the channels of every pixel of x [n, h, w, c], as darknet computes it: x * (kappa + alpha * (W - g)) ** -beta, W the
    window's sum of squares, g the square of channel size // 2 (the one its running sum never adds) (yolo_op_lrn)."""
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty_like(x)
    _op_check(load_library().yolo_op_lrn(x.ctypes.data, n, h, w, c, int(size), float(alpha), float(beta), float(kappa), dtype, out.ctypes.data, device), "yolo_op_lrn")
    return out


def op_upsample(x, stride=2, scale=1.0, dtype=FP32, device=0):
    """darknet's [upsample]: nearest, out = scale * in (yolo_op_upsample)."""
    x = _f32(x); n, h, w, c = x.shape
    out = np.empty((n, h * max(stride, 0), w * max(stride, 0), c), dtype=np.float32)
    _op_check(load_library().yolo_op_upsample(x.ctypes.data, n, h, w, c, stride, float(scale), dtype, out.ctypes.data, device), "yolo_op_upsample")
    return out


def op_label_map(m, thresh=0.5, device=0):
    """[n, h, w, c] float32 map -> [n, h, w] uint8 labels: arg-max over the channels, 255 where the maximum is below thresh (yolo_op_label_map)."""
    m = _f32(m); n, h, w, c = m.shape
    out = np.empty((n, h, w), dtype=np.uint8)
    _op_check(load_library().yolo_op_label_map(m.ctypes.data, n, h, w, c, float(thresh), out.ctypes.data, device), "yolo_op_label_map")
    return out


def op_softmax(x, groups=1, temperature=1.0, top_k=0, device=0):
    """darknet's [softmax] of x [n, len] -> probs [n, len]; top_k > 0: -> (probs, classes int32 [n, top_k], top probs [n, top_k]) from
    the same launch."""
    x = _f32(x); n, ln = x.shape
    probs = np.empty((n, ln), dtype=np.float32)
    cls = np.full((n, max(top_k, 1)), -1, dtype=np.int32); tkp = np.zeros((n, max(top_k, 1)), dtype=np.float32)
    _op_check(load_library().yolo_op_softmax(x.ctypes.data, n, ln, groups, float(temperature), top_k, probs.ctypes.data,
                                             cls.ctypes.data if top_k else None, tkp.ctypes.data if top_k else None, device), "yolo_op_softmax")
    return (probs, cls, tkp) if top_k else probs


def op_view_reduce(rows, views, scale=1.0, top_k=0, device=0):
    """The reduction launch of multi-view classification alone (yolo_op_view_reduce): rows float32 [n * views, len], slot = image * views + view
    -> sums [n, len] = (((0 + row_0) + row_1) + ...) * scale; top_k > 0: -> (sums, classes int32 [n, top_k], top sums [n, top_k]) from the same
    launch, value descending, equal values by ascending class."""
    rows = _f32(rows); views = int(views); top_k = int(top_k)
    if rows.ndim != 2 or views < 1 or rows.shape[0] % views or rows.shape[0] < views:
        raise YoloError("op_view_reduce: rows [n * views, len] with views >= 1, got %s and views %d" % (rows.shape, views))
    n, ln = rows.shape[0] // views, rows.shape[1]
    sums = np.empty((n, ln), dtype=np.float32)
    cls = np.full((n, max(top_k, 1)), -1, dtype=np.int32); top = np.zeros((n, max(top_k, 1)), dtype=np.float32)
    _op_check(load_library().yolo_op_view_reduce(rows.ctypes.data, n, views, ln, float(scale), top_k, sums.ctypes.data,
                                                 cls.ctypes.data if top_k else None, top.ctypes.data if top_k else None, device), "yolo_op_view_reduce")
    return (sums, cls, top) if top_k else sums


def op_sample(probs, uniforms, clip=1e-4, device=0):
    """darknet's sampler (rnn.c:290-293 + sample_array) over probs float32 [n, len] and uniforms float32 [n] -> tokens int32 [n].  clip: as for
    Engine.sequence (char_rnn.CharRNN.CLIP reproduces darknet's comparison with the double .0001)"""
    probs = _f32(probs); uniforms = _f32(uniforms).reshape(-1); n, ln = probs.shape
    if uniforms.size != n:
        raise YoloError("op_sample: %d rows need %d uniforms, got %d" % (n, n, uniforms.size))
    out = np.full(n, -1, dtype=np.int32)
    _op_check(load_library().yolo_op_sample(probs.ctypes.data, n, ln, uniforms.ctypes.data, float(clip), out.ctypes.data, device), "yolo_op_sample")
    return out


def tree_read(path):
    """The library's reader of a darknet tree file (yolo_tree_read; no device needed) -> dict(n, groups, parent, child, group_offset,
    group_size, leaf); YoloError with the library's message for a file it refuses."""
    lib = load_library()
    n, g = C.c_int32(0), C.c_int32(0)
    err = C.create_string_buffer(512)
    rc = lib.yolo_tree_read(os.fsencode(path), C.byref(n), C.byref(g), None, None, None, None, None, err, 512)
    if rc != 0:
        raise YoloError("yolo_tree_read failed (%d): %s" % (rc, err.value.decode()))
    a = {k: np.zeros(n.value if k in ("parent", "child", "leaf") else g.value, dtype=np.int32) for k in ("parent", "child", "group_offset", "group_size", "leaf")}
    lib.yolo_tree_read(os.fsencode(path), None, None, a["parent"].ctypes.data, a["child"].ctypes.data, a["group_offset"].ctypes.data,
                       a["group_size"].ctypes.data, a["leaf"].ctypes.data, err, 512)
    a.update(n=n.value, groups=g.value)
    return a


def plan_check(cfg_text, dtype=BF16):
    """Parse and plan a cfg without a device (yolo_plan_check) -> (status, message); status 0: it plans."""
    err = C.create_string_buffer(1024)
    rc = load_library().yolo_plan_check(cfg_text.encode(), dtype, err, 1024)
    return rc, err.value.decode()


def plan_table(cfg_text, dtype=BF16, max_batch=1, keep_layers=False):
    """The plan of a cfg without a device (yolo_plan_table) -> (status, text): one line per layer (own kernel, fused launch and its
    launcher, folded shortcut, 1x1 tail, storage, buffer, first writer, last reader) and the buffer total; the planner's message when
    it refuses."""
    out, err = C.create_string_buffer(1 << 18), C.create_string_buffer(1024)
    rc = load_library().yolo_plan_table(cfg_text.encode(), dtype, max_batch, int(keep_layers), out, len(out), err, 1024)
    return rc, (err if rc else out).value.decode()


def plan_dump(cfg_text, dtype=BF16, max_batch=1, keep_layers=False):
    """Every field the planner writes, without a device (yolo_plan_dump) -> (status, text): a line per layer, a line per storage and
    the context's line; the planner's message when it refuses."""
    out, err = C.create_string_buffer(1 << 20), C.create_string_buffer(1024)
    rc = load_library().yolo_plan_dump(cfg_text.encode(), dtype, max_batch, int(keep_layers), out, len(out), err, 1024)
    return rc, (err if rc else out).value.decode()


def op_tree_softmax(x, tree_path, temperature=1.0, mode=HIER_CONDITIONAL, device=0):
    """x [n, len] logits -> [n, len]: one softmax per group of the tree (mode 0), the absolute probabilities (1), leaves only (2)."""
    x = _f32(x); out = np.empty_like(x)
    _op_check(load_library().yolo_op_tree_softmax(x.ctypes.data, x.shape[0], x.shape[1], os.fsencode(tree_path), temperature, mode, out.ctypes.data, device), "yolo_op_tree_softmax")
    return out


def op_tree_top(x, tree_path, hier_thresh=0.5, device=0):
    """x [n, nodes] raw logits -> int32 [n]: hierarchy_top_prediction of every row, walked from the root (the descent kernel)."""
    x = _f32(x); out = np.empty(x.shape[0], dtype=np.int32)
    _op_check(load_library().yolo_op_tree_top(x.ctypes.data, x.shape[0], os.fsencode(tree_path), hier_thresh, out.ctypes.data, device), "yolo_op_tree_top")
    return out


def op_resize_u8(img, size, post_scale=1.0, device=0):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    out = np.empty((size, size, 3), dtype=np.float32)
    _op_check(load_library().yolo_op_resize_u8(img.ctypes.data, img.shape[0], img.shape[1], size, post_scale, out.ctypes.data, device), "yolo_op_resize_u8")
    return out


def op_resize_u8_hw(img, out_hw, post_scale=1.0, device=0):
    """yolo_op_resize_u8_hw: the legacy-bilinear stretch of one uint8 [h,w,3] image to [out_h,out_w,3] float32."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = np.empty((oh, ow, 3), dtype=np.float32)
    _op_check(load_library().yolo_op_resize_u8_hw(img.ctypes.data, img.shape[0], img.shape[1], oh, ow, post_scale, out.ctypes.data, device), "yolo_op_resize_u8_hw")
    return out


def op_resize_cv2(img, out_hw, swap_rb=True, divisor=225.0, device=0):
    """yolo_op_resize_cv2: `cv2.resize(image.astype(float32)[, BGR -> RGB], (w, h)) / divisor` of one uint8 [h,w,3] image -> [oh,ow,3] float32."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    out = np.empty((int(out_hw[0]), int(out_hw[1]), 3), dtype=np.float32)
    _op_check(load_library().yolo_op_resize_cv2(img.ctypes.data, img.shape[0], img.shape[1], int(out_hw[0]), int(out_hw[1]), 1 if swap_rb else 0,
                                                float(divisor), out.ctypes.data, device), "yolo_op_resize_cv2")
    return out


def op_letterbox(image_chw, w, h, embed=True, device=0):
    """yolo_op_letterbox: darknet's letterbox_image (embed) or resize_image of a planar float [3, ih, iw] image -> [3, h, w]."""
    img = _f32(image_chw)
    out = np.empty((3, int(h), int(w)), dtype=np.float32)
    _op_check(load_library().yolo_op_letterbox(img.ctypes.data, img.shape[2], img.shape[1], int(w), int(h), 1 if embed else 0, out.ctypes.data, device), "yolo_op_letterbox")
    return out


def op_nms_detections(boxes_xywh, prob, objectness, thresh, by_objectness=False, device=0):
    """darknet do_nms_sort / do_nms_obj on arrays; returns (prob, objectness) after suppression."""
    b = _f32(boxes_xywh); p = _f32(prob).copy(); o = _f32(objectness).copy()
    n, classes = p.shape
    _op_check(load_library().yolo_op_nms_detections(b.ctypes.data, p.ctypes.data, o.ctypes.data, n, classes, thresh, 1 if by_objectness else 0, device), "yolo_op_nms_detections")
    return p, o


def op_detections_boxes(det, device=0):
    det = _f32(det); n, rows, attrs = det.shape
    out = np.empty_like(det)
    _op_check(load_library().yolo_op_detections_boxes(det.ctypes.data, n, rows, attrs, out.ctypes.data, device), "yolo_op_detections_boxes")
    return out


def op_decode(raw, anchors, classes, img_size, decode=DECODE_RATIO, region=False, device=0):
    raw = _f32(raw); n, g = raw.shape[0], raw.shape[1]
    anchors = _f32(anchors).reshape(-1)
    na = anchors.size // 2
    out = np.empty((n, g * g * na, 5 + classes), dtype=np.float32)
    _op_check(load_library().yolo_op_decode(raw.ctypes.data, n, g, na, classes, anchors.ctypes.data, img_size, decode,
                                            1 if region else 0, out.ctypes.data, device), "yolo_op_decode")
    return out


def op_decode_hw(raw, anchors, classes, img_hw, decode=DECODE_RATIO, region=False, device=0):
    """yolo_op_decode_hw: raw [n, gh, gw, na * (5 + classes)] of a network input of img_hw = (height, width) -> [n, gh * gw * na, 5 + classes]."""
    raw = _f32(raw); n, gh, gw = raw.shape[0], raw.shape[1], raw.shape[2]
    anchors = _f32(anchors).reshape(-1)
    na = anchors.size // 2
    out = np.empty((n, gh * gw * na, 5 + classes), dtype=np.float32)
    _op_check(load_library().yolo_op_decode_hw(raw.ctypes.data, n, gh, gw, na, classes, anchors.ctypes.data, int(img_hw[0]), int(img_hw[1]), decode,
                                               1 if region else 0, out.ctypes.data, device), "yolo_op_decode_hw")
    return out


def op_postprocess(det, score_thr, iou_thr, max_out, nms_mode=NMS_TF, select_mode=SELECT_GT, image_hw=None, corners=False, device=0,
                   return_rows=False):
    """det [n,rows,5+C] fp32 rows (cx,cy,w,h,obj,cls..) -- or (x0,y0,x1,y1,obj,cls..) with corners=True.
    return_rows=True: -> (records, rows): the row of `det` every kept record was formed from."""
    det = _f32(det); n, rows, attrs = det.shape
    mode = nms_mode
    if corners:
        select_mode |= 0x100
    if image_hw is not None:
        mode |= (int(image_hw[0]) << 8) | (int(image_hw[1]) << 20)
    boxes = np.zeros((n, max_out), dtype=BOX_DTYPE); counts = np.zeros(n, dtype=np.int32)
    ridx = np.full((n, max_out), -1, dtype=np.int32) if return_rows else None
    _op_check(load_library().yolo_op_postprocess_rows(det.ctypes.data, n, rows, attrs, score_thr, iou_thr, max_out, mode, select_mode,
                                                      boxes.ctypes.data, counts.ctypes.data, ridx.ctypes.data if return_rows else None, device),
              "yolo_op_postprocess")
    recs = [boxes[i, :counts[i]].copy() for i in range(n)]
    if return_rows:
        return recs, [ridx[i, :counts[i]].copy() for i in range(n)]
    return recs


# ---- include/yolo_dist.h: the image-sharded detect step behind the C ABI ----
def shard_bounds(global_batch, world_size, rank):
    """yolo_shard_bounds: (lo, hi) of rank's contiguous slice of the global batch."""
    first, count = C.c_int(0), C.c_int(0)
    _op_check(load_library().yolo_shard_bounds(global_batch, world_size, rank, C.byref(first), C.byref(count)), "yolo_shard_bounds")
    return first.value, first.value + count.value


def dist_split_records(gathered, world_size, global_batch, max_out):
    """yolo_dist_split_records: gathered int32 [world, flat] (host) -> (boxes [global_batch, max_out] records, counts [global_batch])."""
    lib = load_library()
    per = -(-global_batch // world_size)
    g = np.ascontiguousarray(gathered, dtype=np.int32)
    if g.size != world_size * lib.yolo_dist_flat_words(per, max_out):
        raise YoloError("gathered buffer holds %d words, %d ranks x %d expected" % (g.size, world_size, lib.yolo_dist_flat_words(per, max_out)))
    boxes = np.zeros((global_batch, max_out), dtype=BOX_DTYPE)
    counts = np.zeros(global_batch, dtype=np.int32)
    _op_check(lib.yolo_dist_split_records(g.ctypes.data, world_size, global_batch, max_out, boxes.ctypes.data, counts.ctypes.data),
              "yolo_dist_split_records")
    return boxes, counts


def dist_unique_id():
    """yolo_dist_unique_id: the 128 bytes rank 0 hands to every rank's ShardedDetector."""
    buf = (C.c_uint8 * 128)()
    _op_check(load_library().yolo_dist_unique_id(buf), "yolo_dist_unique_id (RCCL)")
    return bytes(buf)


class ShardedDetector(object):
    """yolo_dist_*: this rank's Engine bound to a communicator of `world_size` ranks.  detect(images) takes THIS rank's slice
    (device tensor) and returns the whole batch's per-image record arrays, in global image order, on every rank."""

    def __init__(self, engine, world_size, rank, unique_id, global_batch, max_out=20):
        self.lib = load_library()
        self.engine = engine
        self.global_batch, self.max_out, self.world_size, self.rank = global_batch, max_out, world_size, rank
        self.lo, self.hi = shard_bounds(global_batch, world_size, rank)
        err = C.create_string_buffer(512)
        idbuf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self.h = self.lib.yolo_dist_create(engine.ctx, world_size, rank, idbuf, None, global_batch, max_out, err, 512)
        if not self.h:
            raise YoloError("yolo_dist_create: " + err.value.decode())

    def detect(self, images, scale=1.0 / 255.0, score_thr=0.5, iou_thr=0.5, nms_mode=NMS_TF, select_mode=SELECT_GT):
        p, loc = _ptr(images)
        if self.hi > self.lo and (loc != DEVICE or int(images.shape[0]) != self.hi - self.lo):
            raise YoloError("rank %d serves images [%d, %d): a device tensor of that many images is needed" % (self.rank, self.lo, self.hi))
        self._images = images                       # the graph replays from this buffer: keep it alive
        fmt = IMG_U8
        if images is not None:                      # (a rank whose slice is empty -- more ranks than images -- only takes part in the gather)
            self.engine._order_after_producer(images)
            fmt = IMG_U8 if str(images.dtype).endswith("uint8") else IMG_F32
        boxes = np.zeros((self.global_batch, self.max_out), dtype=BOX_DTYPE)
        counts = np.zeros(self.global_batch, dtype=np.int32)
        self.engine._check(self.lib.yolo_dist_detect(self.h, p, fmt, scale, score_thr, iou_thr, nms_mode, select_mode,
                                                      boxes.ctypes.data, counts.ctypes.data), "yolo_dist_detect")
        return [boxes[i, :counts[i]].copy() for i in range(self.global_batch)]

    def close(self):
        """Destroy BEFORE the engine (include/yolo_dist.h): a later step would use a dead context.  (yolo_dist_destroy itself only needs the
        device number, which the handle keeps, so the order of two close() calls cannot crash.)"""
        if self.h:
            self.lib.yolo_dist_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass
