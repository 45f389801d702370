/* libyolo_hip.so -- C ABI of the MI355X (gfx950) YOLO inference hot path.
 *
 * Drop-in boundary for the reference's "process -> runtime" call (`sess.run([...], feed_dict)`:
 * V3/YOLO_V3_inference.py:106-107, V3/convert_ckpt_and_inference.py:88, V2/YOLO_v2.py:55,
 * D2T/YOLO_V3_convert_darkenet_to_Tensorflow.py:588) and, on the C side, for the entry points the
 * reference's own ctypes binding uses (D2T/darknet.py:48-115 over D2T/include/darknet.h):
 *
 *   reference                                              this library
 *   ---------------------------------------------------    ---------------------------------------
 *   load_network(cfg, weights, clear)   DN/network.c:53     yolo_create + yolo_load_darknet_weights
 *   load_weights(var_list, file)        V3/yolo_v3.py:270   yolo_load_darknet_weights / yolo_set_weights
 *   network_predict(net, float*)        DN/network.c:497    yolo_forward
 *   sess.run(detections)                V3/yolo_v3.py:266   yolo_forward(..., detections_out)
 *   get_network_boxes + do_nms_sort     DN/network.c:562,   yolo_postprocess / yolo_detect
 *     / tf.image.non_max_suppression    DN/box.c:58, V3/YOLOV3.py:364-379
 *   free_network                        DN/network.c:716    yolo_destroy
 *   error(): perror+exit                DN/utils.c:253      int return code + yolo_last_error()
 *
 * Conventions: extern "C", plain pointers and sizes, caller-owned output buffers (no callee malloc
 * on the hot path, unlike make_network_boxes DN/network.c:526-540), every call returns YOLO_OK or a
 * negative code and never exits the process.  A context is single-threaded and bound to one HIP
 * device + stream; one context per GPU.  Activations are NHWC; images are NHWC RGB.
 */
#ifndef YOLO_HIP_H
#define YOLO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct yolo_ctx yolo_ctx;

enum yolo_status {
    YOLO_OK = 0,
    YOLO_ERR_INVALID = -1,     /* bad argument / malformed cfg */
    YOLO_ERR_HIP = -2,         /* HIP runtime error (text in yolo_last_error) */
    YOLO_ERR_STATE = -3,       /* call order (e.g. forward before weights) */
    YOLO_ERR_NOMEM = -4,
    YOLO_ERR_IO = -5,          /* weights file missing / wrong length */
    YOLO_ERR_UNSUPPORTED = -6
};

/* storage/compute type of the conv stack.  YOLO_FP8 (BASELINE config 5): OCP e4m3 filters and activations on the
 * fp8 MFMA (fp32 accumulation, heads in fp32, first conv in bf16); scheme and scales: DESIGN.md "fp8 scheme". */
enum yolo_dtype { YOLO_BF16 = 0, YOLO_FP32 = 1, YOLO_FP8 = 2,
                  YOLO_FP16 = 3,    /* IEEE fp16 filters and activations on v_mfma_f32_16x16x32_f16: the bf16 configuration's kernels,
                                     * tile plans and MFMA rate with an 11-bit significand instead of 8 (values saturate at +-65504);
                                     * what it buys in box accuracy: DESIGN.md section 4 */
                  YOLO_FP16X2 = 4 };/* split fp16 (round 4): every filter and stored activation is a PAIR of fp16 numbers hi = f16(v),
                                     * lo = f16(v - hi) -- 22 significant bits -- and a conv forms W_hi x_hi + W_hi x_lo + W_lo x_hi on the
                                     * fp16 MFMA with fp32 accumulation (three products per algorithmic one, W_lo x_lo is dropped).  The
                                     * configuration that meets north_star's IoU >= 0.999 on weights with a trained file's statistics at
                                     * several times the exact-fp32 path's rate; shortcuts are folded into the conv epilogues, the stem /
                                     * residual-block / 1x1-tail fusions are off on tensors stored as pairs; [connected] / [local] layers are
                                     * not served.  Mixed plans (round 5): `yolo_pair=0` on a [convolutional] section stores that layer's
                                     * output -- and what is derived from it without arithmetic -- as PLAIN fp16 (`yolo_pair_input=0` in
                                     * [net]: the image); a conv that reads a plain tensor runs one MFMA product per algorithmic one, and
                                     * stretches of plain tensors are served by the fp16 configuration's fused kernels.  Both operands of
                                     * a shortcut and all inputs of a concatenation share one form.  DESIGN.md section 3.6 */
enum yolo_semantics { YOLO_SEM_TF = 0, YOLO_SEM_DARKNET = 1 };
/* TF: bilinear `_upsample` (V3/yolo_v3.py:162-192) + tf.space_to_depth (V2/model_darknet19_slim.py:44);
 * DARKNET: nearest upsample (DN/blas.c:334) + reorg_cpu (DN/blas.c:9) -- lets the whole network be
 * checked against the compiled reference. */
enum yolo_decode { YOLO_DECODE_RATIO = 0, YOLO_DECODE_PIXEL = 1 };
/* RATIO: `_ratio_detection_layer` V3/YOLOV3.py:168-238 (normalised); PIXEL: `_detection_layer`
 * V3/yolo_v3.py:111-159 (input pixels).  Region (v2) heads are always normalised (V2/decode.py:13). */
enum yolo_location { YOLO_HOST = 0, YOLO_DEVICE = 1 };
enum yolo_image_format {
    YOLO_IMG_U8 = 0,           /* uint8  [n,H,W,3] already at network size ([net] height x width) */
    YOLO_IMG_F32 = 1,          /* float32 [n,H,W,3] already at network size */
    YOLO_IMG_F32_CHW = 2       /* float32 [n,3,H,W] planar: darknet's `image` layout (DN/image.c get_pixel) */
};
enum yolo_nms_mode {
    YOLO_NMS_TF = 0,           /* tf.image.non_max_suppression: class-agnostic, `>` iou, top max_out (row N1) */
    YOLO_NMS_PER_CLASS = 1,    /* V2 bboxes_nms (V2/utils.py:176-187): same-class, drop unless iou < thr (row N3) */
    YOLO_NMS_DARKNET = 2,      /* do_nms_sort (DN/box.c:58-89) on max-class score: same-class, drop if iou > thr */
    YOLO_NMS_TF_V1 = 4,        /* YOLOv1's call of tf.image.non_max_suppression (V1/YOLO_V1_Inference.py:259-266): as YOLO_NMS_TF on
                                * boxes whose horizontal extent is built from h and vertical extent from w (the reference's swap);
                                * the records hold those corners: centre = their midpoint, w = y1 - y0, h = x1 - x0 */
    YOLO_NMS_NUMPY_V3 = 3      /* `non_max_suppression` V3/yolo_v3.py:376-420 (row N2): gate on objectness > thr, class =
                                * argmax cls, per class by objectness, keep iou < thr with the unclamped `_iou`; reported
                                * score reproduces the reference's shifted-index behaviour.  Records come out class by
                                * class (ascending), in selection order; boxes are corners (x - w/2 form). */
};
enum yolo_select_mode {
    YOLO_SELECT_GT = 0,        /* max(obj*cls) >  thr  (V3/YOLOV3.py:358) */
    YOLO_SELECT_GE = 1         /* max(obj*cls) >= thr  (V2/postprocess.py:61) */
};

typedef struct yolo_config {
    uint32_t struct_size;      /* = sizeof(yolo_config) */
    const char *cfg_text;      /* darknet cfg text: [net] + convolutional/shortcut/route/upsample/maxpool/reorg/yolo/region */
    int32_t max_batch;
    int32_t dtype;             /* enum yolo_dtype */
    int32_t semantics;         /* enum yolo_semantics */
    int32_t decode;            /* enum yolo_decode */
    int32_t device;            /* HIP device ordinal */
    int32_t keep_layers;       /* 1: every layer output keeps its own buffer (yolo_layer_output valid) */
    void *stream;              /* hipStream_t to launch on, or NULL for a context-owned stream */
} yolo_config;

/* One detection: corners in the decode's units, max class score, class id (24 bytes). */
typedef struct yolo_box {
    float x0, y0, x1, y1;
    float score;
    int32_t cls;
} yolo_box;

/* One image of a ragged batch (yolo_*_images_*): a uint8 RGB [h][w][3] image at byte `offset` of one packed buffer (16 bytes). */
typedef struct yolo_image_desc {
    uint64_t offset;
    int32_t h, w;
} yolo_image_desc;
/* How a native-size image is fitted into the S x S network input (each bit-identical, per pixel, to the single-image path named). */
enum yolo_fit {
    YOLO_FIT_STRETCH = 0,      /* /255, then TF legacy bilinear stretch (yolo_forward_image_u8; D2T/YOLO_V3_convert...py:106-111) */
    YOLO_FIT_LETTERBOX = 1,    /* darknet letterbox_image: darknet's (float)p/255., aspect-preserving resize_image, 0.5 fill, centred
                                * (yolo_forward_letterbox_chw on the same image converted on the host, DN/image.c:960-981) */
    YOLO_FIT_CV2 = 2,          /* V2 preprocess_image: cv2.resize INTER_LINEAR, then /225 (yolo_op_resize_cv2, V2/utils.py:13-27), RGB in */
    YOLO_FIT_CV2_BGR = 3,      /* the same on a BGR image: the RGB swap of cv2.cvtColor(.., COLOR_BGR2RGB) first */
    YOLO_FIT_CENTER_CROP = 4   /* darknet's classifier validation (DN/examples/classifier.c:635-636): darknet's (float)p/255., resize_min(im, net_w) -- the
                                * shorter side becomes the network WIDTH, integer divisions, no resize where the size does not change --, then crop_image
                                * of net_w x net_h from the centre, coordinates clamped (the edge is replicated, no fill; DN/image.c:857-875, :997-1011).
                                * The forward and classify entry points take it; yolo_detect_images_* and yolo_segment_images_u8 return
                                * YOLO_ERR_UNSUPPORTED: boxes and labels cannot be mapped back through a crop that discards part of the image */
};
/* Units of the records yolo_detect_images_* returns.
 * NETWORK: as yolo_postprocess returns them for an image at network size (STRETCH / CV2: normalised or network pixels by the decode;
 * LETTERBOX: un-letterboxed boxes normalised to the source image, darknet's relative = 1).
 * SOURCE_PIXELS: in the source image's pixels -- STRETCH / CV2: the kept records scaled after NMS (`convert_to_original_size`,
 * V3/YOLO_V3_inference.py:55-57, V3/convert_ckpt_and_inference.py:43-45); LETTERBOX: relative = 0; YOLO_NMS_PER_CLASS: the image's
 * (h, w) is V2's `image_shape` (V2/utils.py:30-43). */
enum yolo_box_units { YOLO_UNITS_NETWORK = 0, YOLO_UNITS_SOURCE_PIXELS = 1 };

/* ---- lifecycle ------------------------------------------------------------------------------ */
/* Parses the topology, plans buffers on `device`.  On failure returns NULL and writes a message to
 * err (if non-NULL).  Replaces load_network's cfg half (DN/parser.c:730-875). */
yolo_ctx *yolo_create(const yolo_config *cfg, char *err, size_t err_len);
void yolo_destroy(yolo_ctx *ctx);
const char *yolo_last_error(const yolo_ctx *ctx);

/* ---- weights (row L) ------------------------------------------------------------------------ */
/* Reads a Darknet .weights file (header rule DN/parser.c:1259-1265; header_ints 4 or 5 forces the
 * reference loaders' fixed counts V3/yolo_v3.py:278 / D2T V2 :351, 0 = auto), folds BN
 * (W*g/sqrt(v+1e-5), b - m*g/sqrt(v+1e-5), fp32), packs and uploads. */
int yolo_load_darknet_weights(yolo_ctx *ctx, const char *path, int header_ints);
/* Export artifact: ONE self-describing file holding the cfg text, the run configuration (dtype, semantics,
 * decode), the folded + packed device-ready parameters of every conv (fp8: codes and scales) and the tile plan.  It is
 * to this library what the frozen `.pb` (input -> detected_boxes / detected_scores / detected_classes,
 * D2T/YOLO_V3_convert_darkenet_to_Tensorflow.py:99-104, D2T/object_detect.py:64-99) is to the reference: a caller
 * needs nothing else to run detections.  The file is checksummed; a mismatch, truncation or a packing that does not
 * fit the topology is an error, never a partial load. */
int yolo_export(yolo_ctx *ctx, const char *path);
yolo_ctx *yolo_create_from_file(const char *path, int max_batch, int device, void *stream, int keep_layers, char *err, size_t err_len);
/* Same from the float stream that follows the header (n floats, must match the topology). */
int yolo_set_weights(yolo_ctx *ctx, const float *flat, size_t n);
size_t yolo_weights_count(const yolo_ctx *ctx);
/* YOLO_FP8 only: per-layer activation scales (stored code = e4m3(value / scale)), one float per cfg layer; entries of
 * layers that only move data (route, upsample, maxpool, reorg, yolo/region) are ignored.  Default: all 1.  Call BEFORE
 * loading weights (filters absorb their input scales; a later call invalidates loaded weights).  No reference
 * counterpart: the reference has no reduced-precision path. */
int yolo_set_act_scales(yolo_ctx *ctx, const float *scales, int n_layers);

/* ---- geometry ------------------------------------------------------------------------------- */
int yolo_input_size(const yolo_ctx *ctx, int *height, int *width, int *channels);
int yolo_num_rows(const yolo_ctx *ctx);      /* candidates per image: 10647 @416 v3, 845 v2 */
int yolo_num_attrs(const yolo_ctx *ctx);     /* 5 + classes */
int yolo_num_layers(const yolo_ctx *ctx);
/* detection head number `head` (0-based, cfg order): kind 0 = [yolo], 1 = [region], 2 = [detection]; grid rows and columns; anchors
 * per cell; first row of this head in the decoded tensor (rows are cell-major, cell = row * grid_w + col, anchor inner).
 * YOLO_ERR_INVALID past the last head. */
int yolo_head_geometry_hw(const yolo_ctx *ctx, int head, int *kind, int *grid_h, int *grid_w, int *anchors, int *row_offset);
/* the same for a head whose grid is square (grid = its side).  A head of a network with width != height has two sides:
 * YOLO_ERR_UNSUPPORTED, use yolo_head_geometry_hw. */
int yolo_head_geometry(const yolo_ctx *ctx, int head, int *kind, int *grid, int *anchors, int *row_offset);
double yolo_conv_flops(const yolo_ctx *ctx); /* 2*k*k*Cin*Cout*Ho*Wo summed (DN/convolutional_layer.c:325), per image */
double yolo_conv_bytes(const yolo_ctx *ctx, int n); /* algorithmic HBM bytes of the conv stack for n images */

/* ---- hot path ------------------------------------------------------------------------------- */
/* The image's channel count.  A cfg without a [net] yolo_input key reads RGB images: channels=3, anything else is refused.  With
 * [net] yolo_input=planes the network reads images of C = [net] channels planes, 1 <= C <= 1024 (grey, thermal, RGB-D, multispectral,
 * darknet's 19 x 19 x 1 go board); darknet ignores the key, so the same cfg loads there.  yolo_input_size reports C.  Wherever the
 * entry points below say 3, read C: yolo_forward takes [n,H,W,C] (YOLO_IMG_F32_CHW: [n,C,H,W]), yolo_forward_letterbox_chw [C,h,w],
 * yolo_forward_image_u8 and the yolo_*_images_u8 family packed [h,w,C] bytes, C bytes per pixel and w * C per row.  The channels
 * C .. roundup(C, 8) - 1 of the staged input are zero (the letterbox's 0.5 fill and [net] yolo_input_mul / yolo_input_add belong to
 * the C real channels).  With C = 3 the key changes nothing.  With C != 3: configurations bf16, fp16 and fp32 (fp8 and split-fp16
 * are refused when the cfg is planned, by name); layer 0 runs the kernels every inner layer runs, no fused first-stage kernel; and,
 * YOLO_ERR_UNSUPPORTED before any launch, naming the entry point and C: YOLO_FIT_CV2 / YOLO_FIT_CV2_BGR (their meaning is an RGB /
 * BGR image) and yolo_detect_tiled_u8.
 *
 * images: [n,H,W,3] ([net] height x width) in `fmt`, at `loc`; each value is multiplied by `scale` on the way in
 * (1/255 for the `inputs / 255` of V3/yolo_v3.py:215, 1 for pre-normalised input).  Runs the conv stack
 * and the head decode; the decoded tensor [n, rows, attrs] (V3/yolo_v3.py:266) stays resident and, when
 * detections_out != NULL, is also copied there (fp32, at out_loc).  Asynchronous on the context stream
 * unless a host buffer is involved. */
int yolo_forward(yolo_ctx *ctx, const void *images, int n, int fmt, int loc, float scale,
                 float *detections_out, int out_loc);

/* Row P: ONE uint8 RGB image of any size [h,w,3] -> /255 -> legacy bilinear stretch to
 * S x S on the device (D2T/YOLO_V3_convert...py:106-111), then as yolo_forward with n = 1. */
int yolo_forward_image_u8(yolo_ctx *ctx, const uint8_t *image, int h, int w, int loc,
                          float *detections_out, int out_loc);
/* darknet's network_predict_image (DN/network.c:579-586): ONE planar float image [3,h,w] (0..1) of any size ->
 * letterbox_image (DN/image.c:960-981: aspect-preserving resize_image DN/image.c:1347-1393, 0.5 fill, centred) on the
 * device, then as yolo_forward with n = 1. */
int yolo_forward_letterbox_chw(yolo_ctx *ctx, const float *image_chw, int w, int h, int loc,
                               float *detections_out, int out_loc);

/* A ragged batch of native-size uint8 RGB images in ONE device step: `pixels` holds n images packed in one buffer of `bytes` bytes (at
 * `loc`; YOLO_HOST: staged with one host-to-device copy), descs[n] (host memory) where each one lies.  One launch fits every image
 * into the network input (`fit`, enum yolo_fit), then as yolo_forward with n images.  YOLO_ERR_INVALID before any launch when n is
 * outside 1..max_batch, a descriptor has h < 1 or w < 1 or ends past `bytes`, `bytes` >= 2^32, a letterboxed image would be less
 * than one pixel wide or high, or (YOLO_FIT_CENTER_CROP) an image's longer side times the network width does not fit an int. */
int yolo_forward_images_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc,
                           float *detections_out, int out_loc);
/* The same + threshold + NMS with each image's geometry (enum yolo_box_units): boxes_out [n * max_out], counts_out [n] at out_loc.
 * LETTERBOX un-letterboxes every box for its image before NMS, darknet's order (networks with a [detection] head:
 * YOLO_ERR_UNSUPPORTED, darknet v1 does not letterbox). */
int yolo_detect_images_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc,
                          float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                          yolo_box *boxes_out, int32_t *counts_out, int out_loc);
/* yolo_detect_images_u8 replayed from a HIP graph, as yolo_detect_graph: `pixels`, boxes_out and counts_out are device pointers, descs
 * host memory.  The graph is keyed on the buffer pointer, `bytes`, n and the modes -- NOT on the image sizes or offsets: every call
 * validates the descriptors on the host and copies them into the context's device table on the context stream before the launch, so
 * one captured graph serves batches whose image sizes change from call to call. */
int yolo_detect_images_graph(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit,
                             float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                             yolo_box *boxes_out, int32_t *counts_out);
/* The value one source byte `value` (0..255) contributes to a fit's arithmetic before interpolation: STRETCH value / 255.0f, LETTERBOX and
 * CENTER_CROP darknet's (float)value/255. (a double division rounded to float, DN/image.c load_image_stb), CV2 the byte itself.  Host-side; the
 * device evaluates the same expression. */
float yolo_fit_unit_value(int fit, int value);

/* ---- tiled detection of images larger than the network input ("Tiled detection"; no counterpart in the reference) ----
 * One window of the grid an image is cut into: rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1 of the image (16 bytes). */
typedef struct yolo_tile_window {
    int32_t y0, x0, h, w;
} yolo_tile_window;
/* The window grid of an img_h x img_w image.  Per axis, with image extent L, tile extent T and overlap O (0 <= O < T): L <= T gives ONE
 * window [0, L) -- the whole extent, smaller than the tile; otherwise the stride is S = T - O, there are ceil((L - T) / S) + 1 windows of
 * extent T and window k starts at min(k * S, L - T): the last one is pulled back to the image's edge, so every window lies inside the
 * image.  Windows are listed row-major, y outer and x inner.  *count is always written; at most `cap` windows are written to out (cap = 0 /
 * out = NULL: the count only).  YOLO_ERR_INVALID for a non-positive extent, O < 0, O >= T, count == NULL or a grid of 2^31 windows or
 * more.  Host-side: no context, no device. */
int yolo_tile_windows(int img_h, int img_w, int tile_h, int tile_w, int overlap_h, int overlap_w, yolo_tile_window *out, int cap, int *count);
/* Detection in images of any size at the resolution of their windows: every image of descs[n_images] (whole images in `pixels`, as for
 * yolo_detect_images_u8; n_images is NOT bound by max_batch) is cut into the windows of yolo_tile_windows (tile_h = tile_w = 0: the
 * network's own input size), each window is fitted into the network input straight from the image it lies in (`fit`: YOLO_FIT_STRETCH or
 * YOLO_FIT_LETTERBOX; bit for bit the fit of the same crop handed over as an image of its own), the windows run max_batch at a time --
 * ceil(windows / max_batch) network steps, images may share a step --, after every step the rows that pass `select_mode` against
 * score_thr are mapped to SOURCE-IMAGE pixels and appended to their image's candidate list in (window, row) order, and after the last
 * step ONE NMS launch (nms_mode: YOLO_NMS_TF or YOLO_NMS_DARKNET) runs over all images: duplicates across windows are suppressed like
 * duplicates inside one.  boxes_out [n_images * max_out], counts_out [n_images] at out_loc.  The records are in the image's pixels
 * (relative = 0) or divided by its width and height (relative = 1): corners for YOLO_NMS_TF, (cx, cy, w, h) for YOLO_NMS_DARKNET, as
 * yolo_detect_images_u8 reports them.  Results do not depend on max_batch and are bit-reproducible from run to run.
 * Every check runs before any launch.  YOLO_ERR_INVALID: a classifier or map context, a descriptor as yolo_forward_images_u8 refuses it,
 * tile or overlap outside the rule above, an image too large for 32-bit sizes.  YOLO_ERR_UNSUPPORTED, naming what is refused: the CV2 and
 * CENTER_CROP fits, YOLO_NMS_PER_CLASS / YOLO_NMS_TF_V1 / YOLO_NMS_NUMPY_V3, a softmax-tree head, a [detection] head with the letterbox.
 * An image whose windows yield more than 32768 candidates in all: YOLO_ERR_UNSUPPORTED naming the image and the count, and nothing is
 * written to boxes_out / counts_out.  There is no captured-graph form. */
int yolo_detect_tiled_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n_images,
                         int tile_h, int tile_w, int overlap_h, int overlap_w, int fit, int loc,
                         float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative,
                         yolo_box *boxes_out, int32_t *counts_out, int out_loc);

/* ---- decoded video frames: NV12, I420 and pitched RGB / BGR surfaces (no counterpart in the reference) ----
 * A frame is h x w pixels (odd sizes are served) as a video decoder or a capture leaves them, described in place:
 *   YOLO_PIX_NV12   plane 0: Y, h rows of w bytes; plane 1: interleaved U,V, ceil(h/2) rows of 2 * ceil(w/2) bytes
 *   YOLO_PIX_I420   plane 0: Y; planes 1 and 2: U and V, each ceil(h/2) rows of ceil(w/2) bytes
 *   YOLO_PIX_RGB24 / YOLO_PIX_BGR24   plane 0: h rows of 3 * w bytes
 * Every plane has its own byte offset into the packed buffer and its own row pitch (at least the row's bytes; any larger value is
 * allowed); the planes a format does not have are not read.  Pixel (y, x) takes its chroma sample from (y >> 1, x >> 1): nearest, no
 * chroma interpolation.  The RGB bytes of a YUV pixel are, with m the frame's matrix, in int32 with an arithmetic `>>`:
 *   y' = max(0, Y - yoff[m]) * CY[m];   u = U - 128;   v = V - 128
 *   R = clamp8((y' + CVR[m] * v                 + 2^19) >> 20)
 *   G = clamp8((y' - CUG[m] * u - CVG[m] * v    + 2^19) >> 20)
 *   B = clamp8((y' + CUB[m] * u                 + 2^19) >> 20)
 *   matrix                               yoff  CY       CVR      CUG     CVG     CUB       round(k * 2^20) of
 *   YOLO_MATRIX_BT601 (limited range)    16    1220542  1673527  409993  852492  2116026   1.164, 1.596, 0.391, 0.813, 2.018
 *   YOLO_MATRIX_BT709 (limited range)    16    1220542  1880097  223347  558891  2214593   1.164, 1.793, 0.213, 0.533, 2.112
 *   YOLO_MATRIX_BT601_FULL (JFIF)        0     1048576  1470104  360853  748826  1858077   1, 1.402, 0.344136, 0.714136, 1.772
 * (every intermediate lies in -282 943 616 .. +573 487 137).  The BT.601 limited row is believed to be what OpenCV's COLOR_YUV2RGB_NV12
 * evaluates; cv2 is absent where this was written: that equality is unpinned, the rule above is what is promised.  RGB24 bytes are the
 * image's own, BGR24 swaps channels 0 and 2; the matrix of such a frame must still be a valid one.
 * From there on a frame IS the h x w x 3 byte image this rule yields: every fit reads it exactly as it reads a packed RGB image
 * (yolo_fit_unit_value, the /255, darknet's two-pass resize_image, the cv2 rule, [net] yolo_input_mul / yolo_input_add), host and device
 * evaluate the rule identically, and no RGB copy of the frame is ever stored.  64 bytes. */
enum yolo_pix_format { YOLO_PIX_NV12 = 0, YOLO_PIX_I420 = 1, YOLO_PIX_RGB24 = 2, YOLO_PIX_BGR24 = 3,
                       /* the component planes of a decoded JPEG file (below, "JPEG files"); 4 .. 15 are no format */
                       YOLO_PIX_JPEG_GREY = 16, YOLO_PIX_JPEG_444 = 17, YOLO_PIX_JPEG_422 = 18, YOLO_PIX_JPEG_420 = 19, YOLO_PIX_JPEG_440 = 20 };
enum yolo_color_matrix { YOLO_MATRIX_BT601 = 0, YOLO_MATRIX_BT709 = 1, YOLO_MATRIX_BT601_FULL = 2 };
typedef struct yolo_frame_desc {
    uint64_t offset[3];        /* where each plane begins in the packed buffer */
    uint64_t pitch[3];         /* bytes from one row of the plane to the next */
    int32_t h, w;
    int32_t format;            /* enum yolo_pix_format */
    int32_t matrix;            /* enum yolo_color_matrix */
} yolo_frame_desc;
/* The rule on the host: the frame `desc` describes inside pixels[bytes] -> rgb_out [h][w][3] uint8.  The counterpart of
 * yolo_fit_unit_value: no context, no device.  YOLO_ERR_INVALID (text in yolo_last_error(NULL)): a NULL pointer, and what every
 * yolo_*_frames_* entry point refuses for a descriptor: an unknown format or matrix, h or w below 1, a pitch below the plane's row
 * bytes, a pitch or a plane that passes 32 bits, a plane that ends past `bytes`. */
int yolo_frame_to_rgb_host(const yolo_frame_desc *desc, const uint8_t *pixels, size_t bytes, uint8_t *rgb_out);
/* The same on the device, by one kernel of its own (host buffers, in the style of the other yolo_op_*): pins the rule there. */
int yolo_op_frame_to_rgb(const yolo_frame_desc *desc, const uint8_t *pixels, size_t bytes, uint8_t *rgb_out, int device);
/* yolo_forward_images_u8, yolo_detect_images_u8, yolo_detect_images_graph and yolo_detect_tiled_u8 over frames, argument for argument:
 * yolo_frame_desc in the place of yolo_image_desc, everything else as documented there -- the fit launch converts while it fits, one
 * batch may mix formats and matrices, boxes come back in the frame's own pixels (YOLO_UNITS_SOURCE_PIXELS / the tiled form), frame
 * averaging and recurrent state advance as for images.  The graph form keeps a captured step of its own: a caller that alternates
 * yolo_detect_images_graph and yolo_detect_frames_graph recaptures neither; the frame table is copied on the context stream before
 * every replay.  A tiled window indexes chroma by the pixel's position in the FRAME: a window may start on an odd row or column.
 * Every refusal comes before any launch and names the frame.  YOLO_ERR_INVALID: a descriptor as yolo_frame_to_rgb_host refuses it, and
 * everything the image form refuses with that code.  YOLO_ERR_UNSUPPORTED: a network of other than 3 channels ([net]
 * yolo_input=planes); YOLO_FIT_CV2_BGR (the frame's format states its channel order); whatever the image form of the same entry point
 * refuses (the centre crop where boxes are mapped back, tiling's list). */
int yolo_forward_frames_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc,
                           float *detections_out, int out_loc);
int yolo_detect_frames_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc,
                          float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                          yolo_box *boxes_out, int32_t *counts_out, int out_loc);
int yolo_detect_frames_graph(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit,
                             float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                             yolo_box *boxes_out, int32_t *counts_out);
int yolo_detect_tiled_frames_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n_images,
                                int tile_h, int tile_w, int overlap_h, int overlap_w, int fit, int loc,
                                float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative,
                                yolo_box *boxes_out, int32_t *counts_out, int out_loc);

/* ---- JPEG files: what darknet's load_image reads through its vendored stb_image (DN/image.c load_image_stb) ----
 * The host parses the file and Huffman-decodes it to dequantised coefficient blocks; the device does the rest: one IDCT launch per
 * batch writes the component planes (uint8, whole MCUs: plane_w x plane_h) into a surface the context owns, and a decoded file is
 * then a FRAME over those planes, in one of five formats that carry the reference's integer rule with them:
 *   YOLO_PIX_JPEG_GREY  plane 0: Y, h rows of w bytes; R = G = B = Y
 *   YOLO_PIX_JPEG_444   planes 0, 1, 2: Y, Cb, Cr, each h rows of w bytes
 *   YOLO_PIX_JPEG_422   Y as above; Cb, Cr: h rows of ceil(w / 2) bytes
 *   YOLO_PIX_JPEG_420   Y as above; Cb, Cr: ceil(h / 2) rows of ceil(w / 2) bytes
 *   YOLO_PIX_JPEG_440   Y as above; Cb, Cr: ceil(h / 2) rows of w bytes
 * (any pitch at least the row's bytes, as for the other formats).  Pixel (y, x) takes its chroma through the reference's upsamplers
 * (stbi__resample_row_h_2 / _hv_2 / _v_2: 3:1 linear interpolation with their edge cases, rows clamped to the component's own), indexed by
 * the pixel's position in the frame, and its colour through stbi__YCbCr_to_RGB_row; kernels.h states both as closed forms.  The
 * `matrix` field of such a frame must be 0: it selects nothing.  The result is bit-equal to load_image's bytes.
 * Served: baseline and extended sequential Huffman (SOF0, SOF1), 8-bit, one scan; 1 component, or 3 components as YCbCr with luma
 * sampled 1x1, 2x1, 2x2 or 1x2 and chroma 1x1; any size, any restart interval, 8- and 16-bit quantisation tables.  APPn / COM segments
 * are skipped, EXIF orientation is ignored as the reference ignores it.  YOLO_ERR_UNSUPPORTED, naming the file's index and the
 * feature: progressive, arithmetic-coded, lossless, hierarchical or 12-bit files, 4 components (CMYK / YCCK), 3 components stored
 * as RGB (component ids R, G, B, or Adobe APP14 transform 0 without JFIF), any other sampling, several scans.
 * YOLO_ERR_INVALID, naming the file's index and the byte offset: anything malformed or truncated (the reference decodes a truncated
 * file as if zero bits followed; this library refuses it). */
struct yolo_jpeg_info {        /* (a tag, no typedef: the function below has the name, as stat(2) and struct stat share theirs) */
    int32_t h, w;
    int32_t components;        /* 1 or 3 */
    int32_t hs, vs;            /* the luma sampling factors; chroma is 1 x 1 */
    int32_t format;            /* the YOLO_PIX_JPEG_* of its frame */
    int32_t restart_interval;  /* MCUs, 0: none */
    int32_t mcus_w, mcus_h;
    int32_t plane_w[3], plane_h[3];   /* the padded component planes the IDCT writes: whole MCUs (0 for the planes a grey file lacks) */
    int32_t blocks[3];         /* 8 x 8 blocks of every plane */
};
/* The headers of one file: host only; the text of a refusal in yolo_last_error(NULL), "file 0: ...". */
int yolo_jpeg_info(const uint8_t *file, size_t bytes, struct yolo_jpeg_info *out);
/* The host stage by itself: the dequantised coefficient blocks of the file, coef_out [blocks[0] + blocks[1] + blocks[2]][64] int16 in
 * natural (de-zigzagged) order, plane by plane, each plane's blocks in raster order -- what the IDCT kernel reads, and what the
 * reference hands to its IDCT (the wrap to 16 bits of its dequantising multiply included).  cap_blocks: the room in coef_out. */
int yolo_jpeg_coefficients(const uint8_t *file, size_t bytes, int16_t *coef_out, size_t cap_blocks);
/* The whole decode on the host, no context and no device: rgb_out [h][w][3] uint8, cap its size in bytes (YOLO_ERR_INVALID when
 * below h * w * 3).  The CPU anchor of the rule, and what libdarknet_hip.so's load_image reads JPEG files with. */
int yolo_jpeg_to_rgb_host(const uint8_t *file, size_t bytes, uint8_t *rgb_out, size_t cap);
/* The same through the device (host buffers; rgb_out holds h * w * 3 bytes): host entropy stage, the IDCT kernel, then the
 * frame-to-RGB operator over its planes. */
int yolo_op_jpeg_to_rgb(const uint8_t *file, size_t bytes, uint8_t *rgb_out, int device);
/* files[i] of bytes[i] bytes, i < n (any n >= 1) -> a frame table over the context's surface.  The batch is entropy-decoded by
 * min(n, 8) host threads into pinned memory, uploaded once and transformed by one launch on the context stream.  descs_out[n]
 * (host) describes every file's planes inside *device_pixels (device memory) of *device_bytes bytes -- the surface's capacity, so
 * that batches of different sizes present the same buffer to yolo_detect_frames_graph --: pass the three to any yolo_*_frames_*
 * entry point with loc = YOLO_DEVICE.  Table and surface are valid until the next decode on this context; a decode that needs a
 * larger surface moves it.  Every refusal comes before the first launch and names the file. */
int yolo_decode_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, yolo_frame_desc *descs_out,
                      const uint8_t **device_pixels, size_t *device_bytes);
/* What the last decode on this context cost (waits for its IDCT): the host's entropy stage in wall-clock ms, the upload and the IDCT
 * launch in device ms between events on the context stream, and the bytes uploaded.  Any pointer may be NULL.  tools/jpeg_rate.py. */
int yolo_jpeg_decode_times(yolo_ctx *ctx, double *entropy_ms, double *upload_ms, double *idct_ms, size_t *upload_bytes);
/* ---- the entropy stage on the device, over restart intervals ----
 * A restart interval (DRI) is byte-aligned, begins with zeroed DC predictors and ends at a marker: the intervals of a file are independent
 * streams, and k_jpeg_entropy Huffman-decodes one per lane, a whole batch per launch, from the uploaded file bytes into the coefficient
 * array the IDCT reads.  YOLO_JPEG_ENTROPY_HOST (the default) is the host stage above for every file.  Under YOLO_JPEG_ENTROPY_AUTO,
 * yolo_decode_jpegs and every yolo_*_jpegs entry point send the ELIGIBLE files of a batch to the device and the others through the
 * host stage, in one call, with one IDCT launch over all.  Eligible: the file has a DRI and a scan of its entropy-coded segment finds
 * exactly the expected RSTm markers (fill bytes 0xFF allowed in front, nothing else between).  The results are bit-equal, and so are
 * the verdicts: a file of which any interval fails on the device, or leaves whole bytes unread in front of its marker, is decoded
 * again by the host stage, and what that returns -- its coefficients, or its code and message -- is what the call returns.  Such a
 * refusal comes after the first launch; refusals of header kinds still come before it.  After it the contents of the context's surface
 * and what the two *_times calls report are undefined until the next successful decode (a batch refused under HOST leaves the
 * previous surface as it was).  A decode under AUTO that ran the device stage has waited for it when it returns. */
enum { YOLO_JPEG_ENTROPY_HOST = 0, YOLO_JPEG_ENTROPY_AUTO = 1 };
int yolo_set_jpeg_entropy(yolo_ctx *ctx, int mode);          /* any other mode: YOLO_ERR_INVALID */
int yolo_jpeg_entropy(yolo_ctx *ctx);                        /* the mode; a fresh context: YOLO_JPEG_ENTROPY_HOST */
/* What the entropy stage of the last decode on this context did: files decoded on the device and by the host stage (a file handed
 * back counts as the host's, its intervals are not counted), restart intervals decoded on the device and served, the interval scan in wall-clock ms, the device stage
 * (k_jpeg_entropy and what zeroes its blocks) in device ms, and the bytes of the uploaded files.  Any pointer may be NULL.
 * yolo_jpeg_decode_times keeps its meaning: the host stage's wall clock, all uploads, the IDCT launch. */
int yolo_jpeg_entropy_times(yolo_ctx *ctx, int *device_files, int *host_files, int *intervals, double *scan_ms, double *device_ms,
                            size_t *stream_bytes);
/* The interval scan by itself, host only: the restart intervals of an eligible file, interval i the bytes begin_out[i] .. end_out[i] - 1
 * of it, *n_out their count (cap: the room in the two arrays, either of which may be NULL).  A file that is not eligible: YOLO_OK and
 * *n_out = 0.  A file whose headers are refused: that refusal. */
int yolo_jpeg_intervals(const uint8_t *file, size_t bytes, uint32_t *begin_out, uint32_t *end_out, size_t cap, size_t *n_out);
/* One file through scan, upload, k_jpeg_entropy and read-back: coef_out as yolo_jpeg_coefficients.  YOLO_ERR_UNSUPPORTED ("no restart
 * interval") for a file without DRI; for a file that is not eligible, or that the device hands back, the host stage's result. */
int yolo_op_jpeg_entropy(const uint8_t *file, size_t bytes, int16_t *coef_out, size_t cap_blocks, int device);
/* yolo_decode_jpegs, then yolo_forward_frames_u8 / yolo_detect_frames_u8 / yolo_detect_tiled_frames_u8 over its table: the
 * arguments of those, with (files, bytes, n) in the place of the packed buffer, its descriptors and its location. */
int yolo_forward_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, int fit, float *detections_out, int out_loc);
int yolo_detect_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, int fit,
                      float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                      yolo_box *boxes_out, int32_t *counts_out, int out_loc);
int yolo_detect_tiled_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n_images,
                            int tile_h, int tile_w, int overlap_h, int overlap_w, int fit,
                            float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative,
                            yolo_box *boxes_out, int32_t *counts_out, int out_loc);

/* darknet's get_network_boxes on the device (DN/network.c:536-567 = num_detections + fill_network_boxes ->
 * get_yolo_detections DN/yolo_layer.c:316-343 / get_region_detections DN/region_layer.c:364-437 (softmax heads, no tree),
 * then correct_yolo_boxes DN/yolo_layer.c:247-273) over image 0 of the last forward: boxes above `thresh`, compacted in
 * darknet's order, un-letterboxed for a w x h source image.  records: host [cap][5 + classes] = x, y, w, h, objectness,
 * prob[classes]; *count = number of detections (may exceed cap; cap = 0 / records = NULL: count only = num_detections). */
int yolo_darknet_boxes(yolo_ctx *ctx, int w, int h, float thresh, int relative, float *records, int cap, int *count);
/* The same over image `image` of the last forward (0 <= image < its batch): e.g. the letterboxed batch of yolo_forward_images_u8,
 * each image with its own w x h.  yolo_darknet_boxes is yolo_darknet_boxes_at(ctx, 0, ...). */
int yolo_darknet_boxes_at(yolo_ctx *ctx, int image, int w, int h, float thresh, int relative, float *records, int cap, int *count);
/* What darknet's network_predict returns (DN/network.c:497-508, net->output): the LAST layer's output of image 0 in darknet's
 * own layout -- for a [yolo] / [region] layer the planar [anchors * (5 + classes)][grid_h * grid_w] tensor with that layer's
 * activations applied (DN/yolo_layer.c:143-152, DN/region_layer.c:160-186).  host buffer of yolo_last_layer_size() floats. */
size_t yolo_last_layer_size(const yolo_ctx *ctx);
int yolo_last_layer_output(yolo_ctx *ctx, float *out, size_t out_floats);
/* The same for images 0..n-1 of the last forward, image after image (darknet's net->output is batch * outputs contiguous floats,
 * DN/network.c:497-508 with l.output sized batch * l.outputs, DN/yolo_layer.c:50): out holds n * yolo_last_layer_size() floats. */
int yolo_last_layer_output_batch(yolo_ctx *ctx, int n, float *out, size_t out_floats);

/* The raw tensor detection head `head` (0-based, cfg order) decodes, for images 0..n-1 of the last forward: the head conv's fp32
 * output [n, grid, grid, anchors * (5 + classes)] dense, to host -- what the reference's graph builders return before any decode
 * (`build_network` V2/model_darknet19_slim.py:198-200; the per-scale `predictions` of V3/yolo_v3.py:239-263). */
int yolo_head_raw(yolo_ctx *ctx, int head, int n, float *out, size_t out_floats);

/* Threshold + NMS on the resident decoded tensor of the last forward (rows S, N1/N3).
 * boxes_out: [n * max_out] caller-owned, counts_out: [n]; both at out_loc.
 * Replaces get_network_boxes + do_nms_* (DN/network.c:562, DN/box.c:21-89) and the TF tail
 * V3/YOLOV3.py:347-379. */
int yolo_postprocess(yolo_ctx *ctx, int n, float score_thr, float iou_thr, int max_out,
                     int nms_mode, int select_mode, yolo_box *boxes_out, int32_t *counts_out, int out_loc);

/* The same, and for every box record the ROW of the decoded tensor it was formed from (0 .. yolo_num_rows()-1 within its image):
 * rows_out [n * max_out] int32 at out_loc, -1 in the unused slots; NULL = not reported.  `self.boxes` of the reference's detectors
 * is the decoded row itself (V1/YOLO_V1_Inference.py:255-268 gathers `_boxes` with the NMS indices): the index is what
 * tf.image.non_max_suppression returns, mapped back through the threshold mask. */
int yolo_postprocess_rows(yolo_ctx *ctx, int n, float score_thr, float iou_thr, int max_out,
                          int nms_mode, int select_mode, yolo_box *boxes_out, int32_t *counts_out, int32_t *rows_out, int out_loc);

/* forward + postprocess. */
int yolo_detect(yolo_ctx *ctx, const void *images, int n, int fmt, int loc, float scale,
                float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode,
                yolo_box *boxes_out, int32_t *counts_out, int out_loc);

/* yolo_detect for device-resident inputs and outputs, replayed from a HIP graph: the first call with a given argument
 * tuple runs eagerly, the second captures the launch sequence (preprocess, ~80 conv/ew launches, decode, NMS) into a
 * hipGraph, later calls replay it (removes the per-launch gaps of a launch-bound step).  Any change of argument
 * re-captures.  images / boxes_out / counts_out must be device pointers that stay valid between calls. */
int yolo_detect_graph(yolo_ctx *ctx, const void *images, int n, int fmt, float scale, float score_thr, float iou_thr,
                      int max_out, int nms_mode, int select_mode, yolo_box *boxes_out, int32_t *counts_out);

int yolo_synchronize(yolo_ctx *ctx);

/* ---- recurrent networks: [rnn] / [gru] / [lstm] layers carry state from one call to the next ---------------------
 * One yolo_forward* / yolo_detect* / yolo_classify* call is ONE TIME STEP (darknet after set_batch_network(net, 1) with
 * time_steps=1): batch index b of every call is stream b, a call with n images advances streams 0 .. n-1 and leaves streams
 * n .. max_batch-1 as they were.  Every state is zero at yolo_create and is no part of an export artifact.  A call that is
 * refused changes no state; yolo_time_forward / yolo_time_layers / yolo_autotune hand the states back as they found them; the
 * captured steps (yolo_detect_graph, yolo_detect_images_graph) hold the state update.  The state tensors are numbered in layer
 * order: an [rnn] or [gru] layer has one (its state, `output` floats per stream), an [lstm] layer two (h, then the cell c).
 * Values are exchanged as fp32: h of an [rnn] / [lstm] is kept in the network's storage type (it is a matrix operand), so
 * yolo_set_state rounds it as the kernels do and yolo_get_state -> yolo_set_state reproduces the next step bit for bit. */
int yolo_num_state_tensors(const yolo_ctx *ctx);                 /* 0: the network is a pure function of the batch */
int yolo_state_geometry(const yolo_ctx *ctx, int k, int *layer, size_t *floats_per_stream);
int yolo_get_state(yolo_ctx *ctx, int k, int stream, float *out, size_t out_floats);        /* host fp32, exactly floats_per_stream */
int yolo_set_state(yolo_ctx *ctx, int k, int stream, const float *in, size_t in_floats);
int yolo_reset_state(yolo_ctx *ctx, int stream);                 /* darknet's reset_network_state(net, b); stream < 0: every stream */

/* ---- frame-averaged detection on video streams (darknet's `detector demo`: remember_network + avg_predictions) -----
 * frames = K in 1 .. 8; 1 (the default) is off.  With K >= 2 every yolo_forward* / yolo_detect* call with n images is one time
 * step of the streams 0 .. n-1 (batch index b = stream b; the streams n .. max_batch-1 are untouched): per [yolo] / [region]
 * head the step writes the layer's activated output -- darknet's l.output: logistic on x, y, objectness and a [yolo] head's
 * classes, a [region] head's class softmax, w and h raw -- into slot pos[stream] of a ring of K slots, forms
 * avg = 0; avg = avg + (float)(1. / K) * slot[j] for j = 0 .. K-1 (slot order, fp32), decodes the boxes from avg, and then
 * moves pos[stream] on by one.  Everything behind the decode (scores, NMS, yolo_postprocess*, yolo_darknet_boxes*) reads the
 * averaged rows.  The slots are ZERO when the setting is made and after yolo_reset_state, so a stream's first K-1 steps are
 * attenuated by the empty slots, exactly as in darknet's demo (which callocs them).  yolo_detect* run the full decode while
 * K >= 2.  Changing K empties the ring and drops the captured steps; yolo_reset_state(ctx, stream) also empties that stream's
 * slots and position.  The timing calls and yolo_autotune are steps of no stream.  The setting is no part of the plan or of an
 * export artifact.  Refused: K outside 1 .. 8; a classifier, map or vector-input network; a [detection] (YOLOv1) head; a
 * [region] head with a softmax tree; more than 128 attributes per box; yolo_detect_tiled_u8 while K >= 2.
 * Device memory: (K + 1) * max_batch * rows * attrs * 4 bytes. */
int yolo_set_frame_average(yolo_ctx *ctx, int frames);
int yolo_frame_average(const yolo_ctx *ctx);                     /* the current K */

/* ---- vector-input networks: char-rnn ([net] yolo_input=vector, inputs=N) ------------------------------------------
 * A cfg whose [net] section says yolo_input=vector and inputs=N (1 .. 2^24, no height / width) reads one row of N values per
 * stream instead of an image; darknet ignores the key, so the same cfg loads there.  Served sections: [connected], [rnn], [gru],
 * [lstm], [dropout], [activation], [softmax], [cost]; configurations: bf16, fp16, fp32.  The output layer must be a [softmax].
 * The image entry points (yolo_forward*, yolo_detect*, yolo_classify*, the tiled and map calls) refuse such a network and the
 * calls below refuse an image network; yolo_input_size reports 1 x 1 x N; the state calls, yolo_layer_output and the timing
 * calls work as on any recurrent network.
 *
 * yolo_forward_vectors: ONE step of streams 0 .. n-1 over x, fp32 [n][N] (loc: where x lies); out (may be NULL, host): the
 * output layer's probabilities [n][classes].
 *
 * yolo_sequence: `steps` steps of streams 0 .. n-1 in one call, without a host synchronisation between them.  Step t < forced
 * (1 <= forced <= steps) feeds the one-hot row of tokens[t][b]; a later step feeds the token sampled from step t - 1.  A token
 * is sampled from the output of every step t >= forced - 1 as darknet's test_char_rnn samples it (rnn.c:290-293 and
 * sample_array, in fp32 and in their order of operations: probabilities below `clip` become 0, the rest are divided by their
 * sum, and the first class at which uniforms[t - forced + 1][b] minus the running sum reaches 0 is taken), into
 * tokens_out[t - forced + 1][b]: tokens_out is [steps - forced + 1][n].  uniforms == NULL is allowed only with steps == forced:
 * nothing is sampled (teacher forcing, valid_char_rnn's scoring form) and tokens_out is not written.  probs_out (may be NULL) is
 * [steps][n][N]: every step's [softmax] row as the layer wrote it.  test_char_rnn(seed, num): forced = len, steps = len - 1 + num.
 * loc: where tokens, uniforms, tokens_out and probs_out lie, all of them (YOLO_HOST: copied up once, back once at the end;
 * YOLO_DEVICE: read and written in place, stream-ordered; a device token outside 0 .. N-1 feeds a row of zeros).  States carry
 * over calls: 12 steps equal 5 steps, then 7 with forced = 1 on the last sampled token.  Every check stands in front of the
 * first launch: a refused call changes no state.
 *
 * yolo_set_temperature: the temperature of every [softmax] layer (rnn.c:261), > 0, until it is set again; yolo_reset_temperature
 * gives every [softmax] layer the temperature its cfg section names (valid_char_rnn sets none).
 * yolo_op_sample: the sampler alone over host arrays: probs [n][len] (len <= 8192), uniforms [n] -> out [n]. */
int yolo_vector_inputs(const yolo_ctx *ctx);                 /* N; 0: an image network */
int yolo_forward_vectors(yolo_ctx *ctx, const float *x, int n, int loc, float *out, size_t out_floats);
int yolo_sequence(yolo_ctx *ctx, int n, int steps, const int32_t *tokens, int forced, const float *uniforms, float clip,
                  int32_t *tokens_out, float *probs_out, int loc);
int yolo_set_temperature(yolo_ctx *ctx, float t);
int yolo_reset_temperature(yolo_ctx *ctx);
int yolo_op_sample(const float *probs, int n, int len, const float *uniforms, float clip, int32_t *out, int device);

/* ---- introspection / measurement ------------------------------------------------------------ */
/* Copies layer `index`'s output of the last forward as fp32 NHWC [n,H,W,C] to host (needs
 * keep_layers=1; without it only a conv layer's own tensor that still sits in its buffer after the
 * forward -- launched, no folded shortcut, buffer not reused by a later layer -- is served, anything else is
 * YOLO_ERR_STATE).  dims_out receives H,W,C.  Head (yolo/region) layers return the raw conv tensor. */
int yolo_layer_output(yolo_ctx *ctx, int index, int n, float *out, size_t out_floats, int *dims_out);
/* The staged network input of images 0..n-1 of the last forward as fp32 [n,H,W,S] to host, EVERY stored channel of a pixel: S = 8 for
 * an RGB network (3 real + 5 zero), roundup(C, 8) for C planes.  dims_out receives H,W,S; out == NULL: the dims only.
 * YOLO_ERR_UNSUPPORTED: a vector-input network, a split-fp16 image stored as pairs.  YOLO_ERR_STATE: the last forward's uint8 batch was
 * read in place by the fused first layers (nothing was staged). */
int yolo_staged_input(yolo_ctx *ctx, int n, float *out, size_t out_floats, int *dims_out);
/* Times `iters` forwards of batch n on the context stream with HIP events:
 * total_ms = wall per forward; conv_ms = the conv launches' share of it (all layers minus all-but-conv, bulk-timed)
 * (events around every conv launch, separate pass).  Either may be NULL.
 * The timing entry points (this one, yolo_time_layers, yolo_autotune) run the network on the INPUT OF THE LAST FORWARD.  When that call
 * was given a device-resident uint8 batch, the fused first layers read the caller's buffer in place: it must still be valid here.  A
 * timing pass over more images than that batch held reads the context's own (zero-initialised or previously staged) input instead. */
int yolo_time_forward(yolo_ctx *ctx, int n, int iters, float *total_ms, float *conv_ms);
/* What this chip sustains on a register-resident MFMA loop (v_mfma_f32_16x16x32_bf16, or _f16 when f16 != 0; random operands, 8 waves per
 * CU, back-to-back launches for `seconds`, the second half measured): TFLOP/s and the shader clock the waves held (GHz; s_memtime over
 * s_memrealtime).  bench.py prints both next to its roofline fraction: the same binary reads 9 % apart by box, and `frac / (tflops / peak)`
 * is what compares across boxes.  No counterpart in the reference.  stream: a hipStream_t or NULL. */
int yolo_calibrate(int device, void *stream, int f16, double seconds, float *tflops, float *clock_ghz);
/* The memory side of the yardstick: GB/s (bytes read + bytes written) of a streaming device-to-device copy between two 1 GiB buffers,
 * launched back to back for `seconds`.  The boxes of one pool differ in their matrix-pipe clock AND in what their memory system sustains;
 * bench.py prints both numbers (roofline.calib_tflops, roofline.calib_copy_gbs). */
int yolo_calibrate_copy(int device, void *stream, double seconds, float *gbs);
/* Per-layer kernel time (ms, averaged over iters) for batch n into ms_out[num_layers].  A [convolutional] layer with xnor=1 is its k_xconv
 * launch (xconv.hip: window staging as int8, the int8 MFMA, the epilogue) plus, for an activation outside the slope family, k_activate;
 * yolo_time_forward counts it among the convs (conv_ms). */
int yolo_time_layers(yolo_ctx *ctx, int n, int iters, float *ms_out);
/* Tries every conv tile configuration on every conv layer at batch n and keeps the fastest. */
int yolo_autotune(yolo_ctx *ctx, int n, int iters);
/* Read / restore the per-layer tile choices (one int per layer, -1 for non-conv layers or "library default") so a
 * tuned plan can be persisted by the caller.  cfgs has yolo_num_layers() entries. */
int yolo_get_tile_configs(const yolo_ctx *ctx, int32_t *cfgs);
int yolo_set_tile_configs(yolo_ctx *ctx, const int32_t *cfgs);
/* The tile configuration every layer would launch at batch n (1..max_batch) under the plan as it stands, into out[yolo_num_layers()]:
 * yolo_set_tile_configs stores any in-range id, and a layer whose id does not apply to it (another storage type's, a halo-staged form
 * its size does not tile into) runs its default instead.  -1: not a tunable layer (no [convolutional] section, a fixed kernel, a 1x1
 * conv computed in its producer's epilogue, an fp32 network).  Read-only: no device call, no state changed. */
int yolo_resolved_tile_configs(const yolo_ctx *ctx, int n, int32_t *out);

/* ---- single operators on host buffers (parity tests call the production kernels through these) - */
/* x [n,h,w,cin] fp32 NHWC, w_hwio [k,k,cin,cout], bias [cout] (or NULL), residual [n,ho,wo,cout] or NULL.
 * act: 0 linear, 1 leaky(0.1).  pad = k/2.  out [n,ho,wo,cout] fp32.  dtype selects the kernel family;
 * tile_cfg < 0 lets the library choose, otherwise forces one tile configuration (0..yolo_op_conv_num_cfgs()-1). */
int yolo_op_conv2d(const float *x, int n, int h, int w, int cin, const float *w_hwio, const float *bias,
                   int k, int stride, int cout, int act, const float *residual, float *out,
                   int dtype, int tile_cfg, int device);
/* ... with an explicit `padding` (darknet's padding= key; yolo_op_conv2d is padding = k / 2): k 1..11, any stride >= 1, out
 * [n, (h + 2 padding - k) / stride + 1, ..., cout], in fp32, bf16 and fp16; the fp8 and split-fp16 kernels keep k = 1 and 3 with
 * padding k / 2.  A conv of more than 25 taps runs the tile configurations that have the row / column tap-mask form only: a forced
 * tile_cfg without it is YOLO_ERR_UNSUPPORTED. */
int yolo_op_conv2d_pad(const float *x, int n, int h, int w, int cin, const float *w_hwio, const float *bias,
                       int k, int stride, int padding, int cout, int act, const float *residual, float *out,
                       int dtype, int tile_cfg, int device);
int yolo_op_conv_num_cfgs(void);
int yolo_op_upsample2x(const float *x, int n, int h, int w, int c, int semantics, float *out, int device);
int yolo_op_reorg(const float *x, int n, int h, int w, int c, int stride, int semantics, float *out, int device);
int yolo_op_maxpool(const float *x, int n, int h, int w, int c, int size, int stride, float *out, int device);
/* legacy-bilinear stretch of one uint8 image to [out_h,out_w,3] fp32: (value/255 then resize) * post_scale. */
int yolo_op_resize_u8_hw(const uint8_t *img, int h, int w, int out_h, int out_w, float post_scale, float *out, int device);
/* ... to [s,s,3]: the out_h == out_w call of the same kernel */
int yolo_op_resize_u8(const uint8_t *img, int h, int w, int s, float post_scale, float *out, int device);
/* V2/utils.py:13-27 `preprocess_image`'s arithmetic on the device: cv2.resize(float32 image, (ow, oh)) -- INTER_LINEAR, half-pixel centres,
 * restated from OpenCV's published CV_32F linear resize -- of one uint8 [h,w,3] image, optionally after BGR -> RGB (swap_rb), then
 * / divisor (the reference divides by 225.0, a typo kept).  out [oh,ow,3] fp32. */
int yolo_op_resize_cv2(const uint8_t *img, int h, int w, int oh, int ow, int swap_rb, float divisor, float *out, int device);
/* `detections_boxes` (V3/yolo_v3.py:329-347): (cx,cy,w,h,...) -> (x0,y0,x1,y1,...) over [n,rows,attrs] fp32 */
int yolo_op_detections_boxes(const float *det, int n, int rows, int attrs, float *out, int device);
/* head decode of raw [n,gh,gw,na*(5+classes)] fp32 (gh grid rows, gw columns) of a network input of img_h x img_w: yolo (logistic) or
 * region (softmax).  x and w follow the columns / the width, y and h the rows / the height; per-axis strides img_w / gw and img_h / gh */
int yolo_op_decode_hw(const float *raw, int n, int gh, int gw, int na, int classes, const float *anchors_wh,
                      int img_h, int img_w, int decode, int region, float *out, int device);
/* ... of raw [n,g,g,na*(5+classes)]: the gh == gw call of the same kernels */
int yolo_op_decode(const float *raw, int n, int g, int na, int classes, const float *anchors_wh,
                   int img_size, int decode, int region, float *out, int device);
/* threshold + NMS over det [n,rows,attrs] fp32.  nms_mode bits 8..19 / 20..31 carry image height / width for
 * YOLO_NMS_PER_CLASS (V2 pixel boxes); select_mode bit 8 set = rows already hold corners (x0,y0,x1,y1). */
/* darknet letterbox_image (embed = 1, DN/image.c:960-981) / resize_image (embed = 0, DN/image.c:1347-1389) of a planar
 * float image [3][ih][iw] into a planar w x h image, on the device.  Host buffers. */
int yolo_op_letterbox(const float *image_chw, int iw, int ih, int w, int h, int embed, float *out_chw, int device);
/* darknet's do_nms_sort (by_objectness = 0) / do_nms_obj (1), DN/box.c:21-89, on caller arrays (host): boxes [n] (cx,cy,w,h),
 * prob [n][classes], objectness [n]; suppressed entries are zeroed IN PLACE (prob[j][k], or objectness[j] and all of
 * prob[j]); detections whose objectness is 0 do not take part.  n <= 4096.  Array order is left unchanged (the
 * reference qsorts its array; callers only read the surviving probabilities). */
int yolo_op_nms_detections(const float *boxes_xywh, float *prob, float *objectness, int n, int classes, float thresh,
                           int by_objectness, int device);
int yolo_op_postprocess(const float *det, int n, int rows, int attrs, float score_thr, float iou_thr,
                        int max_out, int nms_mode, int select_mode, yolo_box *boxes_out,
                        int32_t *counts_out, int device);
/* ... with the source row of every record (see yolo_postprocess_rows); rows_out [n * max_out] host, or NULL */
int yolo_op_postprocess_rows(const float *det, int n, int rows, int attrs, float score_thr, float iou_thr,
                             int max_out, int nms_mode, int select_mode, yolo_box *boxes_out,
                             int32_t *counts_out, int32_t *rows_out, int device);

/* ---- classifier networks (darknet.py `classify`, D2T/darknet.py:117-123) ------------------------------------------------------
 * A cfg without a detection head whose output layer -- the last layer that is not [cost] -- is a [softmax] plans a CLASSIFIER
 * context: [avgpool] (global), [softmax] (keys groups, temperature) and [cost] (identity) are served in the fp32, bf16, fp16 and
 * split-fp16 configurations; the logits stay fp32.  For such a context yolo_num_rows / yolo_num_attrs are 0, yolo_last_layer_output*
 * returns the probabilities, and the detection entry points (yolo_postprocess*, yolo_detect*, yolo_head_raw, yolo_darknet_boxes*)
 * return YOLO_ERR_INVALID. */
/* outputs of the [softmax] layer of a classifier context; for a detector, attrs - 5 */
int yolo_num_classes(const yolo_ctx *ctx);
/* yolo_forward's image arguments, then the tail.  top_k == 0: probs_out receives the n x classes probability matrix (classes_out
 * is not written).  0 < top_k <= min(32, classes), a [softmax] with groups=1: the [softmax] launch itself selects, and only n x top_k
 * records are copied: classes_out / probs_out [n][top_k], probability descending, equal probabilities by ascending class (the order
 * of classify()'s stable sort by -prob).  out_loc: where classes_out / probs_out live. */
int yolo_classify(yolo_ctx *ctx, const void *images, int n, int fmt, int loc, float scale, int top_k,
                  int32_t *classes_out, float *probs_out, int out_loc);
/* ... over a ragged batch of native-size images through the one-launch fit of yolo_forward_images_u8 */
int yolo_classify_images_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc,
                            int top_k, int32_t *classes_out, float *probs_out, int out_loc);
/* ... over decoded video frames: yolo_forward_frames_u8's arguments (one launch converts and fits every frame; chroma upsampling and colour happen inside
 * it, no RGB copy of a frame is stored), then the tail.  Every fit yolo_classify_images_u8 takes except YOLO_FIT_CV2_BGR, which is refused for frames
 * (YOLO_ERR_UNSUPPORTED); YOLO_FIT_CENTER_CROP over a frame is darknet's `classifier predict` preprocessing.  The staged input, the probabilities and the
 * top_k records equal, bit for bit, those of yolo_classify_images_u8 over the RGB image yolo_frame_to_rgb_host yields.  Refused before any launch: what
 * yolo_classify_images_u8 refuses of a context and of top_k, what yolo_forward_frames_u8 refuses of descriptors (naming the frame), a network of other
 * than 3 planes (YOLO_ERR_UNSUPPORTED). */
int yolo_classify_frames_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc,
                            int top_k, int32_t *classes_out, float *probs_out, int out_loc);
/* ... over JPEG files (files[i], bytes[i]: file i, host): yolo_decode_jpegs of the batch, then yolo_classify_frames_u8 over its frame table on the device.
 * The pixels are the reference's load_image pixels, so with YOLO_FIT_CENTER_CROP this is `darknet classifier predict cfg weights file.jpg`.  Refused before
 * the IDCT launch: everything above, and every file yolo_decode_jpegs refuses (naming the file). */
int yolo_classify_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, int fit, int top_k, int32_t *classes_out,
                        float *probs_out, int out_loc);
/* ---- multi-view classification: darknet's ten-crop and flip averaging (DN/examples/classifier.c:234-301 validate_classifier_10,
 * `classifier valid10`; DN/examples/cifar.c:101-128 test_cifar_multi).  Every image is predicted over K views and the K rows are added.
 * YOLO_VIEWS_FLIP, K = 2: view 0 is the image fitted by `fit` (any fit yolo_classify_images_u8 takes), view 1 its mirror,
 * view1[y][x][c] = view0[y][net_w - 1 - x][c] (flip_image on the network-sized image; [net] yolo_input_mul / yolo_input_add as in view 0).
 * YOLO_VIEWS_TEN_CROP, K = 10, shift >= 0 (the reference's constant is 32): with W' = net_w + shift and H' = net_h + shift, R is darknet's
 * (float)p/255. image put through resize_image(., W', H') -- the image itself where it already has that size --, and pixel (x, y) of view v
 * is R[clamp(y + dy, 0, H' - 1)][cx] for v = 0..4 and R[..][W' - 1 - cx] for v = 5..9 (flip_image on R, then the same crops), with
 * cx = clamp(x + dx, 0, W' - 1) and (dx, dy) = (-s,-s), (s,-s), (0,0), (-s,s), (s,s) indexed by v % 5.  The reference's quirks are kept: the
 * (0,0) view is the top-left window, the -s views replicate the edge.  `fit` is not read.  No view is stored at W' x H'; the source bytes are
 * uploaded once. */
enum yolo_views { YOLO_VIEWS_FLIP = 1, YOLO_VIEWS_TEN_CROP = 2 };
/* one view: the crop offsets in pixels and whether the image is mirrored (16 bytes) */
typedef struct yolo_view { int32_t dy, dx, flip, pad; } yolo_view;
/* The views of a mode, in view order: FLIP {0,0,0}, {0,0,1}; TEN_CROP the table above for `shift`.  *count is always written; at most `cap`
 * views are written to out (cap = 0 / out = NULL: the count only).  YOLO_ERR_INVALID for an unknown `views`, shift < 0, count == NULL.
 * Host-side: no context, no device. */
int yolo_view_table(int views, int shift, yolo_view *out, int cap, int *count);
/* descs[n_images] whole images in `pixels`, as for yolo_classify_images_u8; n_images is NOT bound by max_batch.  Slots are ordered
 * image * K + view and run max_batch per network step, ceil(n_images * K / max_batch) steps: images may share a step, one image's views may
 * span steps.  One launch per step fits that step's slots straight from the source bytes; every slot's row -- the context's classifier
 * output, for a [softmax] with a tree in the context's hierarchy mode (classifier.c:287 is YOLO_HIER_LEAVES) -- is kept on the device, and
 * after the last step ONE launch forms sum[i][c] = ((((0 + p_0) + p_1) + ..) + p_{K-1}) in fp32 in view order (axpy_cpu's order), multiplies it
 * by `scale` once (1.0f leaves the bits alone, 1.0f / K gives the mean) and selects: top_k == 0: probs_out receives the n_images x classes
 * sums; 0 < top_k <= min(32, classes): classes_out / probs_out [n_images][top_k], value descending, equal values by ascending class (the order
 * of yolo_classify and of the reference's top_k), and only these records are copied.  The result does not depend on max_batch and is
 * bit-reproducible from run to run.  Every check runs before any launch.  YOLO_ERR_INVALID: a detector, map or vector-input context; a
 * descriptor yolo_forward_images_u8 refuses; an unknown `views`; shift < 0; top_k out of range; TEN_CROP with W' < 2 or H' < 2 (resize_image
 * divides by W' - 1) or extents that do not fit an int.  YOLO_ERR_UNSUPPORTED, naming what is refused: a context with recurrent state
 * (yolo_num_state_tensors > 0: a batch slot is a stream there), the cv2 fits on a network of C != 3 planes, fp8.  Planes networks are served
 * in both modes.  There is no captured-graph form. */
int yolo_classify_views_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n_images, int views, int fit,
                           int shift, int loc, float scale, int top_k, int32_t *classes_out, float *probs_out, int out_loc);
/* ... over decoded video frames, argument for argument: descs[n_images] frames in `pixels` (host or device), n_images NOT bound by max_batch (the call
 * carries a frame table of its own to the device).  Slot image * K + view is one view of frame `image`, fitted straight from the frame's planes by the
 * step's one launch: YOLO_VIEWS_FLIP under any fit yolo_classify_frames_u8 takes, YOLO_VIEWS_TEN_CROP as above.  The mirror and the crops act on
 * coordinates of the fitted / resized image; chroma is always indexed by the pixel's position in the FRAME (the nearest chroma of NV12 / I420, the JPEG
 * formats' upsamplers with their edge cases), so every staged slot, every sum and every top_k record equals, bit for bit, yolo_classify_views_u8 over the
 * RGB images yolo_frame_to_rgb_host yields.  Steps, the device-resident rows, the one reduction launch, `scale`, `top_k` and the independence from
 * max_batch are yolo_classify_views_u8's; so are its refusals, with yolo_forward_frames_u8's of descriptors (naming the frame), YOLO_FIT_CV2_BGR and a
 * network of other than 3 planes (YOLO_ERR_UNSUPPORTED).  No RGB copy of a frame or a view is stored; the source bytes are uploaded once. */
int yolo_classify_views_frames_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n_images, int views, int fit,
                                  int shift, int loc, float scale, int top_k, int32_t *classes_out, float *probs_out, int out_loc);
/* ... over JPEG files: ONE decode batch for all n_images files (n_images <= 65536 and the planes of the batch < 2^32 bytes, as yolo_decode_jpegs), then
 * the frame form over its table on the device -- `classifier valid10` over files.  Every refusal comes before the IDCT launch. */
int yolo_classify_views_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n_images, int views, int fit, int shift,
                              float scale, int top_k, int32_t *classes_out, float *probs_out, int out_loc);
/* the reduction launch alone over host arrays: rows [n * views][len] fp32 (slot = image * views + view), 1 <= views <= 32, any len >= 1 ->
 * sums_out [n][len]; top_k > 0 (<= min(32, len)): also classes_out / top_out [n][top_k] from the same launch (else NULL; NaN and -inf are
 * never selected) */
int yolo_op_view_reduce(const float *rows, int n, int views, int len, float scale, int top_k, float *sums_out, int32_t *classes_out,
                        float *top_out, int device);
/* darknet's [avgpool] on x [n,h,w,c] fp32 stored as `dtype` (YOLO_FP32 / BF16 / FP16 / FP16X2) first: out [n,c] fp32 */
int yolo_op_avgpool(const float *x, int n, int h, int w, int c, int dtype, float *out, int device);
/* Activations: the names DN/activations.c get_activation accepts.  YOLO_ACT_LINEAR .. YOLO_ACT_RELIE are the slope family, max(v, v * slope)
 * in every conv epilogue; the others are applied by a kernel of their own behind the layer's launch ("Activations"). */
enum yolo_activation { YOLO_ACT_LINEAR = 0, YOLO_ACT_LEAKY = 1, YOLO_ACT_RELU = 2, YOLO_ACT_RELIE = 3, YOLO_ACT_LOGISTIC = 4, YOLO_ACT_LOGGY = 5,
                       YOLO_ACT_ELU = 6, YOLO_ACT_RAMP = 7, YOLO_ACT_TANH = 8, YOLO_ACT_PLSE = 9, YOLO_ACT_STAIR = 10, YOLO_ACT_HARDTAN = 11, YOLO_ACT_LHTAN = 12 };
/* the code of an activation name as a cfg spells it, -1 for a name darknet does not know (the mapping the planner uses) */
int yolo_activation_code(const char *name);
/* out = act(x), x and out [n,h,w,c] fp32; x is stored as `dtype` (YOLO_FP32 / BF16 / FP16 / FP16X2) first and the result is rounded to it */
int yolo_op_activate(const float *x, int n, int h, int w, int c, int act, int dtype, float *out, int device);
/* darknet's [shortcut] (DN/blas.c:68-92 shortcut_cpu, then the activation): out [n,h2,w2,c2] = act(x + gather(from)), x [n,h2,w2,c2] the
 * layer's input, from [n,h1,w1,c1]: the first min(c1, c2) channels, sampled with stride w1 / w2 (or written to every (w2 / w1)-th
 * position), both integer divisions raised to 1.  Stored as `dtype` first, rounded to it once.  FP16X2: c1 and c2 multiples of 32. */
int yolo_op_shortcut(const float *x, int n, int h2, int w2, int c2, const float *from, int h1, int w1, int c1, int act, int dtype,
                     float *out, int device);
/* darknet's [softmax] on x [n][len] fp32, `groups` equal runs per row: probs_out [n][len]; top_k > 0 (groups == 1, <= 32): also
 * classes_out / topk_probs_out [n][top_k] from the same launch (else NULL) */
int yolo_op_softmax(const float *x, int n, int len, int groups, float temperature, int top_k, float *probs_out,
                    int32_t *classes_out, float *topk_probs_out, int device);

/* ---- hierarchical softmax: darknet's softmax trees (`tree=` on a [region] or [softmax] section; YOLO9000, the tree classifiers) ----
 * The tree file is opened as darknet opens it (relative to the working directory) when the context is created; an export artifact
 * embeds it.  A [region] head with a tree decodes ABSOLUTE class probabilities (hierarchy_predictions, DN/tree.c:37-51) into the
 * detection tensor; yolo_postprocess* / yolo_detect* score a box with its objectness and label it with hierarchy_top_prediction
 * (DN/tree.c:53-81) at the context's hier_thresh.  A [softmax] layer with a tree outputs CONDITIONAL probabilities, as
 * network_predict does. */
enum yolo_hierarchy_mode { YOLO_HIER_CONDITIONAL = 0, YOLO_HIER_ABSOLUTE = 1, YOLO_HIER_LEAVES = 2 };
/* hier_thresh of yolo_postprocess*, yolo_detect* and yolo_darknet_boxes* on a network with a tree head; default 0.5 (darknet.py's).
 * No effect on other networks. */
int yolo_set_hier_thresh(yolo_ctx *ctx, float hier_thresh);
/* what yolo_classify* returns (and selects its top-k over) for a tree classifier: the conditional probabilities (default), the
 * absolute ones (hierarchy_predictions), or the absolute ones with every inner node zeroed (only_leaves). */
int yolo_set_hierarchy_mode(yolo_ctx *ctx, int mode);
/* get_network_boxes with a `map` (DN/region_layer.c:415-420): yolo_darknet_boxes_at whose class columns are prob[j < 200] =
 * objectness * absolute[map200[j]] gated by thresh, zeros beyond; map200 == NULL: yolo_darknet_boxes_at.  YOLO_ERR_INVALID for a
 * head of fewer than 200 classes (the reference writes past prob[] there) or a map entry that is not a class. */
int yolo_darknet_boxes_map(yolo_ctx *ctx, int image, int w, int h, float thresh, int relative, const int32_t *map200, float *records, int cap, int *count);
/* The network's tree (the [region] head's, else the last [softmax] layer's that has one): node and group counts (0, 0: no tree) and,
 * where a pointer is given, a copy of parent / child / leaf [nodes] and group_offset / group_size [groups] as DN/tree.c builds them. */
int yolo_tree_geometry(const yolo_ctx *ctx, int32_t *nodes, int32_t *groups, int32_t *parent, int32_t *child, int32_t *group_offset,
                       int32_t *group_size, int32_t *leaf);
/* The same for a tree file, without a context or a device.  YOLO_ERR_INVALID with a message that names the line for a file that
 * cannot be opened, a parent that is not below its own index, children that are not one contiguous run, a first parent other than -1. */
int yolo_tree_read(const char *path, int32_t *nodes, int32_t *groups, int32_t *parent, int32_t *child, int32_t *group_offset, int32_t *group_size,
                   int32_t *leaf, char *err, size_t err_len);
/* Parse and plan a cfg for `dtype` without a device, with the defaults of a zeroed yolo_config (TF semantics, ratio decode, no
 * keep_layers, batch 1): the planner's status and message, or YOLO_OK.  What only a device can tell (memory, the per-context
 * batch limit) is not checked. */
int yolo_plan_check(const char *cfg_text, int dtype, char *err, size_t err_len);
/* The plan itself, as text, for `max_batch` and `keep_layers` (the other defaults as above): one line per layer --
 *   <index> <section> kernel=<tiled|halo|s2|-> fused=<none|stem|pair-stem|resblock|c3s2> launcher=<layer that issues the fused launch, -1>
 *   residual_from=<folded shortcut source, -2> tail_layer=<1x1 conv that can ride in this conv's epilogue, -1> storage=<index, -1>
 *   phys=<pooled buffer> def=<first writer> last=<last reader>
 * -- then `buffers <count> bytes <total>`.  YOLO_ERR_INVALID with the size needed when `out` is too small.
 * A [convolutional] section with groups > 1 runs the grouped kernel and prints, as a [deconvolutional] section does, kernel=- fused=none
 * launcher=-1 residual_from=-2 tail_layer=-1: it is no member of a fused launch, hosts no folded [shortcut] and no 1x1 tail.  The planner
 * refuses (YOLO_ERR_INVALID) groups that do not divide the input channels or the filters, and (YOLO_ERR_UNSUPPORTED) a grouped section in
 * the fp8 and split-fp16 configurations, as the first layer, or directly in front of a [yolo] / [region] / [detection] head. */
int yolo_plan_table(const char *cfg_text, int dtype, int max_batch, int keep_layers, char *out, size_t out_len, char *err, size_t err_len);
/* Everything the planner writes, as text, with the calling convention of yolo_plan_table: one `layer <index> <section> name=value ...` line per
 * layer (geometry, conv keys, padded sizes, types and pair form, fusion marks, route copies, head and classifier keys, storage and channel
 * offset), one `storage <index> def= last= bytes= phys= stride= dt= persistent=` line per storage, then one `context ...` line (input, rows,
 * attrs, the kind of network, normalisation, weights_count, conv_flops, phys_bytes[]).  Enumerations print as their numbers, floats and the
 * conv_flops double as %a.  The text is meant to be compared, not parsed: tests/test_plan_dump.py pins its SHA-256 per cfg. */
int yolo_plan_dump(const char *cfg_text, int dtype, int max_batch, int keep_layers, char *out, size_t out_len, char *err, size_t err_len);
/* single operators: x [n][len] fp32 logits, one softmax per group of the tree at tree_path, `mode` a yolo_hierarchy_mode -> out [n][len];
 * hierarchy_top_prediction of n rows of raw logits (temperature 1) walking down from the root -> labels_out [n] */
int yolo_op_tree_softmax(const float *x, int n, int len, const char *tree_path, float temperature, int mode, float *out, int device);
int yolo_op_tree_top(const float *x_logits, int n, const char *tree_path, float hier_thresh, int32_t *labels_out, int device);


/* ---- dense-prediction ("map") networks: segmentation masks, heat maps, U-Net-shaped cfgs (the reference: examples/segmenter.c, which
 * calls network_predict and then get_network_image) ------------------------------------------------------------------------------
 * Served sections: [deconvolutional] (DN/deconvolutional_layer.c; 1 <= size <= 7, 1 <= stride <= 4, 0 <= padding < size, pad=1 meaning
 * size / 2, a positive output; fp32, bf16 and fp16 configurations), [logistic], [activation] (any of the thirteen names), [l2norm], and
 * with darknet semantics [upsample] with stride 1..8 and scale.  A cfg whose [net] section says `yolo_output=map` (darknet ignores the
 * key) and that has no detection head plans a MAP context: its output is the image-shaped tensor of the last layer that is not [cost],
 * kept in fp32.  For such a context yolo_num_rows / yolo_num_attrs are 0, yolo_last_layer_output* returns the map planar (CHW per image,
 * what darknet's net->output holds), and the detection and classification entry points return YOLO_ERR_INVALID with a message that says
 * `map network`; the calls below return the same on a detector or a classifier. */
int yolo_output_map_geometry(yolo_ctx *ctx, int *h, int *w, int *c);
/* the map of images 0..n-1 of the last forward: NHWC fp32 [n][h][w][c], host */
int yolo_output_map(yolo_ctx *ctx, int n, float *out, size_t out_floats);
/* per map pixel of those images the arg-max over the channels, the lowest index winning a tie; 255 where the maximum is < thresh.
 * labels_u8 [n][h][w], host.  YOLO_ERR_UNSUPPORTED for a map of more than 255 channels. */
int yolo_label_map(yolo_ctx *ctx, int n, float thresh, uint8_t *labels_u8);
/* A ragged batch of native-size images (host: `pixels` packed as for yolo_forward_images_u8, ending where its last image ends): one fit
 * launch and one forward, then one kernel that writes image i's labels AT THAT IMAGE'S OWN SIZE, [h_i][w_i] uint8 at labels_u8 +
 * label_offsets[i] (NULL: back to back in image order; with offsets, the bytes between the images are zeroed).  Each native pixel takes
 * its map pixel by nearest lookup through the fit, in integers: pixel x of an image w wide, fitted to new_w columns at offset dx of a
 * net_w-wide input, with a map_w-wide map, reads column floor(((2x + 1) new_w + 2 w dx) map_w / (2 w net_w)), clamped to map_w - 1; the
 * same for y.  YOLO_FIT_LETTERBOX: new_w, new_h, dx, dy are darknet's letterbox_image integers; every other fit: new_w = net_w, dx = 0. */
int yolo_segment_images_u8(yolo_ctx *ctx, const uint8_t *pixels, const yolo_image_desc *descs, int n, int fit, float thresh,
                           uint8_t *labels_u8, const uint64_t *label_offsets);
/* ... over decoded video frames: `pixels` (bytes; host or device, `loc`) and descs[n] as for yolo_forward_frames_u8 -- one launch converts and fits, one
 * forward, then the same label kernel: frame i's labels at THAT FRAME'S OWN h_i x w_i, placed as above, equal byte for byte to yolo_segment_images_u8
 * over the RGB images yolo_frame_to_rgb_host yields.  Refused before any launch: a detector or a classifier, YOLO_FIT_CENTER_CROP, more than 255 channels,
 * and what yolo_forward_frames_u8 refuses (a bad descriptor, naming the frame; YOLO_FIT_CV2_BGR; a network of other than 3 planes). */
int yolo_segment_frames_u8(yolo_ctx *ctx, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc, float thresh,
                           uint8_t *labels_u8, const uint64_t *label_offsets);
/* ... over JPEG files: yolo_decode_jpegs of the batch, then the frame form on the device (the reference's `segmenter test` takes a file).  Every refusal,
 * those of the files included, comes before the IDCT launch. */
int yolo_segment_jpegs(yolo_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n, int fit, float thresh, uint8_t *labels_u8,
                       const uint64_t *label_offsets);
/* single operators.  deconv2d: x [n,h,w,cin] fp32 NHWC, w_iohw [cin][cout][size][size] (the order of darknet's weight files), bias [cout]
 * or NULL, act a yolo_activation, dtype YOLO_FP32 / BF16 / FP16 (the operands are stored as it first), out_f32 != 0: the fp32 store of a
 * 16-bit kernel (a map network's output layer); out [n, (h-1) stride + size - 2 padding, ..., cout] fp32 */
int yolo_op_deconv2d(const float *x, int n, int h, int w, int cin, const float *w_iohw, const float *bias, int size, int stride, int padding,
                     int cout, int act, int dtype, int out_f32, float *out, int device);
/* darknet's [convolutional] with groups= (DN/convolutional_layer.c:458-471): group g reads the input channels g cin/groups .. and writes the output
 * channels g cout/groups ..  x [n,h,w,cin] fp32 NHWC, w_oihw [cout][cin/groups][size][size] (the order of darknet's weight files), bias [cout] or NULL;
 * 1 <= size <= 7, 1 <= stride <= 4, 0 <= padding < size; groups >= 1 divides cin and cout (1 runs the same kernel with one group: a direct comparison
 * against yolo_op_conv2d); dtype and out_f32 as for yolo_op_deconv2d; out [n, (h + 2 padding - size) / stride + 1, ..., cout] fp32 */
int yolo_op_conv2d_grouped(const float *x, int n, int h, int w, int cin, const float *w_oihw, const float *bias, int size, int stride, int padding,
                           int cout, int groups, int act, int dtype, int out_f32, float *out, int device);
/* darknet's [convolutional] with xnor=1 (XNOR-Net layers, DN/convolutional_layer.c:28-49, 451-485): the input becomes +1 where it is > 0 and -1
 * elsewhere (+0, -0 and NaN give -1), a tap outside the image contributes 0; filter f becomes alpha_f * sign(w) with alpha_f = mean |w_f| (in float, added in the order
 * the reference's build adds: DESIGN.md 3.20); out = act(alpha_f * sum of the sign products + bias).  The sum runs on the int8 MFMA (xconv.hip).
 * x [n,h,w,cin] fp32 NHWC, stored as `dtype` before its sign is taken; w_oihw [cout][cin][size][size], bias [cout] or NULL; 1 <= size <= 11,
 * stride >= 1, padding >= 0; dtype and out_f32 as for yolo_op_deconv2d; out [n, (h + 2 padding - size) / stride + 1, ..., cout] fp32.
 * In a cfg: a [convolutional] section with xnor=1 plans a layer of this kind in the fp32, bf16 and fp16 configurations (yolo_plan_table prints
 * kernel=- fused=none, as for a grouped section); the planner refuses (YOLO_ERR_UNSUPPORTED) xnor=1 in the fp8 and split-fp16 configurations,
 * together with groups != 1, as the first layer, and directly in front of a [yolo] / [region] / [detection] head.  binary=1 without xnor, and
 * flipped=1, are read by nobody. */
int yolo_op_conv2d_xnor(const float *x, int n, int h, int w, int cin, const float *w_oihw, const float *bias, int size, int stride, int padding,
                        int cout, int act, int dtype, int out_f32, float *out, int device);
/* [l2norm]: per pixel x / sqrtf(sum over the channels of x^2); an all-zero pixel is NaN, as in the reference */
int yolo_op_l2norm(const float *x, int n, int h, int w, int c, int dtype, float *out, int device);
/* [normalization] / [lrn] (DN/normalization_layer.c:66-95) over the channels of every pixel: out[k] = x[k] * (kappa + alpha * (W(k) - g))^(-beta), W(k) the sum of
 * x[j]^2 over k - (size - 1) / 2 <= j <= k + size / 2 inside the tensor, g = x[size / 2]^2 -- the channel the reference's running sum never adds -- or 0 where
 * size / 2 == c.  1 <= size <= 17 and size / 2 <= c, else YOLO_ERR_UNSUPPORTED / YOLO_ERR_INVALID; a negative base is NaN, as in the reference */
int yolo_op_lrn(const float *x, int n, int h, int w, int c, int size, float alpha, float beta, float kappa, int dtype, float *out, int device);
/* darknet's [upsample]: nearest, out = scale * in, stride 1..8; out [n, h stride, w stride, c] */
int yolo_op_upsample(const float *x, int n, int h, int w, int c, int stride, float scale, int dtype, float *out, int device);
/* yolo_label_map's kernel on a host map [n,h,w,c] fp32: labels_out [n,h,w] */
int yolo_op_label_map(const float *map, int n, int h, int w, int c, float thresh, uint8_t *labels_out, int device);

#ifdef __cplusplus
}
#endif
#endif /* YOLO_HIP_H */
