// Private to libyolo_hip.so's host side: the planned network (layers, storage pool, context) and the functions its translation
// units share.  yolo_plan.cpp: darknet-cfg parser, planner, buffer pool, the plan queries that need no device.  yolo_pack.cpp: BN fold (fold_bn), filter packing
// (put_elt), fp8 scales, weight stream / export artifact.  yolo_run.cpp: launch sequence, input staging (input_fill_dst / input_filled), the two captured detect steps (graph_step over
// yolo_ctx::graph), what a forward leaves (forward_done), timing.  yolo_tune.cpp: tile selection rule, autotuner, tile plan.  yolo_api.cpp: create / destroy,
// introspection, darknet-flavoured views.  yolo_ops.cpp: single-operator entry points.  The side convs ([deconvolutional], groups=, xnor=1: is_side_conv below) share
// their argument fields and launch checks (SideConvArgs, kernels.h), their store (side_epilogue.h), one run_layer case and one operator body.
#pragma once
#include "../../include/yolo_hip.h"
#include "kernels.h"
#include "yolo_jpeg.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace yolo_impl {

enum LType { L_CONV, L_SHORTCUT, L_ROUTE, L_UPSAMPLE, L_MAXPOOL, L_REORG, L_YOLO, L_REGION, L_DETECT, L_LOCAL, L_AVGPOOL, L_SOFTMAX,
             L_DECONV, L_ACTIVATE, L_L2NORM,        // [deconvolutional] (deconv.hip), a side conv: is_side_conv; [logistic] / [activation]: k_activate over the producer's tensor; [l2norm]
             L_GCONV,                               // [convolutional] with groups > 1 (gconv.hip), a side conv; Layer::groups
             L_RECUR,                               // [rnn] / [gru] / [lstm] (rnn_ops.hip); Layer::rkind
             L_CRNN,                                // [crnn]: three 3x3 convs around a state map, run by the dense conv kernels; Layer::sub
             L_LRN, L_CROP,                         // [normalization] / [lrn]: k_lrn, Layer::size / lrn_*; [crop] at inference: k_crop, the output geometry and Layer::crop_adjust
             L_XCONV };                             // [convolutional] with xnor=1 (xconv.hip), a side conv: int8 signs in d_w, the per-filter scale in d_sc
enum ConvKernel { K_TILED, K_HALO, K_S2 };      // a conv's own kernel: the tiled family (fp32 / direct / pair form picked by dtype), conv_halo_c32_c64 (3x3/s1, 32 -> 64), conv_s2_c64_c128 (3x3/s2, 64 -> 128)
// the fused launch a conv is a member of, {members} -> launcher: conv_stem.hip {0, 1, optionally the 1x1 conv 2} -> 1; conv_stem_pair.hip (split-fp16) {0, 1} -> 1; conv_block.hip {1x1 i, 3x3 i + 1} -> i + 1; conv_c3s2.hip {conv3 i, stride-2 conv i + 2} -> i + 2 (both keep K_HALO / K_S2, the fall-back)
enum FuseKind { F_NONE, F_STEM, F_PSTEM, F_RESBLOCK, F_C3S2 };

struct Section { std::string type; std::map<std::string, std::string> kv; };

struct Layer {
    LType type;
    int H = 0, W = 0, C = 0;             // logical output geometry
    std::vector<int> in;                 // producer layer indices (-1 = network input)
    // conv
    int filters = 0, size = 0, stride = 1, pad = 0, bn = 0, act = ACT_LINEAR;      // act: the activation of the layer's own kernel -- a conv / [connected] / [local]: slope family only; a [shortcut]: any
    int post_act = ACT_LINEAR;           // conv / [connected] / [local] with an activation outside the slope family: applied in place on the output by k_activate after the layer's launch
    bool general = false;                // [shortcut]: a `from` tensor of another shape, or an activation -- runs as k_shortcut, never folded
    int cin = 0, cin_pad = 0, kpad = 0, cout_pad = 0;
    void *d_w = nullptr; float *d_b = nullptr; float *d_sc = nullptr;   // filters, bias, fp8 per-channel dequant scale (an L_XCONV: the epilogue's per-filter scale)
    void *d_wf = nullptr;                   // bf16 1x1 conv that can ride in its producer's epilogue: its filters in MFMA-fragment order (tail_fragments)
    void *d_wfrag = nullptr;                // 16-bit 3x3 / stride 1 conv a free-running halo id can run: d_w in MFMA-fragment order (filter_fragments)
    int in_dt = DT_BF16;                 // operand type of this conv's MFMA (filters are stored in it)
    int store_dt = DT_BF16;              // element type of this layer's output tensor (mixed plans: an fp8 network with bf16 islands, cfg key yolo_store)
    bool pair = false;                   // YOLO_FP16X2 networks: this layer's output tensor is split-fp16 PAIRS (interleaved per 32-channel group, 2 x the channels); false there:
                                         // plain fp16 (mixed plans, cfg key yolo_pair=0 on a [convolutional] section; layers that move data inherit their operands' form)
    int tile_cfg = -1;
    int residual_from = -2;              // >= -1: fused shortcut source
    bool head = false;                   // conv feeding a yolo/region layer: fp32 output
    float *d_obj = nullptr;              // ... feeding a [yolo] layer (bf16 / fp8 networks): compact plane of its objectness logits [max_batch * H * W][anchors]
    int kernel = K_TILED;                // its own kernel: what it runs when it issues a launch of its own.  This and the next line: written by the planner's marking passes only, read through the predicates below
    int fused = F_NONE, launcher = -1;   // the fused launch it is a member of, and the layer that issues that launch
    int fuse_n = 0; bool fuse_ok = false;      // run state (run_conv), on the launcher of a group that may fall back: does its kernel take batch fuse_n (0: not asked yet)?  Valid for the plan's life: the answer depends on n and plan-fixed geometry only
    // [connected] (YOLOv1's fully connected head, V1/YOLO_V1_Inference.py:196-206; DN/connected_layer.c:151): a 1x1 conv over the
    // producer's tensor flattened to one pixel per image; fc_h/w/c = the producer's geometry (darknet / the TF graph flatten CHW)
    bool fc = false; int fc_h = 0, fc_w = 0, fc_c = 0;
    // 7x7 / stride 2 / pad 3 first conv (YOLOv1): computed as a 4x4 / stride 1 conv over the 2x2 space-to-depth of the input
    bool s2d7 = false;
    int side = 0, sqr = 0;                  // [detection] head
    // fused 1x1 tail of the tiled conv kernel: `tail_layer` (on the producer) = index of the 1x1 conv that can be computed
    // in the producer's epilogue, `fused_into` (on that 1x1) = the producer; `tail_on` = the plan uses it
    int tail_layer = -1, fused_into = -1; bool tail_on = false;
    // shortcut/route bookkeeping
    bool noop = false;                   // output is an alias / was produced by someone else
    std::vector<int> copy_inputs;        // route inputs that must be copied (could not be placed)
    std::vector<int> copy_offsets;
    // pool / upsample / reorg
    int psize = 0, pstride = 0, ppad = 0;
    float up_scale = 1.f;                // [upsample] scale= (DN/upsample_layer.c: out = scale * in)
    float lrn_alpha = 1e-4f, lrn_beta = 0.75f, lrn_kappa = 1.f;      // [normalization] alpha= beta= kappa= (DN/parser.c:511-519); its size= is `size`
    bool crop_adjust = true;             // [crop]: out = in * 2 - 1 (false with noadjust=1: the plain copy)
    // [logistic] / [activation] (L_ACTIVATE; the activation is L.act): `inplace` = the layer aliases its producer's tensor and is ONE k_activate launch over it (nobody
    // else reads that tensor and nobody asked to keep it); else it copies into a tensor of its own first
    bool inplace = false;
    // head
    int na = 0, classes = 0, row_off = 0;
    std::vector<float> anchors;          // masked, in reference units
    // classifier tail: [softmax] keys; an [avgpool] whose fp32 input is pooled inside the launch of the [softmax] behind it (cls_ops.hip);
    // `cost`: a [cost] section (inference identity, never the network's output)
    int groups = 1; float temperature = 1.f, cfg_temperature = 1.f; bool pool_fused = false; bool cost = false;
    int tree = -1;                       // [region] / [softmax] with tree=: index into yolo_ctx::trees (hierarchical softmax), else -1
    // [rnn] / [gru] / [lstm] (L_RECUR; DESIGN.md "Recurrent layers"): `filters` units over the flattened producer (fc_h / fc_w / fc_c its geometry, cin = their
    // product, as a [connected] layer reads it); act: an [rnn]'s activation, any code (its kernel applies it).  One stacked matrix per launch: d_w / d_b
    // the first launch's (RK_RNN_STATE, RK_GRU_GATES, RK_LSTM), d_w2 / d_b2 the second's (RK_DENSE, RK_GRU_BLEND); d_b / d_b2 hold bx then bh.  The state of
    // max_batch streams lives in allocations of the layer's own, outside the pool (zero at yolo_create): d_h the state as the MFMA operand (storage type),
    // d_hn what the step writes before it becomes d_h, d_h32 / d_z / d_rh a [gru]'s fp32 state, update gate and r * h, d_c an [lstm]'s fp32 cell
    int rkind = 0, rshortcut = 0, rtanh = 0;      // RECUR_*; [rnn] / [crnn] shortcut=; [gru] tanh=
    // [crnn] (L_CRNN, DN/crnn_layer.c): sub = its input, self and output convs (3x3 / stride 1 / pad 1, L_CONV layers of their own with filters and bias, seen by
    // no marking pass); `filters` = output_filters, cin = hidden_filters.  Its state map [max_batch][H][W][roundup(hidden, 8)] is d_h, in the storage type (conv_self
    // reads it); d_rh holds [state +] act(conv_in(x)), d_hn the new state until the step's last read of the old one is issued
    std::vector<Layer> sub;
    void *d_w2 = nullptr; float *d_b2 = nullptr;
    void *d_h = nullptr, *d_hn = nullptr, *d_rh = nullptr; float *d_h32 = nullptr, *d_z = nullptr, *d_c = nullptr;
    // storage
    int storage = -1; int ch_off = 0;    // view = storage buffer + channel offset
    TView out;
};

// a softmax tree (DN/tree.c:83-139 read_tree): the file's text (kept for the export artifact), its arrays, and their device copy
struct Tree {
    std::string path, text;
    int n = 0, groups = 0, levels = 0;
    std::vector<int> parent, child, goff, gsize, leaf, order, lvl;      // order / lvl: see TreeDev (kernels.h)
    int *d_all = nullptr; TreeDev dev{};
};

enum { RECUR_RNN = 0, RECUR_GRU = 1, RECUR_LSTM = 2 };
// one state tensor of a recurrent layer as yolo_get_state / yolo_set_state number them (layer order; an [lstm]: h, then c)
struct StateRef { int layer; bool cell; };

struct Storage { int def = 1 << 30, last = -1; size_t bytes = 0; int phys = -1; int stride = 0; int dt = DT_BF16; bool persistent = false; };


}  // namespace yolo_impl
using namespace yolo_impl;

struct yolo_ctx {
    std::string err, cfg_text;
    int device = 0;
    hipStream_t stream = nullptr; bool own_stream = false;
    int max_batch = 1, dtype = YOLO_BF16, semantics = YOLO_SEM_TF, decode = YOLO_DECODE_RATIO, keep_layers = 0;
    int in_h = 0, in_w = 0, in_c = 0;
    // vector-input network ([net] yolo_input=vector, inputs=N: char-rnn): vec_n = N (0: an image network), in_h = in_w = 1, in_c = N, `input` one row of roundup(N, 8) elements per
    // stream.  d_seq: yolo_sequence's slab (forced tokens, uniforms, sampled tokens, probabilities), grown on demand and never shrunk
    int vec_n = 0; void *d_seq = nullptr; size_t seq_cap = 0;
    std::vector<Layer> layers;
    std::vector<Storage> storages;
    std::vector<void *> phys; std::vector<size_t> phys_bytes;
    TView input;                          // [n, in_h, in_w, 8]
    void *d_zeros = nullptr;
    void *d_stage = nullptr; size_t stage_bytes = 0;     // host->device image staging
    TView s2d;                            // [n, in_h/2, in_w/2, 32]: space-to-depth of the input for a 7x7/2 first conv
    const uint8_t *stem_u8 = nullptr; float stem_scale = 1.f; int stem_u8_n = 0;      // uint8 image (of stem_u8_n images) the fused stem reads itself (no conversion launch), or nullptr: c->input.  May be the CALLER's buffer: only valid for a pass over <= stem_u8_n images while the caller keeps it (yolo_time_*)
    float in_mul = 1.f, in_add = 0.f;     // input normalisation after the /255: v * in_mul + in_add ([net] yolo_input_mul / yolo_input_add)
    float *d_det = nullptr; int rows = 0, attrs = 0;
    // classifier context: no detection head, the output layer (the last one that is not [cost]) is a [softmax].  cls_layer: that layer
    // (-1: a detector); cls_topk: what the next forward's [softmax] launch selects (yolo_classify*), into d_cls_idx / d_cls_prob [max_batch][32];
    // cls_mode: the form (TREE_*) a tree classifier's output layer writes during that forward
    int cls_layer = -1, cls_topk = 0, cls_mode = 0; int *d_cls_idx = nullptr; float *d_cls_prob = nullptr;
    // map context ([net] yolo_output=map): no detection head, no [softmax]; the output is the image-shaped tensor of map_layer, the last layer
    // that is not [cost] (-1: not a map network).  d_map_f32: its dense fp32 copy (+ the planar one of yolo_last_layer_output*), d_map_labels:
    // uint8 labels of yolo_label_map / yolo_segment_images_u8, d_label_off: where each image's labels begin (yolo_segment_images_u8)
    int map_layer = -1; float *d_map_f32 = nullptr; size_t map_f32_cap = 0; uint8_t *d_map_labels = nullptr; size_t map_labels_cap = 0; unsigned long long *d_label_off = nullptr;
    // lean detect path (yolo_detect*): the decode writes scores, labels and the four box numbers of every row, not the tensor
    bool lean_cnt_dirty = false;
    void *d_lean_list = nullptr; unsigned *d_lean_cnt = nullptr;      // lean decode: list of the boxes that pass the objectness pre-filter + its counter (one word)
    float *d_box4 = nullptr; bool lean = false, det_valid = false, lean_ok = false; float lean_thr = 0.f; int lean_heads = 0;      // lean_heads: [yolo] heads when all can share one decode launch, else 0
    // postprocess workspace
    float *d_scores = nullptr; int *d_labels = nullptr; int *d_cand = nullptr; unsigned long long *d_keys = nullptr;
    float4 *d_sbox = nullptr; int *d_slabel = nullptr; float *d_sscore = nullptr; int rows_pow2 = 0;
    void *d_boxes = nullptr; int *d_counts = nullptr; int boxes_cap = 0;
    int *d_srow = nullptr, *d_rows = nullptr;      // rows_out support: row of every sorted candidate [max_batch * rows], staging [boxes_cap]
    // darknet-flavoured outputs (yolo_darknet_boxes / yolo_last_layer_output): records, row list, count, last layer's planar output
    float *d_dn_rec = nullptr; int *d_dn_src = nullptr; int *d_dn_count = nullptr; float *d_dn_last = nullptr; size_t dn_last_cap = 0;
    // the captured detect steps (graph_step, yolo_run.cpp): graph[0] yolo_detect_graph's, graph[1] yolo_detect_images_graph's -- one each: a caller that alternates the two recaptures neither.
    // key: every argument the captured launches hold, both entry points' in one struct (memset to zero before it is filled: memcmp compares it; no image size or offset: those live in d_descs, rewritten before every launch)
    struct GraphKey { const void *src; size_t bytes; int n, fmt, fit, units; float scale, st, it; int mo, nm, sm; void *bo, *co; };
    struct GraphStep { GraphKey key; hipGraphExec_t exec; int state; } graph[3] = {};      // state 0: next call eager, 1: next call captures, 2: replay, -1: capture unsupported (sticky).  graph[2]: yolo_detect_frames_graph's
    // ragged batches of native-size images (yolo_*_images_*): descriptor table [max_batch] (device), staging of a host packed buffer, the
    // geometry the last such forward ran with (what the box mapping of its postprocess reads)
    ImgDesc *d_descs = nullptr; void *d_pix = nullptr; size_t pix_cap = 0;
    int geom_fit = -1, geom_n = 0;
    // decoded video frames (yolo_*_frames_*): the frame table [max_batch] (device) the fit launch reads; d_descs then holds {plane 0's offset, h, w} of the same
    // frames, so the box mapping reads what it reads for images.  h_geom: the host side of that copy, kept here so that it outlives the asynchronous upload
    FrameDesc *d_frames = nullptr; std::vector<ImgDesc> h_geom;
    // JPEG files (yolo_decode_jpegs): the batch being decoded -- parsed headers, its frame table over the surface, the IDCT's plane table, where
    // each file's blocks begin --; h_jin: pinned staging of {plane table, coefficients}, d_jin: its device copy, d_jpeg: the surface of component planes the
    // frame table describes (all three grown on demand, never shrunk; the surface in steps of 4 MiB, so that batches of like size present one buffer to the captured
    // frames step).  jpeg_up: recorded behind the upload; the next decode waits for it before it overwrites the staging
    struct JpegBatch {
        std::vector<yolo_impl::JpegFile> files; std::vector<yolo_frame_desc> descs; std::vector<JpegPlane> planes; std::vector<size_t> first_block;
        size_t blocks = 0, surface = 0, view_bytes = 0;
    } jpeg;
    void *h_jin = nullptr, *d_jin = nullptr; size_t jin_cap = 0; uint8_t *d_jpeg = nullptr; size_t jpeg_cap = 0; hipEvent_t jpeg_up = nullptr; bool jpeg_up_pending = false;
    // what the last decode cost (yolo_jpeg_decode_times): wall time of the entropy stage, bytes uploaded, events in front of the upload, behind it, behind the IDCT
    // ([3]: behind k_jpeg_entropy, in front of the IDCT, recorded by a decode that ran the device's entropy stage)
    hipEvent_t jpeg_t[4] = {nullptr, nullptr, nullptr, nullptr}; double jpeg_entropy_ms = 0; size_t jpeg_upload_bytes = 0;
    // the entropy stage over restart intervals (yolo_set_jpeg_entropy).  jpeg_entropy_mode: YOLO_JPEG_ENTROPY_*; jent: the eligible files of the
    // batch being decoded as k_jpeg_entropy reads them; h_jst: pinned staging of {file records, workgroup table, interval table} and, behind them, of the status
    // words that come back; d_jst: its device copy; d_jstream: the eligible files' bytes (all grown on demand, never shrunk).  je_*: what the last decode did
    // (yolo_jpeg_entropy_times)
    int jpeg_entropy_mode = 0;
    yolo_impl::JpegEntropyPlan jent; std::vector<std::vector<yolo_impl::JpegInterval>> jpeg_iv;
    void *h_jst = nullptr, *d_jst = nullptr; size_t jst_cap = 0; uint8_t *d_jstream = nullptr; size_t jstream_cap = 0;
    int je_dev_files = 0, je_host_files = 0, je_intervals = 0; double je_scan_ms = 0; size_t je_stream_bytes = 0;
    // tiled detection (yolo_detect_tiled_u8): ONE allocation, grown on demand and never shrunk, that holds the window table, the image table, every
    // image's merged candidate list and k_nms_image's workspace over those lists (tile_slab, yolo_run.cpp)
    void *d_tile = nullptr; size_t tile_cap = 0;
    // multi-view classification (yolo_classify_views_u8): ONE allocation, grown on demand and never shrunk, that holds the view table, every slot's
    // classifier row, the summed rows, the selection's scratch and the top-k records (ViewSlab, yolo_run.cpp)
    void *d_views = nullptr; size_t views_cap = 0;
    // hierarchical softmax ("Softmax trees"): the trees of the cfg's tree= keys; tree_head: the [region] layer that has one
    // (-1: none); hier_thresh: yolo_set_hier_thresh; hierarchy_mode: yolo_set_hierarchy_mode; tree_full: YOLO_TREE_FULL forces the full
    // decode in yolo_detect*; lean_hier: the hier_thresh the last descent-form decode labelled its rows with
    std::vector<Tree> trees; int tree_head = -1; float hier_thresh = 0.5f, lean_hier = 0.f; int hierarchy_mode = 0; bool tree_full = false;
    bool fragw = true;                    // the free-running halo forms read their filters as fragments from global memory (Layer::d_wfrag); false under YOLO_NO_FRAGW=1: through LDS
    int *d_map200 = nullptr;
    bool weights_loaded = false;
    int scores_mode = -1;                 // what d_scores/d_labels hold: 0 max(obj*cls) from the decode, 1 objectness, -1 nothing
    size_t weights_count = 0;
    double conv_flops = 0;
    int last_n = 0;
    std::vector<StateRef> states;         // the state tensors of the recurrent layers (empty: a pure function of the batch)
    void *d_state_keep = nullptr;         // the timing entry points' copy of every state, handed back when they return (state_keep / state_restore)
    // frame averaging (yolo_set_frame_average; DESIGN.md "Frame averaging"): avg_k = K frames (1: off, nothing allocated).  d_ring [K][max_batch][rows * attrs] fp32:
    // the last K activated head tensors of every stream, head h at row_off * attrs; d_ring_pos [max_batch]: the slot a stream's next step writes, advanced on
    // the device after the step's last decode.  d_ring_keep [max_batch][rows * attrs]: the one slot per stream the timing entry points overwrite, which run
    // with the positions standing still (ring_frozen) and hand that slot back (state_keep / state_restore).  Not recurrent states, no part of the plan
    int avg_k = 1; float *d_ring = nullptr, *d_ring_keep = nullptr; int *d_ring_pos = nullptr; bool ring_frozen = false;
    size_t ring_elems() const { return (size_t)rows * attrs; }
    // fp8 scheme: stored value = e4m3(real / scale).  user_scale[i] is what yolo_set_act_scales gave for
    // layer i (1 by default); eff_scale[i] is the scale of the tensor layer i's view holds (inherited through
    // upsample / maxpool / reorg / single-input route; NaN for multi-input routes, which are per channel).
    std::vector<float> user_scale, eff_scale;
    // split fp16 storage (YOLO_FP16X2): a layer output of C channels is [pixel][2 * Cp] f16, Cp = roundup(C, 32), interleaved per 32-channel group (32 hi | 32 lo);
    // the network input [pixel][3 * 8]: hi | lo | hi blocks of its 8 padded channels
    bool split() const { return dtype == YOLO_FP16X2; }
    bool in_pair = false;                 // ... the network input is stored as pairs ([net] yolo_pair_input, default 1 in a YOLO_FP16X2 network)
    bool pair_of(int idx) const { return idx < 0 ? in_pair : layers[idx].pair; }      // is tensor `idx` (-1: the input) stored as pairs?
    float *d_f32a = nullptr, *d_f32b = nullptr; size_t f32_cap = 0;      // split mode: fp32 staging of one tensor (input conversion, upsample / pool / reorg run in fp32 between a join and a split)
    int act_dt() const { return dtype == YOLO_FP32 ? DT_F32 : dtype == YOLO_FP8 ? DT_FP8 : (dtype == YOLO_FP16 || dtype == YOLO_FP16X2) ? DT_F16 : DT_BF16; }
    bool half_like() const { return dtype == YOLO_BF16 || dtype == YOLO_FP16; }      // 16-bit storage: the same kernels, the same plan
    int gran() const { return dtype == YOLO_FP8 ? 16 : 8; }            // channel granule = one 16-B piece (8 for fp32 too)
    size_t esize() const { return dt_size(act_dt()); }
};

namespace yolo_impl {

int fail(yolo_ctx *c, int code, const char *fmt, ...);
#define HIPCK(c, expr)                                                                       \
    do { hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail(c, YOLO_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)

inline int roundup(int x, int m) { return (x + m - 1) / m * m; }
inline int pair_width(int C) { return 2 * roundup(C, 32); }      // elements per pixel of an interleaved split-fp16 pair tensor of C channels (32 hi | 32 lo per group)
inline int gran_of(int dt) { return dt == DT_FP8 ? 16 : 8; }      // channels per 16-byte piece (8 for fp32 tensors too)
inline void drop_graph(yolo_ctx *c)      // a plan / parameter / buffer change: no captured detect step may be replayed
{
    for (auto &g : c->graph) { if (g.exec) { hipGraphExecDestroy(g.exec); g.exec = nullptr; } if (g.state > 0) g.state = 0; }
}

// ---- layer kinds the planner asks for by more than one name ----
inline bool is_side_conv(const Layer &L) { return L.type == L_DECONV || L.type == L_GCONV || L.type == L_XCONV; }      // SideConvArgs (kernels.h): a kernel of its own, never a member of a fused launch, neither end of a 1x1 tail, nothing for the tile tuner
inline bool has_packed_filters(const Layer &L) { return L.type == L_CONV || L.type == L_LOCAL || is_side_conv(L); }      // d_w / d_b [/ d_sc] blobs of an export artifact
inline bool computes(const Layer &L) { return L.type == L_CONV || is_side_conv(L) || L.type == L_RECUR || L.type == L_CRNN; }      // has filters and an MFMA kernel ([connected] is an L_CONV; [local] is not among them)
inline bool has_state(const Layer &L) { return L.type == L_RECUR || L.type == L_CRNN; }
inline bool is_head_layer(const Layer &L) { return L.type == L_YOLO || L.type == L_REGION || L.type == L_DETECT; }      // a detection head: no tensor of its own, an alias of the conv in front of it

// ---- what a conv layer's (kernel, fused, launcher) mean: the only places that enumerate fused kinds; `i` = the layer's own index.  Where two of the old lists disagreed: NOTEBOOK 2026-10-18 ----
inline bool fused_may_fall_back(const Layer &L) { return L.fused == F_RESBLOCK || L.fused == F_C3S2; }      // to its members' own kernels, where the fused launch's 32-bit windows do not hold the batch; the stems cannot (layer 0 has no storage) and refuse
inline bool never_stored(const Layer &L, int i) { return L.fused != F_NONE && i < L.launcher; }      // the tensor stays in LDS in the fused plan: every member in front of its launcher
inline bool input_never_loaded(const Layer &L, int i) { return L.fused != F_NONE && L.fused != F_PSTEM && i >= L.launcher; }      // (yolo_conv_bytes) the pair stem's layer 1 is left out: not intended, kept (the bench's roofline line)
inline bool fixed_kernel(const Layer &L) { return L.kernel != K_TILED || L.fused != F_NONE; }      // nothing for the tile tuner to choose, no 1x1 tail to host
inline bool window_check_skipped(const Layer &L, int i) { return L.fused != F_NONE && (!fused_may_fall_back(L) || (L.fused == F_RESBLOCK && i < L.launcher)); }      // by allocate()'s 2 GiB check.  A resblock's inner 1x1 should be checked like the other members of groups that may fall back: not intended, kept, unreachable in darknet-53
inline bool rides_as_tail(const yolo_ctx *c, const Layer &L) { return L.fused_into >= 0 && c->layers[L.fused_into].tail_on; }      // computed in its producer's epilogue (tail_on is toggled after planning)
inline bool issues_launch(const yolo_ctx *c, int i) { const Layer &L = c->layers[i]; return (L.fused == F_NONE || L.launcher == i) && !rides_as_tail(c, L); }      // in the fused plan (the members of a group that fell back do so too)

// yolo_pack.cpp
uint16_t f2bf(float f);
uint16_t f2h(float f);
uint8_t f2e4m3(float f);
void pack_conv(const Layer &L, const float *bn_or_bias, const float *w_oihw, int wdt, const float *in_scale,
               std::vector<uint8_t> &wbuf, std::vector<float> &bias, std::vector<float> &osc, int semantics = YOLO_SEM_TF, int split = 0);      // split: 0 plain, 1 pair input in three blocks (the image), 2 interleaved pair input
// [deconvolutional]: w_iohw [cin][filters][k][k] (darknet's order) -> the per-phase blocks of DeconvArgs, batch norm folded as pack_conv folds it
void pack_deconv(const Layer &L, const float *bn_or_bias, const float *w_iohw, int wdt, std::vector<uint8_t> &wbuf, std::vector<float> &bias, int semantics = YOLO_SEM_TF);
// [convolutional] with groups > 1: w_oihw [filters][cin / groups][k][k] -> the block-diagonal bundles of GConvArgs, batch norm folded as pack_conv folds it
void pack_gconv(const Layer &L, const float *bn_or_bias, const float *w_oihw, int wdt, std::vector<uint8_t> &wbuf, std::vector<float> &bias, int semantics = YOLO_SEM_TF);
// [convolutional] with xnor=1: w_oihw [filters][cin][k][k] -> int8 signs in the fragment order of XConvArgs (L.stride decides the channel chunks), the
// per-filter scale alpha_f (* the folded batch-norm scale) and the folded shift, cout_pad entries each
void pack_xconv(const Layer &L, const float *bn_or_bias, const float *w_oihw, std::vector<uint8_t> &wbuf, std::vector<float> &scale, std::vector<float> &bias, int semantics = YOLO_SEM_TF);
inline size_t filter_bytes(const Layer &L) { return (size_t)L.cout_pad * L.kpad * (L.type == L_XCONV ? 1 : dt_size(L.in_dt)); }      // of d_w: a conv, deconv, grouped or xnor conv
float h2f(uint16_t h);
void resolve_scales(yolo_ctx *c);
void channel_scales(const yolo_ctx *c, int idx, std::vector<float> &out);
int tail_fragments(yolo_ctx *c);
void fragment_order(const uint16_t *src, int rows, int K, uint16_t *dst);      // [row][K] 16-bit filters -> [row / 16][K / 32][64 lanes][8]
int filter_fragments(yolo_ctx *c);      // Layer::d_wfrag of every conv a free-running halo id can run (none under YOLO_NO_FRAGW)
// recurrent layers: the sublayers of layer L in file order -- {inputs, 1 for a sublayer over the state} per sublayer -- and the floats one holds
int recur_sublayers(const Layer &L, int subs[8]);
inline size_t connected_floats(int inputs, int outputs, int bn) { return (size_t)outputs * (1 + (size_t)inputs + (bn ? 3 : 0)); }
struct RecurGeom { int mode[2], Mp[2], Kx[2], Kh[2], x_len, s_stride, launches; };      // of a planned (and, for x_len, allocated) layer: its one or two launches
RecurGeom recur_geom(const yolo_ctx *c, const Layer &L);
size_t recur_blob_bytes(const yolo_ctx *c, const Layer &L, int k);      // k = 0..3: d_w, d_b, d_w2, d_b2 (0: none)
size_t state_elems(const yolo_ctx *c, const Layer &L);      // elements of one stream's state tensor as stored (padded): roundup(units, 8), a [crnn]: H * W * roundup(hidden, 8)
// yolo_run.cpp: states across forwards of the library's own
int state_keep(yolo_ctx *c);
int state_restore(yolo_ctx *c);
// yolo_tree.cpp
int parse_tree(const std::string &text, Tree &t, std::string &err);      // YOLO_OK or YOLO_ERR_INVALID with a message that names the line
int load_tree(const std::string &path, Tree &t, std::string &err);        // ... from the artifact being read (g_tree_texts) or the file, as darknet opens it
std::vector<int> pack_tree(const Tree &t, size_t at[7]);      // the seven arrays of TreeDev in one buffer; at[k]: where array k begins
TreeDev tree_dev(const Tree &t, const int *base, const size_t at[7]);
int upload_tree(yolo_ctx *c, Tree &t);
void free_tree(Tree &t);
int score_tree_rows(yolo_ctx *c, int n);      // full form: d_scores / d_labels of the n images' decoded rows at the context's hier_thresh
extern thread_local const std::vector<std::pair<std::string, std::string>> *g_tree_texts;      // (path, text) of the trees an artifact embeds, while it is loaded
// yolo_plan.cpp
bool parse_cfg(const char *text, std::vector<Section> &out, std::string &err);
int build_plan(yolo_ctx *c, const std::vector<Section> &secs);
int allocate(yolo_ctx *c);
TView view_of(const yolo_ctx *c, int idx);
// yolo_run.cpp
ConvArgs conv_args(const yolo_ctx *c, const Layer &L, int n);
DeconvArgs deconv_geometry(int size, int stride, int pad, int h, int w, int cin_pad, int filters, int act, int in_dt);      // everything of DeconvArgs but pointers, strides, N, out_dt, Cstore
GConvArgs gconv_geometry(int size, int stride, int pad, int h, int w, int cin, int filters, int groups, int act, int in_dt);      // the same of GConvArgs
XConvArgs xconv_geometry(int size, int stride, int pad, int h, int w, int cin, int filters, int act);      // the same of XConvArgs
void side_layout(const Layer &L, int &kpad, int &cout_pad);      // a side conv's cout_pad * kpad filter elements, from its kind's geometry; reads type, size, stride, pad, filters, groups, cin, cin_pad, in_dt
int run_layer(yolo_ctx *c, int i, int n);
int stage_in(yolo_ctx *c, const void *images, int n, int fmt, int loc, float scale);
int run_network(yolo_ctx *c, int n, bool lean = false, int fit = -1);      // fit >= 0: the input is a fitted ragged batch (forward_done records its geometry)
int copy_out(yolo_ctx *c, void *dst, const void *src, size_t bytes, int loc);
int output_layer(const yolo_ctx *c);      // the network's output: the last layer that is not [cost] (DN/network.c:699-706)
int need_image(yolo_ctx *c, const char *what);         // YOLO_ERR_INVALID with a message for a vector-input context ([net] yolo_input=vector)
int need_detector(yolo_ctx *c, const char *what);      // YOLO_ERR_INVALID with a message for a classifier or a map context
int post_args_ok(yolo_ctx *c, int max_out, int nms_mode, int select_mode);
struct PostGeom { int fit, pixels; };      // per-image box mapping of a ragged batch (yolo_box_units), over c->d_descs
int post(yolo_ctx *c, const float *det, int n, int rows, int attrs, float score_thr, float iou_thr, int max_out,
         int nms_mode, int select_mode, int img_h, int img_w, int scores_ready, yolo_box *boxes_out, int32_t *counts_out, int out_loc, int32_t *rows_out = nullptr,
         const PostGeom *geom = nullptr);
// decoded video frames: YOLO_OK, or YOLO_ERR_INVALID with what is wrong with frame `i`'s descriptor inside a packed buffer of `bytes` bytes in `msg` (yolo_run.cpp)
int frame_desc_check(const yolo_frame_desc &d, size_t bytes, int i, std::string &msg);
// JPEG files: a parsed file's planes behind `surface` bytes of a surface and its blocks behind `block` blocks of a coefficient array -> its frame descriptor and
// its f.comps rows of the IDCT's table; both ends advance (yolo_run.cpp)
void jpeg_place(const JpegFile &f, size_t &surface, size_t &block, yolo_frame_desc *desc, JpegPlane *rows);
// yolo_api.cpp: map networks
int need_map(yolo_ctx *c, const char *what);      // YOLO_ERR_INVALID with a message for a detector or a classifier context
int map_to_f32(yolo_ctx *c, int n);
int map_f32_view(yolo_ctx *c, int n, const float **map, int *stride);
int map_labels_room(yolo_ctx *c, size_t bytes);
// yolo_ops.cpp
extern thread_local std::string g_op_err;
TView make_view(void *p, int n, int h, int w, int c, int stride, int dt);

}  // namespace yolo_impl
