// C ABI of libyolo_hip.so (include/yolo_hip.h): context life cycle, introspection, and the darknet-flavoured views of the last forward
// that the veneer libdarknet_hip.so is built on.  The rest of the exports live next to what they drive: yolo_pack.cpp (weights,
// artifact), yolo_run.cpp (forward / detect / timing / tile plans), yolo_ops.cpp (single operators).
#include "yolo_ctx.h"

namespace yolo_impl {

int need_map(yolo_ctx *c, const char *what)
{
    if (int r = need_image(c, what)) return r;
    if (c->map_layer < 0) return fail(c, YOLO_ERR_INVALID, "%s: the network is not a map network (a %s; [net] yolo_output=map declares one)", what, c->cls_layer >= 0 ? "classifier" : "detector");
    return YOLO_OK;
}

// the map of the last forward's first n images as dense fp32 NHWC in d_map_f32 (room for max_batch images, twice: the planar copy of
// yolo_last_layer_output* lies behind it)
int map_to_f32(yolo_ctx *c, int n)
{
    const Layer &M = c->layers[c->map_layer];
    const size_t cap = 2 * (size_t)c->max_batch * M.H * M.W * M.C;
    if (c->map_f32_cap < cap) { HIPCK(c, hipMalloc((void **)&c->d_map_f32, cap * 4)); c->map_f32_cap = cap; }
    TView v = M.out; v.n = n;
    HIPCK(c, launch_to_f32(v, c->d_map_f32, c->stream));
    return YOLO_OK;
}

// the map as fp32 rows for the label kernels: the layer's own tensor where it is fp32 (every map a conv or deconv reaches), else the dense copy
int map_f32_view(yolo_ctx *c, int n, const float **map, int *stride)
{
    const Layer &M = c->layers[c->map_layer];
    if (M.out.dt == DT_F32) { *map = (const float *)M.out.ptr; *stride = M.out.stride; return YOLO_OK; }
    if (int r = map_to_f32(c, n)) return r;
    *map = c->d_map_f32; *stride = M.C;
    return YOLO_OK;
}

int map_labels_room(yolo_ctx *c, size_t bytes)
{
    if (bytes <= c->map_labels_cap) return YOLO_OK;
    HIPCK(c, hipStreamSynchronize(c->stream));
    if (c->d_map_labels) HIPCK(c, hipFree(c->d_map_labels));
    c->d_map_labels = nullptr; c->map_labels_cap = 0;
    HIPCK(c, hipMalloc((void **)&c->d_map_labels, bytes)); c->map_labels_cap = bytes;
    return YOLO_OK;
}

}  // namespace yolo_impl

extern "C" {

yolo_ctx *yolo_create(const yolo_config *cfg, char *err, size_t err_len)
{
    auto bail = [&](yolo_ctx *c, const std::string &m) -> yolo_ctx * { if (err && err_len) snprintf(err, err_len, "%s", m.c_str()); if (c) yolo_destroy(c); return nullptr; };
    if (!cfg || cfg->struct_size != sizeof(yolo_config)) return bail(nullptr, "yolo_create: bad yolo_config (struct_size)");
    if (cfg->max_batch < 1) return bail(nullptr, "yolo_create: max_batch < 1");
    if (cfg->dtype != YOLO_BF16 && cfg->dtype != YOLO_FP32 && cfg->dtype != YOLO_FP8 && cfg->dtype != YOLO_FP16 && cfg->dtype != YOLO_FP16X2) return bail(nullptr, "yolo_create: dtype");
    yolo_ctx *c = new yolo_ctx();
    c->device = cfg->device; c->max_batch = cfg->max_batch; c->dtype = cfg->dtype; c->semantics = cfg->semantics;
    c->decode = cfg->decode; c->keep_layers = cfg->keep_layers;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return bail(c, "yolo_create: no HIP device (this library has no CPU fallback)");
    if (hipSetDevice(c->device) != hipSuccess) return bail(c, "yolo_create: hipSetDevice failed");
    if (cfg->stream) c->stream = (hipStream_t)cfg->stream;
    else { if (hipStreamCreate(&c->stream) != hipSuccess) return bail(c, "yolo_create: hipStreamCreate failed"); c->own_stream = true; }
    std::vector<Section> secs; std::string perr;
    c->cfg_text = cfg->cfg_text ? cfg->cfg_text : "";
    if (!parse_cfg(cfg->cfg_text, secs, perr)) return bail(c, perr);
    if (build_plan(c, secs) != YOLO_OK) return bail(c, c->err);
    if (allocate(c) != YOLO_OK) return bail(c, c->err);
    resolve_scales(c);
    return c;
}

void yolo_destroy(yolo_ctx *c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (void *p : c->phys) if (p) hipFree(p);
    for (auto &L : c->layers) { if (L.d_w) hipFree(L.d_w); if (L.d_b) hipFree(L.d_b); if (L.d_sc) hipFree(L.d_sc); if (L.d_wf) hipFree(L.d_wf); if (L.d_wfrag) hipFree(L.d_wfrag); if (L.d_obj) hipFree(L.d_obj); }
    for (auto &L : c->layers) for (void *p : {L.d_w2, (void *)L.d_b2, L.d_h, L.d_hn, L.d_rh, (void *)L.d_h32, (void *)L.d_z, (void *)L.d_c}) if (p) hipFree(p);
    for (auto &L : c->layers) for (auto &S : L.sub) { if (S.d_w) hipFree(S.d_w); if (S.d_b) hipFree(S.d_b); }
    if (c->d_state_keep) hipFree(c->d_state_keep);
    for (void *p : {(void *)c->d_ring, (void *)c->d_ring_keep, (void *)c->d_ring_pos}) if (p) hipFree(p);
    void *ptrs[] = {c->input.ptr, c->d_zeros, c->d_stage, c->d_det, c->d_scores, c->d_labels, c->d_cand, c->d_keys, c->d_sbox, c->d_slabel, c->d_sscore, c->d_boxes, c->d_counts,
                    c->d_seq, c->d_dn_rec, c->d_dn_src, c->d_dn_count, c->d_dn_last, c->d_box4, c->s2d.ptr, c->d_srow, c->d_rows, c->d_lean_list, c->d_lean_cnt, c->d_f32a, c->d_f32b, c->d_descs, c->d_frames, c->d_pix, c->d_tile, c->d_views, c->d_cls_idx, c->d_cls_prob, c->d_map_f32, c->d_map_labels, c->d_label_off};
    for (void *p : ptrs) if (p) hipFree(p);
    for (auto &t : c->trees) free_tree(t);
    if (c->d_map200) hipFree(c->d_map200);
    for (void *p : {c->d_jin, (void *)c->d_jpeg, c->d_jst, (void *)c->d_jstream}) if (p) hipFree(p);
    for (void *p : {c->h_jin, c->h_jst}) if (p) hipHostFree(p);
    if (c->jpeg_up) hipEventDestroy(c->jpeg_up);
    for (hipEvent_t ev : c->jpeg_t) if (ev) hipEventDestroy(ev);
    drop_graph(c);
    if (c->own_stream && c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char *yolo_last_error(const yolo_ctx *c) { return c ? c->err.c_str() : g_op_err.c_str(); }

size_t yolo_weights_count(const yolo_ctx *c) { return c ? c->weights_count : 0; }

int yolo_input_size(const yolo_ctx *c, int *h, int *w, int *ch) { if (!c) return YOLO_ERR_INVALID; if (h) *h = c->in_h; if (w) *w = c->in_w; if (ch) *ch = c->in_c; return YOLO_OK; }
int yolo_num_rows(const yolo_ctx *c) { return c ? c->rows : YOLO_ERR_INVALID; }
int yolo_num_attrs(const yolo_ctx *c) { return c ? c->attrs : YOLO_ERR_INVALID; }
int yolo_num_classes(const yolo_ctx *c) { return !c ? YOLO_ERR_INVALID : c->cls_layer >= 0 ? c->layers[c->cls_layer].C : c->attrs - 5; }
int yolo_num_layers(const yolo_ctx *c) { return c ? (int)c->layers.size() : YOLO_ERR_INVALID; }
int yolo_head_geometry_hw(const yolo_ctx *c, int head, int *kind, int *grid_h, int *grid_w, int *anchors, int *row_offset)
{
    if (!c || head < 0) return YOLO_ERR_INVALID;
    int k = 0;
    for (auto &L : c->layers) {
        if (L.type != L_YOLO && L.type != L_REGION && L.type != L_DETECT) continue;
        if (k++ != head) continue;
        if (kind) *kind = L.type == L_REGION ? 1 : L.type == L_DETECT ? 2 : 0;
        if (grid_h) *grid_h = L.H;
        if (grid_w) *grid_w = L.W;
        if (anchors) *anchors = L.na;
        if (row_offset) *row_offset = L.row_off;
        return YOLO_OK;
    }
    return YOLO_ERR_INVALID;             // no such head
}
int yolo_head_geometry(const yolo_ctx *c, int head, int *kind, int *grid, int *anchors, int *row_offset)
{
    int gh = 0, gw = 0;
    if (int r = yolo_head_geometry_hw(c, head, kind, &gh, &gw, anchors, row_offset)) return r;
    if (gh != gw) return fail(const_cast<yolo_ctx *>(c), YOLO_ERR_UNSUPPORTED, "yolo_head_geometry: head %d has a %d x %d grid; use yolo_head_geometry_hw", head, gh, gw);
    if (grid) *grid = gh;
    return YOLO_OK;
}
double yolo_conv_flops(const yolo_ctx *c) { return c ? c->conv_flops : 0; }
double yolo_conv_bytes(const yolo_ctx *c, int n)
{
    if (!c) return 0;
    double b = 0;
    for (int i = 0; i < (int)c->layers.size(); ++i) if (c->layers[i].type == L_CONV) {
        const Layer &L = c->layers[i];
        const TView in = view_of(c, L.in[0]); const double ie = (double)dt_size(L.in_dt), oe = (double)dt_size(L.out.dt);
        if (!input_never_loaded(L, i)) b += (double)n * in.h * in.w * L.cin * ie;         // the fused stem / residual block / conv3 + stride-2 launch keep these inputs in LDS
        if (!never_stored(L, i)) b += (double)n * L.H * L.W * L.filters * oe;
        b += (double)L.filters * L.cin * L.size * L.size * ie;
    }
    return b;
}

// ---- darknet-flavoured views of the last forward (image 0), used by the veneer libdarknet_hip.so ----
int yolo_darknet_boxes(yolo_ctx *c, int w, int h, float thresh, int relative, float *records, int cap, int *count)
{
    return yolo_darknet_boxes_at(c, 0, w, h, thresh, relative, records, cap, count);
}

int yolo_darknet_boxes_at(yolo_ctx *c, int image, int w, int h, float thresh, int relative, float *records, int cap, int *count)
{
    return yolo_darknet_boxes_map(c, image, w, h, thresh, relative, nullptr, records, cap, count);
}

int yolo_darknet_boxes_map(yolo_ctx *c, int image, int w, int h, float thresh, int relative, const int32_t *map200, float *records, int cap, int *count)
{
    if (!c || !count) return YOLO_ERR_INVALID;
    if (map200) {
        // DN/region_layer.c:415-420 reads exactly 200 entries and writes prob[0 .. 200): with fewer classes the reference writes past prob[]
        if (c->tree_head < 0) return fail(c, YOLO_ERR_INVALID, "yolo_darknet_boxes_map: the network has no [region] head with a tree");
        if (c->attrs - 5 < 200) return fail(c, YOLO_ERR_INVALID, "yolo_darknet_boxes_map: a map has 200 entries and the head only %d classes", c->attrs - 5);
        for (int j = 0; j < 200; ++j) if (map200[j] < 0 || map200[j] >= c->attrs - 5) return fail(c, YOLO_ERR_INVALID, "yolo_darknet_boxes_map: map[%d] = %d is not a class", j, (int)map200[j]);
    }
    if (int r = need_detector(c, "yolo_darknet_boxes")) return r;
    if (c->last_n < 1 || !c->det_valid) return fail(c, YOLO_ERR_STATE, "yolo_darknet_boxes needs a yolo_forward* pass first");
    if (image < 0 || image >= c->last_n) return fail(c, YOLO_ERR_INVALID, "image %d outside the last forward's batch of %d", image, c->last_n);
    if (w < 1 || h < 1 || cap < 0 || (cap > 0 && !records)) return fail(c, YOLO_ERR_INVALID, "bad image size / capacity");
    HIPCK(c, hipSetDevice(c->device));
    if (!c->d_dn_rec) {
        HIPCK(c, hipMalloc((void **)&c->d_dn_rec, (size_t)c->rows * c->attrs * 4));
        HIPCK(c, hipMalloc((void **)&c->d_dn_src, (size_t)c->rows * 4));
        HIPCK(c, hipMalloc((void **)&c->d_dn_count, 4));
    }
    DnBoxesArgs a; memset(&a, 0, sizeof a);
    a.det = c->d_det + (size_t)image * c->rows * c->attrs; a.attrs = c->attrs;
    for (size_t li = 0; li < c->layers.size(); ++li) {
        const Layer &L = c->layers[li];
        if (L.type != L_YOLO && L.type != L_REGION && L.type != L_DETECT) continue;
        if (a.nheads == 8) return fail(c, YOLO_ERR_UNSUPPORTED, "more than 8 heads");
        if (L.type == L_DETECT) {
            if (a.nheads) return fail(c, YOLO_ERR_UNSUPPORTED, "a [detection] head next to other heads");
            a.raw = (const float *)c->layers[li - 1].out.ptr + (size_t)image * c->layers[li - 1].out.stride; a.side = L.side; a.classes = L.classes; a.sqr = L.sqr;
            a.kind[0] = 2; a.cells[0] = L.side * L.side; a.na[0] = L.na; a.off[0] = L.row_off; a.nheads = 1;
            continue;
        }
        if (a.raw) return fail(c, YOLO_ERR_UNSUPPORTED, "a [detection] head next to other heads");
        a.kind[a.nheads] = L.type == L_REGION; a.cells[a.nheads] = L.H * L.W; a.na[a.nheads] = L.na; a.off[a.nheads] = L.row_off; ++a.nheads;
    }
    a.thresh = thresh; a.w = w; a.h = h; a.netw = c->in_w; a.neth = c->in_h; a.relative = relative;
    a.cap = cap < c->rows ? cap : c->rows;
    a.rec = a.cap > 0 ? c->d_dn_rec : nullptr; a.src = c->d_dn_src; a.count = c->d_dn_count;
    HIPCK(c, launch_darknet_boxes(a, c->stream));
    if (c->tree_head >= 0 && a.rec) {
        // the class columns of a softmax-tree head (DN/region_layer.c:412-424), over the records just written
        if (map200) {
            if (!c->d_map200) HIPCK(c, hipMalloc((void **)&c->d_map200, 200 * 4));
            HIPCK(c, hipMemcpyAsync(c->d_map200, map200, 200 * 4, hipMemcpyHostToDevice, c->stream));
        }
        HIPCK(c, launch_darknet_tree_probs(a.det, c->attrs, c->trees[c->layers[c->tree_head].tree].dev, thresh, c->hier_thresh, map200 ? c->d_map200 : nullptr,
                                           a.rec, a.src, a.count, a.cap, c->stream));
    }
    int n = 0;
    HIPCK(c, hipMemcpyAsync(&n, c->d_dn_count, 4, hipMemcpyDeviceToHost, c->stream)); HIPCK(c, hipStreamSynchronize(c->stream));
    *count = n;
    const int got = n < a.cap ? n : a.cap;
    if (got > 0) { HIPCK(c, hipMemcpyAsync(records, c->d_dn_rec, (size_t)got * c->attrs * 4, hipMemcpyDeviceToHost, c->stream)); HIPCK(c, hipStreamSynchronize(c->stream)); }
    return YOLO_OK;
}

size_t yolo_last_layer_size(const yolo_ctx *c)
{
    if (!c) return 0;
    if (c->cls_layer >= 0) return (size_t)c->layers[c->cls_layer].C;      // the [softmax] layer's probabilities
    if (c->map_layer >= 0) { const Layer &M = c->layers[c->map_layer]; return (size_t)M.H * M.W * M.C; }      // the map, planar
    for (int i = (int)c->layers.size() - 1; i >= 0; --i) {
        const Layer &L = c->layers[i];
        if (L.type == L_DETECT) return (size_t)L.side * L.side * (L.classes + 5 * L.na);      // the layer copies its input (DN/detection_layer.c:50-57)
        if (L.type == L_YOLO || L.type == L_REGION) return (size_t)L.H * L.W * L.na * (5 + L.classes);
    }
    return 0;
}

int yolo_last_layer_output_batch(yolo_ctx *c, int n, float *out, size_t out_floats)
{
    if (!c || !out) return YOLO_ERR_INVALID;
    if (c->last_n < 1) return fail(c, YOLO_ERR_STATE, "yolo_last_layer_output before a forward pass");
    if (n < 1 || n > c->last_n) return fail(c, YOLO_ERR_INVALID, "yolo_last_layer_output of %d images but the last forward ran %d", n, c->last_n);
    if (c->cls_layer >= 0) {             // a classifier: the dense [n][classes] probabilities of its [softmax] layer
        const Layer &S = c->layers[c->cls_layer];
        if (out_floats < (size_t)n * S.C) return fail(c, YOLO_ERR_INVALID, "output buffer too small (%zu < %zu floats)", out_floats, (size_t)n * S.C);
        HIPCK(c, hipSetDevice(c->device));
        return copy_out(c, out, S.out.ptr, (size_t)n * S.C * 4, YOLO_HOST);
    }
    if (c->map_layer >= 0) {             // a map network: planar CHW per image, what darknet's net->output holds
        const Layer &M = c->layers[c->map_layer];
        const size_t per = (size_t)M.H * M.W * M.C;
        if (out_floats < per * n) return fail(c, YOLO_ERR_INVALID, "output buffer too small (%zu < %zu floats)", out_floats, per * n);
        HIPCK(c, hipSetDevice(c->device));
        if (int r = map_to_f32(c, n)) return r;
        HIPCK(c, launch_nhwc_to_chw(c->d_map_f32, c->d_map_f32 + (size_t)c->max_batch * per, n, M.H * M.W, M.C, c->stream));
        return copy_out(c, out, c->d_map_f32 + (size_t)c->max_batch * per, per * n * 4, YOLO_HOST);
    }
    const int li = output_layer(c);
    if (li < 1 || (c->layers[li].type != L_YOLO && c->layers[li].type != L_REGION && c->layers[li].type != L_DETECT))
        return fail(c, YOLO_ERR_UNSUPPORTED, "the last layer is not a detection head");
    const Layer &L = c->layers[li]; const Layer &P = c->layers[li - 1];
    const size_t per = yolo_last_layer_size(c), need = per * (size_t)n;
    if (out_floats < need) return fail(c, YOLO_ERR_INVALID, "output buffer too small (%zu < %zu floats)", out_floats, need);
    HIPCK(c, hipSetDevice(c->device));
    if (L.type == L_DETECT) {             // the prediction vectors as the fully connected layer left them (fp32, one "pixel" of P.out.stride floats per image)
        HIPCK(c, hipMemcpy2DAsync(out, per * 4, P.out.ptr, (size_t)P.out.stride * 4, per * 4, (size_t)n, hipMemcpyDeviceToHost, c->stream)); HIPCK(c, hipStreamSynchronize(c->stream));
        return YOLO_OK;
    }
    if (!c->d_dn_last || c->dn_last_cap < need) {
        if (c->d_dn_last) { HIPCK(c, hipStreamSynchronize(c->stream)); HIPCK(c, hipFree(c->d_dn_last)); c->d_dn_last = nullptr; c->dn_last_cap = 0; }
        HIPCK(c, hipMalloc((void **)&c->d_dn_last, need * 4)); c->dn_last_cap = need;
    }
    const size_t cells = (size_t)L.H * L.W;
    for (int b = 0; b < n; ++b)
        if (L.tree >= 0) HIPCK(c, launch_head_darknet_layout_tree((const float *)P.out.ptr + (size_t)b * cells * P.out.stride, P.out.stride, (int)cells, L.na, L.classes, c->trees[L.tree].dev, c->d_dn_last + (size_t)b * per, c->stream));
        else HIPCK(c, launch_head_darknet_layout((const float *)P.out.ptr + (size_t)b * cells * P.out.stride, P.out.stride, (int)cells, L.na, L.classes, L.type == L_REGION, c->d_dn_last + (size_t)b * per, c->stream));
    HIPCK(c, hipMemcpyAsync(out, c->d_dn_last, need * 4, hipMemcpyDeviceToHost, c->stream)); HIPCK(c, hipStreamSynchronize(c->stream));
    return YOLO_OK;
}

int yolo_last_layer_output(yolo_ctx *c, float *out, size_t out_floats) { return yolo_last_layer_output_batch(c, 1, out, out_floats); }

// The raw tensor a detection head decodes: the head conv's fp32 output [n, grid_h, grid_w, anchors * (5 + classes)] (what the reference's
// graph builders return before any decode: V2/model_darknet19_slim.py:198-200, V3/yolo_v3.py:239-263 `predictions`).
int yolo_head_raw(yolo_ctx *c, int head, int n, float *out, size_t out_floats)
{
    if (!c || !out || head < 0) return YOLO_ERR_INVALID;
    if (int r = need_detector(c, "yolo_head_raw")) return r;
    if (c->last_n < 1 || n < 1 || n > c->last_n) return fail(c, YOLO_ERR_STATE, "yolo_head_raw of %d images but the last forward ran %d", n, c->last_n);
    int k = 0;
    for (size_t li = 1; li < c->layers.size(); ++li) {
        const Layer &L = c->layers[li];
        if (L.type != L_YOLO && L.type != L_REGION && L.type != L_DETECT) continue;
        if (k++ != head) continue;
        const Layer &P = c->layers[li - 1];
        const size_t px = (size_t)n * P.H * P.W, need = px * P.C;
        if (out_floats < need) return fail(c, YOLO_ERR_INVALID, "output buffer too small (%zu < %zu floats)", out_floats, need);
        if (P.out.dt != DT_F32 || !P.out.ptr) return fail(c, YOLO_ERR_STATE, "internal: head conv output is not fp32");
        HIPCK(c, hipSetDevice(c->device));
        HIPCK(c, hipMemcpy2DAsync(out, (size_t)P.C * 4, P.out.ptr, (size_t)P.out.stride * 4, (size_t)P.C * 4, px, hipMemcpyDeviceToHost, c->stream));
        HIPCK(c, hipStreamSynchronize(c->stream));
        return YOLO_OK;
    }
    return fail(c, YOLO_ERR_INVALID, "no detection head %d", head);
}

// ---- map networks ([net] yolo_output=map) ----
int yolo_output_map_geometry(yolo_ctx *c, int *h, int *w, int *ch)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = need_map(c, "yolo_output_map_geometry")) return r;
    const Layer &M = c->layers[c->map_layer];
    if (h) *h = M.H; if (w) *w = M.W; if (ch) *ch = M.C;
    return YOLO_OK;
}

int yolo_output_map(yolo_ctx *c, int n, float *out, size_t out_floats)
{
    if (!c || !out) return YOLO_ERR_INVALID;
    if (int r = need_map(c, "yolo_output_map")) return r;
    if (c->last_n < 1 || n < 1 || n > c->last_n) return fail(c, YOLO_ERR_STATE, "yolo_output_map of %d images but the last forward ran %d", n, c->last_n);
    const Layer &M = c->layers[c->map_layer];
    const size_t need = (size_t)n * M.H * M.W * M.C;
    if (out_floats < need) return fail(c, YOLO_ERR_INVALID, "output buffer too small (%zu < %zu floats)", out_floats, need);
    HIPCK(c, hipSetDevice(c->device));
    if (int r = map_to_f32(c, n)) return r;
    return copy_out(c, out, c->d_map_f32, need * 4, YOLO_HOST);
}

int yolo_label_map(yolo_ctx *c, int n, float thresh, uint8_t *labels_u8)
{
    if (!c || !labels_u8) return YOLO_ERR_INVALID;
    if (int r = need_map(c, "yolo_label_map")) return r;
    if (c->last_n < 1 || n < 1 || n > c->last_n) return fail(c, YOLO_ERR_STATE, "yolo_label_map of %d images but the last forward ran %d", n, c->last_n);
    const Layer &M = c->layers[c->map_layer];
    if (M.C > 255) return fail(c, YOLO_ERR_UNSUPPORTED, "yolo_label_map: a map of %d channels (uint8 labels hold at most 255 classes; 255 itself means `below thresh`)", M.C);
    HIPCK(c, hipSetDevice(c->device));
    const size_t npix = (size_t)n * M.H * M.W;
    const float *map = nullptr; int map_stride = 0;
    if (int r = map_f32_view(c, n, &map, &map_stride)) return r;
    if (int r = map_labels_room(c, npix)) return r;
    HIPCK(c, launch_label_map(map, map_stride, npix, M.C, thresh, c->d_map_labels, c->stream));
    return copy_out(c, labels_u8, c->d_map_labels, npix, YOLO_HOST);
}

// ---- recurrent networks: the state tensors of [rnn] / [gru] / [lstm] layers, one row of `floats_per_stream` values per stream (batch index) ----
int yolo_num_state_tensors(const yolo_ctx *c) { return c ? (int)c->states.size() : YOLO_ERR_INVALID; }

// values of one stream's state tensor: the units of an [rnn] / [gru] / [lstm]; H * W * hidden_filters of a [crnn], in the tensors' own order (pixel, then channel)
static size_t state_values(const Layer &L) { return L.type == L_CRNN ? (size_t)L.H * L.W * L.cin : (size_t)L.filters; }

int yolo_state_geometry(const yolo_ctx *c, int k, int *layer, size_t *floats_per_stream)
{
    if (!c || k < 0 || k >= (int)c->states.size()) return YOLO_ERR_INVALID;
    if (layer) *layer = c->states[k].layer;
    if (floats_per_stream) *floats_per_stream = state_values(c->layers[c->states[k].layer]);
    return YOLO_OK;
}

// where state tensor k of `stream` lives: the fp32 tensor that holds it exactly (*f32: an [lstm]'s cell, a [gru]'s state) and / or its copy in the
// operand type (*op: every h)
static int state_rows(yolo_ctx *c, const char *who, int k, int stream, size_t floats, float **f32, void **op, Layer **layer)
{
    if (k < 0 || k >= (int)c->states.size()) return fail(c, YOLO_ERR_INVALID, "%s: state tensor %d outside 0..%d", who, k, (int)c->states.size() - 1);
    if (stream < 0 || stream >= c->max_batch) return fail(c, YOLO_ERR_INVALID, "%s: stream %d outside 0..%d", who, stream, c->max_batch - 1);
    Layer &L = c->layers[c->states[k].layer];
    if (floats != state_values(L)) return fail(c, YOLO_ERR_INVALID, "%s: state tensor %d holds %zu floats per stream, not %zu", who, k, state_values(L), floats);
    const size_t row = (size_t)stream * state_elems(c, L);
    *f32 = L.type == L_CRNN ? nullptr : c->states[k].cell ? L.d_c + row : L.rkind == RECUR_GRU ? L.d_h32 + row : nullptr;
    *op = c->states[k].cell ? nullptr : (char *)L.d_h + row * dt_size(L.in_dt);
    *layer = &L;
    return YOLO_OK;
}

int yolo_get_state(yolo_ctx *c, int k, int stream, float *out, size_t out_floats)
{
    if (!c || !out) return YOLO_ERR_INVALID;
    float *f32; void *op; Layer *L;
    if (int r = state_rows(c, "yolo_get_state", k, stream, out_floats, &f32, &op, &L)) return r;
    HIPCK(c, hipSetDevice(c->device)); HIPCK(c, hipStreamSynchronize(c->stream));
    // (a [crnn]'s map: `width` channels per pixel out of a pitch of whole granules; the other states: one row)
    const size_t es = dt_size(L->in_dt), width = L->type == L_CRNN ? (size_t)L->cin : out_floats, pitch = L->type == L_CRNN ? (size_t)roundup(L->cin, 8) : out_floats, rows = out_floats / width;
    if (f32 || L->in_dt == DT_F32) { HIPCK(c, hipMemcpy2D(out, width * 4, f32 ? (void *)f32 : op, pitch * 4, width * 4, rows, hipMemcpyDeviceToHost)); return YOLO_OK; }
    std::vector<uint16_t> raw(out_floats);
    HIPCK(c, hipMemcpy2D(raw.data(), width * es, op, pitch * es, width * es, rows, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < out_floats; ++j) { if (L->in_dt == DT_F16) out[j] = h2f(raw[j]); else { const uint32_t u = (uint32_t)raw[j] << 16; memcpy(&out[j], &u, 4); } }
    return YOLO_OK;
}

int yolo_set_state(yolo_ctx *c, int k, int stream, const float *in, size_t in_floats)
{
    if (!c || !in) return YOLO_ERR_INVALID;
    float *f32; void *op; Layer *L;
    if (int r = state_rows(c, "yolo_set_state", k, stream, in_floats, &f32, &op, &L)) return r;
    HIPCK(c, hipSetDevice(c->device)); HIPCK(c, hipStreamSynchronize(c->stream));
    if (f32) HIPCK(c, hipMemcpy(f32, in, in_floats * 4, hipMemcpyHostToDevice));
    if (!op) return YOLO_OK;
    const size_t es = dt_size(L->in_dt), width = L->type == L_CRNN ? (size_t)L->cin : in_floats, pitch = L->type == L_CRNN ? (size_t)roundup(L->cin, 8) : in_floats, rows = in_floats / width;
    if (L->in_dt == DT_F32) { HIPCK(c, hipMemcpy2D(op, pitch * 4, in, width * 4, width * 4, rows, hipMemcpyHostToDevice)); return YOLO_OK; }
    std::vector<uint16_t> raw(in_floats);          // rounded as the kernels round what they store
    for (size_t j = 0; j < in_floats; ++j) raw[j] = L->in_dt == DT_F16 ? f2h(in[j]) : f2bf(in[j]);
    HIPCK(c, hipMemcpy2D(op, pitch * es, raw.data(), width * es, width * es, rows, hipMemcpyHostToDevice));
    return YOLO_OK;
}

// the frame-average ring of one stream (or of all, stream < 0) back to empty: K slots of zeros, position 0
static int ring_clear(yolo_ctx *c, int stream)
{
    const size_t E = c->ring_elems(), slot = (size_t)c->max_batch * E;
    if (stream < 0) HIPCK(c, hipMemsetAsync(c->d_ring, 0, slot * c->avg_k * 4, c->stream));
    else for (int j = 0; j < c->avg_k; ++j) HIPCK(c, hipMemsetAsync(c->d_ring + j * slot + (size_t)stream * E, 0, E * 4, c->stream));
    HIPCK(c, hipMemsetAsync(c->d_ring_pos + (stream < 0 ? 0 : stream), 0, (size_t)(stream < 0 ? c->max_batch : 1) * 4, c->stream));
    return YOLO_OK;
}

// reset_network_state(net, b) (DN/network.c:69): the states of one stream, or of all (stream < 0), back to zero
int yolo_reset_state(yolo_ctx *c, int stream)
{
    if (!c) return YOLO_ERR_INVALID;
    if (stream >= c->max_batch) return fail(c, YOLO_ERR_INVALID, "yolo_reset_state: stream %d outside 0..%d (-1: all)", stream, c->max_batch - 1);
    HIPCK(c, hipSetDevice(c->device));
    for (Layer &L : c->layers) {
        if (!has_state(L)) continue;
        const size_t ss = state_elems(c, L), first = stream < 0 ? 0 : (size_t)stream * ss, ne = stream < 0 ? (size_t)c->max_batch * ss : ss, es = dt_size(L.in_dt);
        HIPCK(c, hipMemsetAsync((char *)L.d_h + first * es, 0, ne * es, c->stream));
        for (float *p : {L.d_h32, L.d_c}) if (p) HIPCK(c, hipMemsetAsync(p + first, 0, ne * 4, c->stream));
    }
    if (c->avg_k > 1) if (int r = ring_clear(c, stream)) return r;      // a new video on the stream starts with empty slots, as demo()'s calloc leaves them
    return YOLO_OK;
}

// ---- frame averaging ("Frame averaging"; DN/examples/demo.c) ----
int yolo_frame_average(const yolo_ctx *c) { return c ? c->avg_k : YOLO_ERR_INVALID; }

int yolo_set_frame_average(yolo_ctx *c, int frames)
{
    static const char *const who = "yolo_set_frame_average";
    if (!c) return YOLO_ERR_INVALID;
    if (frames < 1 || frames > 8) return fail(c, YOLO_ERR_INVALID, "%s: %d frames outside 1..8 (1: off)", who, frames);
    if (frames > 1) {
        if (int r = need_detector(c, who)) return r;
        for (size_t i = 0; i < c->layers.size(); ++i) {
            const Layer &L = c->layers[i];
            if (L.type == L_DETECT) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: layer %d is a [detection] (YOLOv1) head: its output is not averaged (darknet's demo averages it, its boxes take the square of the mean; not served)", who, (int)i);
            if (is_head_layer(L) && L.tree >= 0) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: layer %d is a [region] head with a softmax tree: the mean of per-group softmaxes is not served", who, (int)i);
            if (is_head_layer(L) && 5 + L.classes > 128) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: layer %d has %d attributes per box (at most 128)", who, (int)i, 5 + L.classes);
        }
    }
    HIPCK(c, hipSetDevice(c->device));
    if (frames == c->avg_k && frames == 1) return YOLO_OK;
    // another launch sequence, other buffers: no captured step may be replayed; nothing in flight may still read the old ring
    drop_graph(c);
    HIPCK(c, hipStreamSynchronize(c->stream));
    for (void **p : {(void **)&c->d_ring, (void **)&c->d_ring_keep, (void **)&c->d_ring_pos}) { if (*p) HIPCK(c, hipFree(*p)); *p = nullptr; }
    c->avg_k = 1; c->ring_frozen = false;
    if (frames == 1) return YOLO_OK;
    const size_t slot = (size_t)c->max_batch * c->ring_elems() * 4;
    if (hipMalloc((void **)&c->d_ring, slot * frames) != hipSuccess || hipMalloc((void **)&c->d_ring_keep, slot) != hipSuccess || hipMalloc((void **)&c->d_ring_pos, (size_t)c->max_batch * 4) != hipSuccess) {
        (void)hipGetLastError();
        for (void **p : {(void **)&c->d_ring, (void **)&c->d_ring_keep, (void **)&c->d_ring_pos}) { if (*p) hipFree(*p); *p = nullptr; }
        return fail(c, YOLO_ERR_HIP, "%s: no memory for %d + 1 slots of %zu bytes", who, frames, slot);
    }
    c->avg_k = frames;
    return ring_clear(c, -1);
}

int yolo_synchronize(yolo_ctx *c) { if (!c) return YOLO_ERR_INVALID; HIPCK(c, hipStreamSynchronize(c->stream)); return YOLO_OK; }

int yolo_layer_output(yolo_ctx *c, int index, int n, float *out, size_t out_floats, int *dims_out)
{
    if (!c) return YOLO_ERR_INVALID;
    if (index < 0 || index >= (int)c->layers.size() || n < 1 || n > c->last_n) return fail(c, YOLO_ERR_INVALID, "bad layer index / n");
    const Layer &L = c->layers[index];
    if (!c->keep_layers) {
        // the production plan pools its buffers and keeps fused-away tensors in LDS: only a conv that launches, writes its own tensor and
        // whose buffer no later tensor takes over still holds its output after the forward
        bool kept = L.type == L_CONV && L.storage >= 0 && L.residual_from < -1 && !never_stored(L, index);
        if (kept) for (const Storage &o : c->storages) if (&o != &c->storages[L.storage] && o.phys == c->storages[L.storage].phys && o.def > c->storages[L.storage].def) kept = false;
        if (!kept) return fail(c, YOLO_ERR_STATE, "yolo_layer_output needs keep_layers=1 (without it: only a conv layer's own tensor whose buffer no later layer reuses)");
    }
    if (dims_out) { dims_out[0] = L.H; dims_out[1] = L.W; dims_out[2] = L.C; }
    size_t need = (size_t)n * L.H * L.W * L.C;
    if (!out) return YOLO_OK;
    if (out_floats < need) return fail(c, YOLO_ERR_INVALID, "output buffer too small");
    HIPCK(c, hipSetDevice(c->device));
    float *tmp = nullptr; HIPCK(c, hipMalloc((void **)&tmp, need * 4));
    TView v = L.out; v.n = n;
    float vs = 1.f;
    if (v.dt == DT_FP8) {
        vs = c->eff_scale[index];
        if (vs != vs) { hipFree(tmp); return fail(c, YOLO_ERR_UNSUPPORTED, "layer %d concatenates tensors with different fp8 scales; read its sources", index); }
    }
    hipError_t e = hipSuccess;
    float *wide = nullptr;
    if (L.pair && v.dt == DT_F16) {        // split pairs: join into a Cp-strided fp32 image first, then gather the C logical channels
        const int cp = roundup(L.C, 32);
        e = hipMalloc((void **)&wide, (size_t)n * L.H * L.W * cp * 4);
        if (e == hipSuccess) e = launch_split_to_f32(v.ptr, v.stride, cp, wide, cp, (size_t)n * L.H * L.W, c->stream);
        v.ptr = wide; v.stride = cp; v.dt = DT_F32;
    }
    if (e == hipSuccess) e = launch_to_f32(v, tmp, c->stream, vs);
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, need * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(tmp); if (wide) hipFree(wide);
    if (e != hipSuccess) return fail(c, YOLO_ERR_HIP, "layer_output: %s", hipGetErrorString(e));
    return YOLO_OK;
}

// the staged network input of the last forward as fp32, every stored channel of a pixel: dims_out = {h, w, stored channels}, 8 for an RGB image (3 real + 5 zero),
// roundup(N, 8) for N planes.  Introspection, like yolo_layer_output: a copy through a temporary buffer
int yolo_staged_input(yolo_ctx *c, int n, float *out, size_t out_floats, int *dims_out)
{
    if (!c) return YOLO_ERR_INVALID;
    if (c->vec_n || c->in_pair) return fail(c, YOLO_ERR_UNSUPPORTED, "yolo_staged_input: a vector-input network's row and a split-fp16 image stored as pairs are not served");
    if (c->stem_u8) return fail(c, YOLO_ERR_STATE, "yolo_staged_input: the last forward's uint8 images were read by the fused first-stage kernel itself, nothing was staged");
    if (n < 1 || n > c->last_n) return fail(c, YOLO_ERR_INVALID, "bad n");
    TView v = c->input; v.n = n; v.c = v.stride;
    if (dims_out) { dims_out[0] = v.h; dims_out[1] = v.w; dims_out[2] = v.c; }
    const size_t need = (size_t)n * v.h * v.w * v.c;
    if (!out) return YOLO_OK;
    if (out_floats < need) return fail(c, YOLO_ERR_INVALID, "output buffer too small");
    HIPCK(c, hipSetDevice(c->device));
    float *tmp = nullptr; HIPCK(c, hipMalloc((void **)&tmp, need * 4));
    hipError_t e = launch_to_f32(v, tmp, c->stream, 1.f);
    if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, need * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(tmp);
    if (e != hipSuccess) return fail(c, YOLO_ERR_HIP, "staged_input: %s", hipGetErrorString(e));
    return YOLO_OK;
}

}  // extern "C"
