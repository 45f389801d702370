// Launch sequence of libyolo_hip.so: layer -> kernel launch, input staging, threshold + NMS, the captured detect steps and layer timing.
#include "yolo_ctx.h"
#include <chrono>

namespace yolo_impl {

int fail(yolo_ctx *c, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    if (c) c->err = buf;
    return code;
}

ConvArgs conv_args(const yolo_ctx *c, const Layer &L, int n)
{
    ConvArgs a; memset(&a, 0, sizeof a);
    TView in = view_of(c, L.in[0]);
    a.in = in.ptr; a.in_stride = in.stride; a.wt = L.d_w; a.bias = L.d_b;
    a.out = L.out.ptr; a.out_stride = L.out.stride; a.out_dt = L.out.dt; a.in_dt = L.in_dt; a.oscale = L.d_sc;
    // split fp16: a conv that writes PAIRS leaves through the SPLIT epilogue (interleaved hi | lo groups); the fp32 heads of such a network keep
    // running on the split instantiations too (their tile table); a conv that writes plain fp16 (mixed plans) has the ordinary fp16 epilogue
    if (L.pair || (c->split() && L.out.dt == DT_F32)) a.split = 1;
    a.pairk = L.in[0] >= 0 && c->pair_of(L.in[0]) ? 1 : 0;          // the input is an interleaved pair tensor: the pair K loop (the network input's three blocks: the plain one)
    a.out_inv_scale = 1.f; a.res_scale = 1.f; a.mid_scale = 1.f; a.mid_inv_scale = 1.f;
    if (c->fragw) a.wf = L.d_wfrag;          // (null for every conv but those filter_fragments serves)
    const int li = (int)(&L - c->layers.data());
    if (L.residual_from >= -1) { TView r = view_of(c, L.residual_from); a.res = r.ptr; a.res_stride = r.stride; }
    // the tail runs on the producer's operand type: bf16 needs the fragment-order copy of the 1x1 filters (tail_fragments), e4m3 an
    // e4m3-packed 1x1 conv; anything else leaves w2 null and run_layer refuses the plan instead of launching with a null w2f
    if (L.tail_on && L.tail_layer >= 0 && c->layers[L.tail_layer].in_dt == L.in_dt && (L.in_dt == DT_FP8 || c->layers[L.tail_layer].d_wf)) {
        const Layer &T = c->layers[L.tail_layer];
        a.w2 = T.d_w; a.w2f = T.d_wf; a.b2 = T.d_b; a.out2 = T.out.ptr; a.out2_stride = T.out.stride; a.K2pad = T.kpad; a.act2 = T.act;
        a.oscale2 = T.d_sc; a.out2_inv_scale = T.out.dt == DT_FP8 ? 1.f / c->eff_scale[L.tail_layer] : 1.f;
        if (T.head) {            // the tail is a detection head: fp32 rows + the objectness plane of the [yolo] layer behind it
            a.tail_f32 = 1; a.C2out = T.filters;
            if (T.d_obj && L.tail_layer + 1 < (int)c->layers.size()) { const Layer &Y = c->layers[L.tail_layer + 1]; a.obj_out = T.d_obj; a.obj_attrs = 5 + Y.classes; a.obj_na = Y.na; conv_magic((uint32_t)a.obj_attrs, a.obj_mul, a.obj_shift); }
        }
    }
    if (L.out.dt == DT_FP8) {
        if (L.residual_from >= -1) {     // fused shortcut: this conv writes layer li+1's tensor
            a.mid_scale = c->user_scale[li]; a.mid_inv_scale = 1.f / c->user_scale[li];
            a.res_scale = c->eff_scale[L.residual_from]; a.out_inv_scale = 1.f / c->eff_scale[li + 1];
        } else a.out_inv_scale = 1.f / c->eff_scale[li];
    }
    a.N = n; a.H = in.h; a.W = in.w; a.Cin_pad = L.cin_pad; a.Ho = L.H; a.Wo = L.W; a.Cout = L.filters;
    a.ksize = L.size; a.stride = L.stride; a.pad = L.pad; a.Kpad = L.kpad; a.kchunk = conv_kchunk(L.cin_pad, L.in_dt); a.act = L.act; a.zeros = c->d_zeros;
    if (L.d_obj && li + 1 < (int)c->layers.size()) { const Layer &Y = c->layers[li + 1]; a.obj_out = L.d_obj; a.obj_attrs = 5 + Y.classes; a.obj_na = Y.na; conv_magic((uint32_t)a.obj_attrs, a.obj_mul, a.obj_shift); }
    if (L.fc) { a.H = a.W = 1; a.in_stride = L.fc_h * L.fc_w * in.stride; }         // one "pixel" per image: the flattened producer
    if (L.s2d7) { a.in = c->s2d.ptr; a.in_stride = 32; a.H = c->s2d.h; a.W = c->s2d.w; a.ksize = 4; a.stride = 1; a.pad = 2; }   // see pack_s2d7
    conv_finalize(a);
    return a;
}

DeconvArgs deconv_geometry(int size, int stride, int pad, int h, int w, int cin_pad, int filters, int act, int in_dt)
{
    DeconvArgs a; memset(&a, 0, sizeof a);
    a.size = size; a.stride = stride; a.pad = pad; a.H = h; a.W = w; a.Cin_pad = cin_pad; a.Cout = filters; a.act = act; a.in_dt = in_dt;
    a.Ho = (h - 1) * stride + size - 2 * pad; a.Wo = (w - 1) * stride + size - 2 * pad;
    a.cout_pad = roundup(filters, DECONV_CO_TILE);
    deconv_layout(a);
    return a;
}

static TView nview(int n, TView v) { v.n = n; return v; }      // a tensor's view at this call's batch
// channels a layer that computes `ch` of them stores: zeros in the channels past them, up to the granule of the output's type (a window of a concat buffer holds whole granules)
static int store_width(const Layer &L, int ch) { return std::min(L.out.stride, roundup(ch, L.out.dt == DT_F32 && L.head ? 4 : 8)); }

// the fields of a side conv's arguments its geometry leaves open: tensors, parameters, batch, the stored width
static void side_bind(SideConvArgs &a, const yolo_ctx *c, const Layer &L, int n)
{
    const TView in = view_of(c, L.in[0]);
    a.in = in.ptr; a.in_stride = in.stride; a.wt = L.d_w; a.bias = L.d_b; a.out = L.out.ptr; a.out_stride = L.out.stride; a.out_dt = L.out.dt; a.N = n;
    a.Cstore = store_width(L, L.filters);
}

static DeconvArgs deconv_args(const yolo_ctx *c, const Layer &L, int n)
{
    const TView in = view_of(c, L.in[0]);
    DeconvArgs a = deconv_geometry(L.size, L.stride, L.pad, in.h, in.w, L.cin_pad, L.filters, L.act, L.in_dt);
    side_bind(a, c, L, n);
    return a;
}

GConvArgs gconv_geometry(int size, int stride, int pad, int h, int w, int cin, int filters, int groups, int act, int in_dt)
{
    GConvArgs a; memset(&a, 0, sizeof a);
    a.size = size; a.stride = stride; a.pad = pad; a.H = h; a.W = w; a.C = cin; a.Cout = filters; a.groups = groups; a.act = act; a.in_dt = in_dt;
    a.Ho = (h + 2 * pad - size) / stride + 1; a.Wo = (w + 2 * pad - size) / stride + 1;
    gconv_layout(a);
    return a;
}

static GConvArgs gconv_args(const yolo_ctx *c, const Layer &L, int n)
{
    const TView in = view_of(c, L.in[0]);
    GConvArgs a = gconv_geometry(L.size, L.stride, L.pad, in.h, in.w, L.cin, L.filters, L.groups, L.act, L.in_dt);
    side_bind(a, c, L, n);
    return a;
}

XConvArgs xconv_geometry(int size, int stride, int pad, int h, int w, int cin, int filters, int act)
{
    XConvArgs a; memset(&a, 0, sizeof a);
    a.size = size; a.stride = stride; a.pad = pad; a.H = h; a.W = w; a.C = cin; a.Cout = filters; a.act = act;
    a.Ho = (h + 2 * pad - size) / stride + 1; a.Wo = (w + 2 * pad - size) / stride + 1;
    xconv_layout(a);
    return a;
}

// (the input is read in the type its producer stored it in -- an fp32 tensor of a 16-bit network included: the sign needs no conversion)
static XConvArgs xconv_args(const yolo_ctx *c, const Layer &L, int n)
{
    const TView in = view_of(c, L.in[0]);
    XConvArgs a = xconv_geometry(L.size, L.stride, L.pad, in.h, in.w, L.cin, L.filters, L.act);
    side_bind(a, c, L, n);
    a.in_dt = in.dt; a.scale = L.d_sc;
    return a;
}

static hipError_t launch_side_conv(const yolo_ctx *c, const Layer &L, int n, hipStream_t s)
{
    if (L.type == L_DECONV) return launch_deconv(deconv_args(c, L, n), s);
    if (L.type == L_GCONV) return launch_gconv(gconv_args(c, L, n), s);
    return launch_xconv(xconv_args(c, L, n), s);
}

void side_layout(const Layer &L, int &kpad, int &cout_pad)
{
    if (L.type == L_DECONV) {          // (the K of all phases together)
        const DeconvArgs g = deconv_geometry(L.size, L.stride, L.pad, 1, 1, L.cin_pad, L.filters, ACT_LINEAR, L.in_dt);
        cout_pad = g.cout_pad; kpad = 0;
        for (int p = 0; p < L.stride * L.stride; ++p) kpad += g.kp[p];
    } else if (L.type == L_GCONV) {
        const GConvArgs g = gconv_geometry(L.size, L.stride, L.pad, 1, 1, L.cin, L.filters, L.groups, ACT_LINEAR, L.in_dt);
        kpad = g.kp; cout_pad = g.nb * g.mb;
    } else {
        const XConvArgs g = xconv_geometry(L.size, L.stride, L.pad, 1, 1, L.cin, L.filters, ACT_LINEAR);
        kpad = g.kpad; cout_pad = g.cout_pad;          // (bytes: int8 filters)
    }
}

// split fp16: a layer that moves or interpolates values runs in fp32 between a join (hi + lo) and a split
static int via_f32(yolo_ctx *c, const Layer &L, int n)
{
    hipStream_t s = c->stream;
    const TView in = view_of(c, L.in[0]);
    const int cpi = roundup(in.c, 32), cpo = roundup(L.C, 32);
    const size_t pin = (size_t)n * in.h * in.w, pout = (size_t)n * L.H * L.W;
    if (pin * cpi > c->f32_cap || pout * cpo > c->f32_cap) return fail(c, YOLO_ERR_STATE, "internal: fp32 staging too small");
    HIPCK(c, launch_split_to_f32(in.ptr, in.stride, cpi, c->d_f32a, cpi, pin, s));
    TView a; a.ptr = c->d_f32a; a.n = n; a.h = in.h; a.w = in.w; a.c = cpi; a.stride = cpi; a.dt = DT_F32;
    TView b; b.ptr = c->d_f32b; b.n = n; b.h = L.H; b.w = L.W; b.c = cpo; b.stride = cpo; b.dt = DT_F32;
    switch (L.type) {
    case L_UPSAMPLE: HIPCK(c, launch_upsample2x(a, b, c->semantics == YOLO_SEM_TF, s)); break;
    case L_MAXPOOL: HIPCK(c, launch_maxpool(a, b, L.psize, L.pstride, L.ppad, s)); break;
    default:          // L_REORG.  It scrambles channels: it runs on the LOGICAL channel counts (the padding of a pair tensor is not part of it)
        a.c = in.c; b.c = L.C;
        if (in.c % 32 || L.C % 32) return fail(c, YOLO_ERR_STATE, "internal: reorg of a pair tensor of %d channels (the planner refuses all but whole 32-channel groups)", in.c);
        HIPCK(c, launch_reorg(a, b, L.pstride, c->semantics == YOLO_SEM_DARKNET, s));
    }
    HIPCK(c, launch_split_from_f32(c->d_f32b, cpo, L.out.ptr, L.out.stride, cpo, pout, s));
    return YOLO_OK;
}

// ---- one builder per argument struct of the fused / fixed launches, each called once per launch.  `l`: the group's launcher ----
static StemPairArgs stem_pair_args(const yolo_ctx *c, int l, int n)          // split-fp16: conv0 + conv1 in one launch (conv_stem_pair.hip)
{
    const Layer &A = c->layers[0], &L = c->layers[l]; StemPairArgs t; memset(&t, 0, sizeof t);
    t.in = c->input.ptr; t.w0 = A.d_w; t.b0 = A.d_b; t.Kpad0 = A.kpad; t.C0 = A.filters; t.act0 = A.act;
    t.in_u8 = c->stem_u8; t.in_scale = c->stem_scale; t.in_mul = c->in_mul; t.in_add = c->in_add;
    t.w1 = L.d_w; t.b1 = L.d_b; t.Kpad1 = L.kpad; t.act1 = L.act;
    t.out = L.out.ptr; t.out_stride = L.out.stride; t.N = n; t.H = A.H; t.W = A.W; t.Ho = L.H; t.Wo = L.W;
    return t;
}
static StemArgs stem_args(const yolo_ctx *c, int l, int n)
{
    const Layer &A = c->layers[0], &L = c->layers[l]; StemArgs t; memset(&t, 0, sizeof t);
    t.in = c->input.ptr; t.in_stride = c->input.stride;
    t.in_u8 = c->stem_u8; t.in_scale = c->stem_scale; t.in_mul = c->in_mul; t.in_add = c->in_add;
    t.w0 = A.d_w; t.b0 = A.d_b; t.Kpad0 = A.kpad; t.C0 = A.filters; t.act0 = A.act;
    t.w1 = L.d_w; t.b1 = L.d_b; t.Kpad1 = L.kpad; t.C1 = L.filters; t.act1 = L.act;
    if (l + 1 < (int)c->layers.size() && c->layers[l + 1].fused == L.fused) { const Layer &T = c->layers[l + 1];          // the group's third member: the 1x1 conv behind conv1
        t.w2 = T.d_w; t.b2 = T.d_b; t.Kpad2 = T.kpad; t.C2 = T.filters; t.act2 = T.act; t.out2 = T.out.ptr; t.out2_stride = T.out.stride;
    }
    t.out = L.out.ptr; t.out_stride = L.out.stride; t.N = n; t.H = A.H; t.W = A.W; t.Ho = L.H; t.Wo = L.W; t.zeros = c->d_zeros; t.dt = L.in_dt;
    return t;
}
static BlockArgs block_args(const yolo_ctx *c, int l, int n)          // fused residual block: the 1x1 (A) is computed inside the 3x3's (B) launch
{
    const Layer &A = c->layers[l - 1], &B = c->layers[l]; const TView x = view_of(c, A.in[0]); BlockArgs b; memset(&b, 0, sizeof b);
    b.x = x.ptr; b.x_stride = x.stride; b.w1 = A.d_w; b.b1 = A.d_b; b.Kpad1 = A.kpad; b.act1 = A.act;
    b.w2 = B.d_w; b.b2 = B.d_b; b.Kpad2 = B.kpad; b.act2 = B.act; b.out = B.out.ptr; b.out_stride = B.out.stride;
    b.N = n; b.H = B.H; b.W = B.W; b.C = B.filters; b.Cmid = A.filters; b.dt = B.in_dt;
    return b;
}
static C3S2Args c3s2_args(const yolo_ctx *c, int l, int n)          // conv3 + shortcut (A) are computed inside the stride-2 conv's (B) launch
{
    const Layer &A = c->layers[l - 2], &B = c->layers[l]; const TView x = view_of(c, A.in[0]), r = view_of(c, A.residual_from); C3S2Args t; memset(&t, 0, sizeof t);
    t.in = x.ptr; t.in_stride = x.stride; t.w3 = A.d_w; t.b3 = A.d_b; t.Kpad3 = A.kpad; t.act3 = A.act; t.res = r.ptr; t.res_stride = r.stride;
    t.w5 = B.d_w; t.b5 = B.d_b; t.Kpad5 = B.kpad; t.act5 = B.act; t.out = B.out.ptr; t.out_stride = B.out.stride;
    t.N = n; t.H = A.H; t.W = A.W; t.dt = B.in_dt;
    return t;
}
static HaloArgs halo_args(const ConvArgs &a, const Layer &L, int n)      // for conv_halo_c32_c64 and conv_s2_c64_c128.  H, W: the input's, which are the output's of the 3x3/s1/pad-1 halo conv; res / res_stride: 0 for K_S2 (it folds no shortcut)
{
    HaloArgs h; memset(&h, 0, sizeof h);
    h.in = a.in; h.in_stride = a.in_stride; h.w = a.wt; h.b = a.bias; h.Kpad = a.Kpad; h.Cin = L.cin; h.Cout = L.filters; h.act = L.act;
    h.res = a.res; h.res_stride = a.res_stride; h.out = a.out; h.out_stride = a.out_stride; h.N = n; h.H = a.H; h.W = a.W; h.dt = L.in_dt;
    return h;
}

static bool fused_launch_applies(yolo_ctx *c, const Layer &L, int n)      // at batch n (no group: no)?  A group that may fall back asks its kernel once per batch size and keeps the answer on its launcher: every member takes the same branch
{
    if (!fused_may_fall_back(L)) return L.fused != F_NONE;
    Layer &G = c->layers[L.launcher]; const int l = L.launcher;
    if (G.fuse_n != n) { G.fuse_ok = L.fused == F_RESBLOCK ? conv_resblock_ok(block_args(c, l, n)) : conv_c3s2_ok(c3s2_args(c, l, n)); G.fuse_n = n; }
    return G.fuse_ok;
}

static int run_conv(yolo_ctx *c, int i, int n)
{
    Layer &L = c->layers[i];
    hipStream_t s = c->stream;
    if (fused_launch_applies(c, L, n)) {          // computed inside its group's launch, which the launcher issues
        if (i == L.launcher) switch (L.fused) {
        case F_STEM: { StemArgs t = stem_args(c, i, n); HIPCK(c, launch_conv_stem(t, s)); break; }
        case F_PSTEM: { StemPairArgs t = stem_pair_args(c, i, n); if (c->input.stride != 24 || !conv_stem_pair_ok(t)) return fail(c, YOLO_ERR_STATE, "layer %d: the fused split-fp16 stem does not apply to this plan", i);
            HIPCK(c, launch_conv_stem_pair(t, s)); break; }
        case F_RESBLOCK: { BlockArgs b = block_args(c, i, n); HIPCK(c, launch_conv_resblock(b, s)); break; }
        case F_C3S2: { C3S2Args t = c3s2_args(c, i, n); HIPCK(c, launch_conv_c3s2(t, s)); break; }
        }
        return YOLO_OK;
    }
    if (rides_as_tail(c, L)) return YOLO_OK;        // computed in the producer's epilogue
    ConvArgs a = conv_args(c, L, n);
    if (L.tail_on && !a.w2) return fail(c, YOLO_ERR_STATE, "layer %d: the plan folds the 1x1 conv %d into this layer, but its filters are not available in the producer's operand type", i, L.tail_layer);
    if (L.s2d7) HIPCK(c, launch_reorg(nview(n, c->input), nview(n, c->s2d), 2, 0, s));      // tf.space_to_depth order: (dy, dx, channel)
    if (L.kernel != K_TILED) {          // input tile (K_HALO, conv_stem.hip) / window (K_S2, conv_s2.hip) staged once in LDS; a window over 2 GiB (very large batches): the tiled kernel below checks its own
        HaloArgs h = halo_args(a, L, n);
        if (L.kernel == K_HALO && conv_halo_ok(h)) { HIPCK(c, launch_conv_halo(h, s)); return YOLO_OK; }
        if (L.kernel == K_S2 && conv_s2_ok(h)) { HIPCK(c, launch_conv_s2(h, s)); return YOLO_OK; }
    }
    if (c->dtype == YOLO_FP32) { HIPCK(c, launch_conv_f32(a, s)); return YOLO_OK; }
    const int cfg = conv_resolve_cfg(a, L.tile_cfg);
    if (a.w2 && !a.split && !a.pairk && !conv_cfg_tail_ok(cfg, a.Cout, a.in_dt == DT_FP8, a.tail_f32 != 0)) return fail(c, YOLO_ERR_STATE, "layer %d: tile config %d cannot run the fused 1x1 tail", i, cfg);
    HIPCK(c, a.in_dt == DT_FP8 ? launch_conv_fp8(a, cfg, s) : launch_conv_bf16(a, cfg, s));
    return YOLO_OK;
}

// [rnn] / [gru] / [lstm]: one time step of streams 0 .. n - 1 in the layer's one or two launches (RecurArgs, kernels.h; recur_geom), then the copy that
// makes the new state the state.  Streams n .. max_batch - 1 are not touched
static int run_recurrent(yolo_ctx *c, int i, int n)
{
    const Layer &L = c->layers[i]; hipStream_t s = c->stream;
    const RecurGeom g = recur_geom(c, L); const TView in = view_of(c, L.in[0]);
    RecurArgs a; memset(&a, 0, sizeof a);
    a.dt = L.in_dt; a.units = L.filters; a.n = n; a.act = L.act; a.shortcut = L.rshortcut; a.tanh_ = L.rtanh;
    a.s_stride = g.s_stride; a.c = L.d_c; a.h32 = L.d_h32; a.z = L.d_z; a.rh = L.d_rh; a.h_new = L.d_hn; a.hs = L.d_h;
    a.out = L.out.ptr; a.out_stride = L.out.stride; a.out_dt = L.out.dt;
    a.mode = g.mode[0]; a.w = L.d_w; a.bx = L.d_b; a.bh = L.d_b + g.Mp[0];
    a.x = in.ptr; a.x_stride = g.x_len; a.x_len = g.x_len; a.Kx = g.Kx[0];          // the flattened producer: one "pixel" of fc_h * fc_w * stride elements per stream
    a.h = L.d_h; a.h_stride = g.s_stride; a.h_len = g.s_stride; a.Kh = g.Kh[0];
    HIPCK(c, launch_recur(a, s));
    if (g.launches == 2) {
        a.mode = g.mode[1]; a.w = L.d_w2; a.bx = L.d_b2; a.bh = L.d_b2 + g.Mp[1]; a.Kx = g.Kx[1]; a.Kh = g.Kh[1];
        if (L.rkind == RECUR_RNN) { a.x = L.d_hn; a.x_stride = a.x_len = g.s_stride; a.h = nullptr; a.h_stride = a.h_len = 0; }      // the output sublayer over the new state
        else a.h = L.d_rh;                                                                                                          // [x | r * h]
        HIPCK(c, launch_recur(a, s));
    }
    // every launch that reads the old state as an operand has been issued: the new one takes its place.  A copy, not a swap of pointers: a
    // captured step holds both
    if (L.d_hn) HIPCK(c, hipMemcpyAsync(L.d_h, L.d_hn, (size_t)n * g.s_stride * dt_size(L.in_dt), hipMemcpyDeviceToDevice, s));
    return YOLO_OK;
}

// [crnn]: its three convs through the dense conv kernels' own selection rule; the epilogue's residual sums the state (run after the activation, as a
// folded [shortcut] is) where the activation is of the slope family, else k_activate and an add launch behind the conv do.  in -> d_rh = [state +] act(conv_in(x)); state -> d_hn = d_rh + act(conv_self(state)); d_hn -> out = act(conv_out(state')); then the
// copy that makes the new state the state: both reads of the old one have been issued by then
static int run_crnn(yolo_ctx *c, int i, int n)
{
    const Layer &L = c->layers[i]; hipStream_t s = c->stream;
    const TView in = view_of(c, L.in[0]);
    TView st; st.n = n; st.h = L.H; st.w = L.W; st.c = L.cin; st.stride = roundup(L.cin, 8); st.dt = L.in_dt; st.ptr = L.d_h;
    TView mid = st, nw = st; mid.ptr = L.d_rh; nw.ptr = L.d_hn;
    const TView *ins[3] = {&in, &st, &nw}, *res[3] = {L.rshortcut ? &st : nullptr, &mid, nullptr}, *outs[3] = {&mid, &nw, &L.out};
    const bool post = !act_is_slope(L.act);          // an activation the conv epilogue does not apply (the section's default, logistic, is one)
    for (int q = 0; q < 3; ++q) {
        const Layer &S = L.sub[q];
        ConvArgs a; memset(&a, 0, sizeof a);
        a.in = ins[q]->ptr; a.in_stride = ins[q]->stride; a.wt = S.d_w; a.bias = S.d_b; a.out = outs[q]->ptr; a.out_stride = outs[q]->stride; a.out_dt = outs[q]->dt; a.in_dt = S.in_dt;
        a.out_inv_scale = 1.f; a.res_scale = 1.f; a.mid_scale = 1.f; a.mid_inv_scale = 1.f;
        if (res[q] && !post) { a.res = res[q]->ptr; a.res_stride = res[q]->stride; }
        a.N = n; a.H = L.H; a.W = L.W; a.Cin_pad = S.cin_pad; a.Ho = L.H; a.Wo = L.W; a.Cout = S.filters;
        a.ksize = 3; a.stride = 1; a.pad = 1; a.Kpad = S.kpad; a.kchunk = conv_kchunk(S.cin_pad, S.in_dt); a.act = post ? ACT_LINEAR : S.act; a.zeros = c->d_zeros;
        conv_finalize(a);
        if (c->dtype == YOLO_FP32) HIPCK(c, launch_conv_f32(a, s));
        else HIPCK(c, launch_conv_bf16(a, conv_resolve_cfg(a, -1), s));
        if (post) {          // as a conv layer with such an activation: a linear epilogue, k_activate in place; then the sum the epilogue could not take
            TView o = *outs[q]; o.n = n;
            HIPCK(c, launch_activate(o, false, L.act, s));
            if (res[q]) HIPCK(c, launch_add(o, *res[q], o, s));
        }
    }
    HIPCK(c, hipMemcpyAsync(L.d_h, L.d_hn, (size_t)n * state_elems(c, L) * dt_size(L.in_dt), hipMemcpyDeviceToDevice, s));
    return YOLO_OK;
}

// ---- states across forwards of the library's own (yolo_time_forward, yolo_time_layers and through them yolo_autotune): kept before, handed back after.
//      Per recurrent layer 8 bytes per element of d_state_keep: the operand-type state, then the layer's fp32 tensor ([gru] state, [lstm] cell) ----
static int state_move(yolo_ctx *c, bool restore)
{
    char *k = (char *)c->d_state_keep;
    for (Layer &L : c->layers) {
        if (!has_state(L)) continue;
        const size_t ne = (size_t)c->max_batch * state_elems(c, L), es = dt_size(L.in_dt);
        float *f32 = L.type == L_CRNN ? nullptr : L.rkind == RECUR_GRU ? L.d_h32 : L.d_c;
        HIPCK(c, restore ? hipMemcpyAsync(L.d_h, k, ne * es, hipMemcpyDeviceToDevice, c->stream) : hipMemcpyAsync(k, L.d_h, ne * es, hipMemcpyDeviceToDevice, c->stream));
        if (f32) HIPCK(c, restore ? hipMemcpyAsync(f32, k + ne * 4, ne * 4, hipMemcpyDeviceToDevice, c->stream) : hipMemcpyAsync(k + ne * 4, f32, ne * 4, hipMemcpyDeviceToDevice, c->stream));
        k += ne * 8;
    }
    return YOLO_OK;
}
// the frame-average ring: between keep and restore the positions stand still (run_decode issues no advance), so every pass writes the same one slot per stream
static int ring_move(yolo_ctx *c, bool restore)
{
    HIPCK(c, launch_ring_slot_move(c->d_ring, c->d_ring_keep, c->d_ring_pos, c->max_batch, c->ring_elems(), restore, c->stream));
    return YOLO_OK;
}
// ring_frozen is set only once everything is kept, and cleared by every restore whatever fails in it: no error path leaves the positions standing still
int state_keep(yolo_ctx *c)
{
    if (!c->states.empty()) if (int r = state_move(c, false)) return r;
    if (c->avg_k > 1) { if (int r = ring_move(c, false)) return r; c->ring_frozen = true; }
    return YOLO_OK;
}
int state_restore(yolo_ctx *c)
{
    int r = c->states.empty() ? YOLO_OK : state_move(c, true);
    if (c->avg_k > 1 && c->ring_frozen) { c->ring_frozen = false; const int r2 = ring_move(c, true); if (!r) r = r2; }
    return r;
}
namespace { struct StateGuard { yolo_ctx *c; ~StateGuard() { state_restore(c); } }; }      // hands the states back on every return path

static void yolo_anchors(const yolo_ctx *c, const Layer &Y, float *out)      // a [yolo] head's anchors in cells: pixels over the head's stride
{
    const int stride[2] = {c->in_w / Y.W, c->in_h / Y.H};          // along x (anchor widths), along y (anchor heights)
    for (int k = 0; k < 2 * Y.na; ++k) out[k] = (float)(1.0 * (double)Y.anchors[k] / (double)stride[k & 1]);
}

static int run_decode(yolo_ctx *c, int i, int n)
{
    const Layer &L = c->layers[i];
    hipStream_t s = c->stream;
    if (L.tree < 0 && c->lean && c->lean_thr > 0.f && c->lean_heads >= 1 && c->lean_heads <= 4) {
        // lean detect path: every [yolo] head is decoded by ONE launch, issued at the last head (the head tensors keep their own buffers)
        bool later_head = false;
        for (size_t k = i + 1; k < c->layers.size(); ++k) later_head |= c->layers[k].type == L_YOLO;
        if (later_head) return YOLO_OK;
        LeanArgs la; memset(&la, 0, sizeof la);
        long begin = 0;
        for (size_t k = 0; k < c->layers.size(); ++k) {
            const Layer &Y = c->layers[k];
            if (Y.type != L_YOLO) continue;
            const Layer &P = c->layers[k - 1];
            LeanHead &h = la.h[la.nheads++];
            h.raw = (const float *)P.out.ptr; h.obj = P.d_obj; h.raw_stride = P.out.stride; h.gh = Y.H; h.gw = Y.W; h.na = Y.na; h.row_off = Y.row_off; h.box_begin = begin;
            h.sx = (float)(c->in_w / Y.W); h.sy = (float)(c->in_h / Y.H); yolo_anchors(c, Y, h.anchors);
            begin += (long)n * Y.H * Y.W * Y.na;
        }
        la.total = begin; la.n = n; la.classes = L.classes; la.mode = c->decode; la.rows_total = c->rows;
        la.box4 = c->d_box4; la.reject_below = c->lean_thr; la.list = (uint4 *)c->d_lean_list; la.list_count = c->d_lean_cnt; la.list_cap = (unsigned)((size_t)c->max_batch * c->rows);
        // the list counter must be zero: the NMS launch of the previous detect call resets it; if none ran since the last decode
        // (a failed call in between), a memset does
        if (c->lean_cnt_dirty) HIPCK(c, hipMemsetAsync(c->d_lean_cnt, 0, 4, s));
        c->lean_cnt_dirty = true;
        HIPCK(c, launch_decode_lean(la, c->d_scores, c->d_labels, s));
        return YOLO_OK;
    }
    const Layer &P = c->layers[i - 1];
    DecodeArgs d; memset(&d, 0, sizeof d);          // one fill for the three decode launches below
    d.raw = (const float *)P.out.ptr; d.raw_stride = P.out.stride; d.n = n; d.gh = L.H; d.gw = L.W; d.na = L.na; d.classes = L.classes;
    d.img_h = c->in_h; d.img_w = c->in_w; d.mode = c->decode; d.region = L.type == L_REGION;
    if (L.type == L_YOLO) yolo_anchors(c, L, d.anchors);
    else std::copy(L.anchors.begin(), L.anchors.begin() + 2 * L.na, d.anchors);          // [region]: already in cells
    d.det = c->lean ? nullptr : c->d_det; d.box4 = c->lean ? c->d_box4 : nullptr; d.rows_total = c->rows; d.row_off = L.row_off;
    d.reject_below = c->lean ? c->lean_thr : -INFINITY;
    // [region] with a softmax tree.  Full form: the decoded tensor with absolute class probabilities (scored at postprocess time, with the hier_thresh of that moment); descent form (yolo_detect*): box4, scores, labels straight from the raw tensor
    if (c->avg_k > 1) {
        // frame averaging: this call is one time step of the streams 0 .. n - 1.  Ring store + mean + full decode per head; once the last head has read the
        // positions they move on (not between the timing entry points' keep and restore: steps of no stream)
        const float alpha = (float)(1. / c->avg_k);
        const RingArgs g{c->d_ring, c->d_ring_pos, c->avg_k, c->max_batch, c->ring_elems(), (size_t)L.row_off * c->attrs, alpha};
        HIPCK(c, launch_decode_avg(d, g, c->d_scores, c->d_labels, s));
        bool later_head = false;
        for (size_t k = i + 1; k < c->layers.size(); ++k) later_head |= is_head_layer(c->layers[k]);
        if (!later_head && !c->ring_frozen) HIPCK(c, launch_ring_advance(c->d_ring_pos, n, c->avg_k, s));
        return YOLO_OK;
    }
    if (L.tree < 0) HIPCK(c, launch_decode(d, c->d_scores, c->d_labels, s));
    else if (c->lean) { HIPCK(c, launch_decode_region_tree_lean(d, c->trees[L.tree].dev, c->hier_thresh, c->d_scores, c->d_labels, s)); c->lean_hier = c->hier_thresh; }
    else HIPCK(c, launch_decode_region_tree(d, c->trees[L.tree].dev, s));
    return YOLO_OK;
}

int run_layer(yolo_ctx *c, int i, int n)
{
    Layer &L = c->layers[i];
    hipStream_t s = c->stream;
    switch (L.type) {
    case L_CONV:
        if (int r = run_conv(c, i, n)) return r;
        if (L.post_act != ACT_LINEAR) HIPCK(c, launch_activate(nview(n, L.out), L.pair, L.post_act, s));
        break;
    case L_SHORTCUT:
        if (L.general) {          // DN/blas.c:68-92 + the layer's activation, one launch
            HIPCK(c, launch_shortcut(nview(n, view_of(c, L.in[0])), nview(n, view_of(c, L.in[1])), nview(n, L.out), L.pair, L.act, s));
        } else if (!L.noop && L.pair) {
            HIPCK(c, launch_add_split(view_of(c, L.in[0]).ptr, view_of(c, L.in[0]).stride, view_of(c, L.in[1]).ptr, view_of(c, L.in[1]).stride, L.out.ptr, L.out.stride, roundup(L.C, 32), (size_t)n * L.H * L.W, s));
        } else if (!L.noop) {
            float sa = 1.f, sb = 1.f, so = 1.f;
            if (c->dtype == YOLO_FP8) { sa = c->eff_scale[L.in[0]]; sb = c->eff_scale[L.in[1]]; so = 1.f / c->eff_scale[i]; }
            HIPCK(c, launch_add(nview(n, view_of(c, L.in[0])), nview(n, view_of(c, L.in[1])), nview(n, L.out), s, sa, sb, so));
        }
        break;
    case L_ROUTE:
        for (size_t k = 0; k < L.copy_inputs.size(); ++k) {
            TView src = nview(n, view_of(c, L.copy_inputs[k])); TView dst = nview(n, L.out);
            dst.ptr = (char *)dst.ptr + (size_t)L.copy_offsets[k] * dt_size(dst.dt); dst.c = src.c;
            if (L.pair) {        // interleaved pairs: the source's 2 * Cp elements at twice the channel offset (whole 32-channel groups: the planner refuses the rest)
                if (src.c % 32 || L.copy_offsets[k] % 32) return fail(c, YOLO_ERR_STATE, "internal: route copy of a pair tensor: %d channels at offset %d", src.c, L.copy_offsets[k]);
                TView dv = nview(n, L.out);
                dv.ptr = (char *)L.out.ptr + (size_t)2 * L.copy_offsets[k] * 2; dv.c = 2 * src.c; src.c = 2 * src.c;
                HIPCK(c, launch_copy(src, dv, s));
                continue;
            }
            // a source at a whole-granule offset is copied granule by granule (the zeros behind a ragged channel count come along and end the
            // concatenation's last granule, or are overwritten by the next source's copy); at any other offset element by element, and the last
            // source then writes the zeros up to the end of the granule itself
            if (L.copy_offsets[k] % 8 == 0 && dst.dt != DT_FP8) { HIPCK(c, launch_copy(src, dst, s)); continue; }
            if (dst.dt == DT_FP8) { if (src.c % 8) return fail(c, YOLO_ERR_STATE, "internal: route copy of %d e4m3 channels", src.c); HIPCK(c, launch_copy(src, dst, s)); continue; }
            const int end = L.copy_offsets[k] + src.c;
            HIPCK(c, launch_copy_channels(src, dst, s, end == L.C ? std::min(L.out.stride, roundup(L.C, 8)) - L.copy_offsets[k] : 0));
        }
        break;
    case L_LOCAL:
        HIPCK(c, launch_local(nview(n, view_of(c, L.in[0])), nview(n, L.out), L.d_w, L.d_b, L.size, L.stride, L.pad, L.act, s));
        if (L.post_act != ACT_LINEAR) HIPCK(c, launch_activate(nview(n, L.out), false, L.post_act, s));
        break;
    case L_DECONV: case L_GCONV: case L_XCONV:
        HIPCK(c, launch_side_conv(c, L, n, s));
        if (L.post_act != ACT_LINEAR) HIPCK(c, launch_activate(nview(n, L.out), false, L.post_act, s));
        break;
    case L_ACTIVATE: {
        TView out = nview(n, L.out);
        if (!L.inplace) {          // a tensor of its own (keep_layers, a second reader of the producer, a concat window): copied first
            // whole granules: the channels C .. of the last one are the producer's zeros, not what the pooled buffer's last tenant left there
            // (a consumer multiplies them by zero filters, and 0 * Inf is NaN)
            TView src = nview(n, view_of(c, L.in[0])), dst = out;
            src.c = dst.c = L.pair ? pair_width(L.C) : std::min(src.stride, store_width(L, L.C));
            HIPCK(c, launch_copy_channels(src, dst, s));
        }
        HIPCK(c, launch_activate(out, L.pair, L.act, s));
        break; }
    case L_L2NORM: HIPCK(c, launch_l2norm(nview(n, view_of(c, L.in[0])), nview(n, L.out), s)); break;
    case L_LRN: HIPCK(c, launch_lrn(nview(n, view_of(c, L.in[0])), nview(n, L.out), L.size, L.lrn_alpha, L.lrn_beta, L.lrn_kappa, s)); break;
    case L_CROP: HIPCK(c, launch_crop(nview(n, view_of(c, L.in[0])), nview(n, L.out), L.crop_adjust, s)); break;          // (layer 0: the staged input, 3 of whose 8 channels are the image's)
    case L_UPSAMPLE:
        if (L.pstride != 2 || L.up_scale != 1.f) {          // (never pairs: the planner refuses these in the split-fp16 configuration)
            if (c->semantics == YOLO_SEM_DARKNET) { HIPCK(c, launch_upsample_nearest(nview(n, view_of(c, L.in[0])), nview(n, L.out), L.pstride, L.up_scale, s)); break; }
            HIPCK(c, launch_upsample2x(nview(n, view_of(c, L.in[0])), nview(n, L.out), 1, s));
            HIPCK(c, launch_scale(nview(n, L.out), L.up_scale, s));
            break;
        }
        if (L.pair && getenv("YOLO_PAIR_UPSAMPLE_VIA_F32")) { if (int r = via_f32(c, L, n)) return r; }
        else if (L.pair) HIPCK(c, launch_upsample2x_pair(nview(n, view_of(c, L.in[0])), nview(n, L.out), c->semantics == YOLO_SEM_TF, s));
        else HIPCK(c, launch_upsample2x(nview(n, view_of(c, L.in[0])), nview(n, L.out), c->semantics == YOLO_SEM_TF, s));
        break;
    case L_MAXPOOL:          // (split fp16: no pair form of the pool and the reorg)
        if (L.pair) { if (int r = via_f32(c, L, n)) return r; }
        else HIPCK(c, launch_maxpool(nview(n, view_of(c, L.in[0])), nview(n, L.out), L.psize, L.pstride, L.ppad, s));
        break;
    case L_REORG:
        if (L.pair) { if (int r = via_f32(c, L, n)) return r; }
        else HIPCK(c, launch_reorg(nview(n, view_of(c, L.in[0])), nview(n, L.out), L.pstride, c->semantics == YOLO_SEM_DARKNET, s));
        break;
    case L_AVGPOOL: {
        if (L.pool_fused) break;             // pooled inside the [softmax] launch that follows
        const TView in = nview(n, view_of(c, L.in[0]));
        HIPCK(c, launch_avgpool(in, c->pair_of(L.in[0]) && in.dt == DT_F16, nview(n, L.out), s));
        break; }
    case L_SOFTMAX: {
        SoftmaxArgs a; memset(&a, 0, sizeof a);
        a.n = n; a.groups = L.groups; a.len = L.C / L.groups; a.temperature = L.temperature; a.probs = (float *)L.out.ptr; a.p_stride = L.out.stride;
        a.top_k = i == c->cls_layer ? c->cls_topk : 0; a.cls = c->d_cls_idx; a.topk_probs = c->d_cls_prob;      // (yolo_classify*: the output layer also selects)
        const Layer &P = c->layers[L.in[0]];
        if (L.tree >= 0) {
            // hierarchical softmax: conditional probabilities are the layer's output (what network_predict returns); the output layer of
            // a classify call writes the form yolo_set_hierarchy_mode selected and takes its top-k from it
            const TView in = view_of(c, L.in[0]);
            if (in.dt != DT_F32) return fail(c, YOLO_ERR_STATE, "layer %d: [softmax] input is not fp32", i);
            const TreeRows rows{(const float *)in.ptr, (size_t)n, 1, in.stride, 0, 0};
            HIPCK(c, launch_tree_softmax(c->trees[L.tree].dev, rows, L.temperature, i == c->cls_layer ? c->cls_mode : TREE_CONDITIONAL, a.probs, a.p_stride,
                                         a.top_k, a.cls, a.topk_probs, s));
            break;
        }
        if (P.type == L_AVGPOOL && P.pool_fused) {
            const TView in = nview(n, view_of(c, P.in[0]));
            if (!avgpool_softmax_ok(in, a)) return fail(c, YOLO_ERR_STATE, "layer %d: the fused [avgpool] + [softmax] launch does not apply to this plan", i);
            HIPCK(c, launch_avgpool_softmax(in, (float *)P.out.ptr, P.out.stride, a, s));
        } else {
            const TView in = view_of(c, L.in[0]);
            if (in.dt != DT_F32) return fail(c, YOLO_ERR_STATE, "layer %d: [softmax] input is not fp32", i);
            a.x = (const float *)in.ptr; a.x_stride = in.stride;
            HIPCK(c, launch_softmax_topk(a, s));
        }
        break; }
    case L_DETECT: {
        const Layer &P = c->layers[i - 1];
        HIPCK(c, launch_decode_v1((const float *)P.out.ptr, P.out.stride, n, L.side, L.na, L.classes, L.sqr, c->d_det, c->rows, L.row_off,
                                  c->d_scores, c->d_labels, s));
        break; }
    case L_YOLO: case L_REGION: return run_decode(c, i, n);
    case L_RECUR: return run_recurrent(c, i, n);
    case L_CRNN: return run_crnn(c, i, n);
    }
    return YOLO_OK;
}

// ---- input staging.  Every site that writes the network input does: auto [dst, dt] = input_fill_dst(c); its own fill launch into dst (c->input.stride channels per
//      pixel: 8 for an RGB image, roundup(N, 8) for N planes; pairs: 8, in fp32); input_filled(c, pixels) ----
static int fill_stride(const yolo_ctx *c) { return c->in_pair ? 8 : c->input.stride; }
static std::pair<void *, int> input_fill_dst(yolo_ctx *c)      // (pointer, element type).  Split fp16: the fill writes the image in fp32 (exact for uint8 pixels x scale up to fp32 rounding), input_filled splits it into pairs
{
    c->stem_u8 = nullptr;          // from here on the fused stem reads the filled input, not a caller's uint8 image: ahead of the fill launch, so also when that launch is refused
    using P = std::pair<void *, int>; return c->in_pair ? P(c->d_f32a, DT_F32) : P(c->input.ptr, c->input.dt);
}
static hipError_t input_filled(yolo_ctx *c, size_t npix) { return c->in_pair ? launch_split_from_f32(c->d_f32a, 8, c->input.ptr, 24, 8, npix, c->stream, PAIR_B3) : hipSuccess; }

int stage_in(yolo_ctx *c, const void *images, int n, int fmt, int loc, float scale)
{
    if (n < 1 || n > c->max_batch) return fail(c, YOLO_ERR_INVALID, "batch %d outside 1..%d", n, c->max_batch);
    if (!images) return fail(c, YOLO_ERR_INVALID, "images == NULL");
    size_t npix = (size_t)n * c->in_h * c->in_w;
    const void *src = images;
    if (loc == YOLO_HOST) {
        HIPCK(c, hipMemcpyAsync(c->d_stage, images, npix * c->in_c * (fmt == YOLO_IMG_U8 ? 1 : 4), hipMemcpyHostToDevice, c->stream));
        src = c->d_stage;
    }
    // uint8 images of a network whose first layers run as the fused stem: the stem converts the pixels itself (conv_stem.hip, U8 form).
    // That form gathers the raw rows in aligned dwords through a descriptor that ends with the image tensor: a batch whose byte count is no
    // multiple of 4 (odd width x odd height x odd n) would lose its last 1-3 bytes to the range check, so it takes the conversion launch
    if (fmt == YOLO_IMG_U8 && c->layers.size() > 1 && never_stored(c->layers[0], 0) && (double)npix * 3 < 2147483648.0 && ((size_t)src & 3) == 0 && (npix * 3) % 4 == 0) {
        c->stem_u8 = (const uint8_t *)src; c->stem_scale = scale; c->stem_u8_n = n;
        return YOLO_OK;
    }
    auto [dst, dt] = input_fill_dst(c);
    HIPCK(c, launch_preprocess(src, fmt, n, c->in_h * c->in_w, scale, dst, dt, fill_stride(c), c->stream, c->in_mul, c->in_add, c->in_c));
    HIPCK(c, input_filled(c, npix));
    return YOLO_OK;
}

// the layer sequence of one forward.  `skip_conv`: the timing pass that runs everything but the convs (dense, grouped and xnor, not [deconvolutional]; conv_flops counts them all); `ev`: per-layer events (yolo_time_layers)
static int run_layers(yolo_ctx *c, int n, bool skip_conv = false, std::vector<hipEvent_t> *ev = nullptr)
{
    const int NL = (int)c->layers.size();
    for (int i = 0; i < NL; ++i) {
        if (!(skip_conv && (c->layers[i].type == L_CONV || (is_side_conv(c->layers[i]) && c->layers[i].type != L_DECONV)))) { int r = run_layer(c, i, n); if (r) return r; }
        if (ev) HIPCK(c, hipEventRecord((*ev)[i + 1], c->stream));
    }
    return YOLO_OK;
}

// What a finished forward of n images leaves for yolo_postprocess* / yolo_darknet_boxes*.  lean: the decode wrote scores, labels and box4, not the tensor; scores_mode: what d_scores holds now (< 0: left as it is); fit >= 0: the input was a ragged batch fitted that way
static void forward_done(yolo_ctx *c, int n, bool lean, int scores_mode = 0, int fit = -1)
{
    c->lean = lean && c->lean_ok && c->avg_k < 2; c->det_valid = !c->lean; c->last_n = n;          // (frame averaging: always the full decode, the lean one never forms what is averaged)
    if (scores_mode >= 0) c->scores_mode = scores_mode;
    if (fit >= 0) { c->geom_fit = fit; c->geom_n = n; }
}

int run_network(yolo_ctx *c, int n, bool lean, int fit)
{
    c->lean = lean && c->lean_ok && c->avg_k < 2;          // (run_decode reads it)
    if (int r = run_layers(c, n)) { c->lean = false; return r; }
    forward_done(c, n, lean, 0, fit);
    return YOLO_OK;
}

int output_layer(const yolo_ctx *c)
{
    int o = (int)c->layers.size() - 1;
    while (o >= 0 && c->layers[o].cost) --o;
    return o;
}

// the entry points that read images refuse a vector-input network by name, and point at the two that serve it
int need_image(yolo_ctx *c, const char *what)
{
    if (c->vec_n) return fail(c, YOLO_ERR_INVALID, "%s: the network is a vector-input network ([net] yolo_input=vector: its input is a row of %d values, not an image); use yolo_forward_vectors / yolo_sequence", what, c->vec_n);
    return YOLO_OK;
}

int need_detector(yolo_ctx *c, const char *what)
{
    if (int r = need_image(c, what)) return r;
    if (c->map_layer >= 0) return fail(c, YOLO_ERR_INVALID, "%s: the network is a map network ([net] yolo_output=map: its output is an image-shaped tensor, it has no detection head); use yolo_output_map / yolo_label_map / yolo_segment_images_u8", what);
    if (c->cls_layer >= 0) return fail(c, YOLO_ERR_INVALID, "%s: the network is a classifier (its output layer is a [softmax], it has no detection head); use yolo_classify*", what);
    return YOLO_OK;
}

int post_args_ok(yolo_ctx *c, int max_out, int nms_mode, int select_mode)
{
    if (int r = need_detector(c, "threshold + NMS")) return r;
    if (max_out < 1) return fail(c, YOLO_ERR_INVALID, "max_out < 1");
    if (nms_mode < 0 || nms_mode > 4 || select_mode < 0 || select_mode > 1) return fail(c, YOLO_ERR_INVALID, "bad nms/select mode");
    return YOLO_OK;
}

int copy_out(yolo_ctx *c, void *dst, const void *src, size_t bytes, int loc)
{
    if (loc == YOLO_HOST) { HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream)); HIPCK(c, hipStreamSynchronize(c->stream)); }
    else HIPCK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return YOLO_OK;
}

int post(yolo_ctx *c, const float *det, int n, int rows, int attrs, float score_thr, float iou_thr, int max_out,
         int nms_mode, int select_mode, int img_h, int img_w, int scores_ready, yolo_box *boxes_out, int32_t *counts_out, int out_loc, int32_t *rows_out,
         const PostGeom *geom)
{
    if (int r = post_args_ok(c, max_out, nms_mode, select_mode)) return r;
    size_t need = (size_t)n * max_out;
    if ((int)need > c->boxes_cap) {
        // a captured detect graph holds the old pointer (memset, NMS writes, D2D copy): it must not be replayed
        drop_graph(c);
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (c->d_boxes) HIPCK(c, hipFree(c->d_boxes));
        if (c->d_rows) HIPCK(c, hipFree(c->d_rows));
        c->d_boxes = nullptr; c->d_rows = nullptr; c->boxes_cap = 0;
        HIPCK(c, hipMalloc(&c->d_boxes, need * sizeof(yolo_box))); HIPCK(c, hipMalloc((void **)&c->d_rows, need * 4)); c->boxes_cap = (int)need;
    }
    if (rows_out && !c->d_srow) HIPCK(c, hipMalloc((void **)&c->d_srow, (size_t)c->max_batch * c->rows * 4));
    PostArgs p; memset(&p, 0, sizeof p);
    p.det = det; p.box4 = (det == c->d_det && !c->det_valid) ? c->d_box4 : nullptr; p.n = n; p.rows = rows; p.attrs = attrs; p.score_thr = score_thr; p.iou_thr = iou_thr; p.max_out = max_out;
    p.nms_mode = nms_mode; p.select_mode = select_mode; p.img_h = img_h; p.img_w = img_w; p.scores_ready = scores_ready;
    p.scores = c->d_scores; p.labels = c->d_labels; p.cand = c->d_cand; p.keys = c->d_keys; p.rows_pow2 = c->rows_pow2;
    p.sbox = c->d_sbox; p.slabel = c->d_slabel; p.sscore = c->d_sscore; p.boxes_out = c->d_boxes; p.counts_out = c->d_counts;
    // device-resident outputs are written by the NMS kernel itself (it also zeroes the unused slots): no memset, no copies
    const bool direct_b = boxes_out && out_loc != YOLO_HOST, direct_c = counts_out && out_loc != YOLO_HOST;
    if (direct_b) p.boxes_out = boxes_out;
    if (direct_c) p.counts_out = (int *)counts_out;
    if (rows_out) { p.srow = c->d_srow; p.rows_out = out_loc != YOLO_HOST ? (int *)rows_out : c->d_rows; }
    if (c->lean_cnt_dirty) p.zero_word = c->d_lean_cnt;
    if (geom) {
        p.geom = c->d_descs; p.geom_fit = geom->fit; p.geom_pixels = geom->pixels; p.netw = c->in_w; p.neth = c->in_h;
        // a letterboxed box leaves darknet's correction in source pixels, unless V2's per-class NMS scales it to the image itself
        p.geom_relative = !(geom->pixels && nms_mode != YOLO_NMS_PER_CLASS);
        p.geom_net_pixels = c->decode == YOLO_DECODE_PIXEL;          // [region] / [detection] heads always decode normalised boxes
        for (auto &L : c->layers) if (L.type == L_REGION || L.type == L_DETECT) p.geom_net_pixels = 0;
    }
    HIPCK(c, launch_postprocess(p, c->stream));
    c->lean_cnt_dirty = false;
    if (rows_out && out_loc == YOLO_HOST) { int r = copy_out(c, rows_out, c->d_rows, need * 4, out_loc); if (r) return r; }
    if (boxes_out && !direct_b) { int r = copy_out(c, boxes_out, c->d_boxes, need * sizeof(yolo_box), out_loc); if (r) return r; }
    if (counts_out && !direct_c) { int r = copy_out(c, counts_out, c->d_counts, (size_t)n * 4, out_loc); if (r) return r; }
    return YOLO_OK;
}

// decoded video frames: what is wrong with frame `i`'s descriptor inside a packed buffer of `bytes` bytes, before anything reads it
int frame_desc_check(const yolo_frame_desc &d, size_t bytes, int i, std::string &msg)
{
    char b[256];
    auto bad = [&](const char *fmt, auto... a) { snprintf(b, sizeof b, fmt, a...); msg = "frame " + std::to_string(i) + ": " + b; return (int)YOLO_ERR_INVALID; };
    const bool jpeg = pix_is_jpeg(d.format);
    if ((d.format < YOLO_PIX_NV12 || d.format > YOLO_PIX_BGR24) && !jpeg) return bad("unknown format %d", (int)d.format);
    if (d.matrix < YOLO_MATRIX_BT601 || d.matrix > YOLO_MATRIX_BT601_FULL) return bad("unknown matrix %d", (int)d.matrix);
    if (jpeg && d.matrix != 0) return bad("matrix %d with a JPEG format: the format carries its colour rule, the matrix must be 0", (int)d.matrix);
    if (d.h < 1 || d.w < 1) return bad("%d x %d", (int)d.h, (int)d.w);
    const uint64_t ch = jpeg ? (uint64_t)jpeg_chroma_rows(d.format, d.h) : ((uint64_t)d.h + 1) / 2, cw = jpeg ? (uint64_t)jpeg_chroma_cols(d.format, d.w) : ((uint64_t)d.w + 1) / 2;
    // the planes the format has: rows and bytes per row
    const int planes = d.format == YOLO_PIX_NV12 ? 2 : d.format == YOLO_PIX_I420 || (jpeg && d.format != YOLO_PIX_JPEG_GREY) ? 3 : 1;
    for (int p = 0; p < planes; ++p) {
        const uint64_t rows = p == 0 ? (uint64_t)d.h : ch;
        const uint64_t row = d.format == YOLO_PIX_RGB24 || d.format == YOLO_PIX_BGR24 ? 3 * (uint64_t)d.w : p == 0 ? (uint64_t)d.w : d.format == YOLO_PIX_NV12 ? 2 * cw : cw;
        if (d.pitch[p] < row) return bad("plane %d: pitch %llu below the row's %llu bytes", p, (unsigned long long)d.pitch[p], (unsigned long long)row);
        if (d.pitch[p] > 0xffffffffull) return bad("plane %d: pitch %llu does not fit 32 bits", p, (unsigned long long)d.pitch[p]);
        if (d.offset[p] > 0xffffffffull || (rows - 1) * d.pitch[p] + row > 0xffffffffull - d.offset[p])
            return bad("plane %d: %llu rows of pitch %llu at offset %llu pass 32 bits", p, (unsigned long long)rows, (unsigned long long)d.pitch[p], (unsigned long long)d.offset[p]);
        if (d.offset[p] + (rows - 1) * d.pitch[p] + row > (uint64_t)bytes)
            return bad("plane %d: %llu rows of pitch %llu (%llu bytes each) at offset %llu end past the %zu-byte buffer", p, (unsigned long long)rows, (unsigned long long)d.pitch[p],
                       (unsigned long long)row, (unsigned long long)d.offset[p], bytes);
    }
    return YOLO_OK;
}

}  // namespace yolo_impl

extern "C" {

// lean: the caller goes straight on to threshold + NMS (yolo_detect*): the decoded tensor is not written, see yolo_ctx::lean
static int forward_impl(yolo_ctx *c, const void *images, int n, int fmt, int loc, float scale, float *det_out, int out_loc, bool lean, float score_thr = 0.f)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = need_image(c, "yolo_forward")) return r;
    c->lean_thr = score_thr;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "yolo_forward before weights were loaded");
    if (fmt != YOLO_IMG_U8 && fmt != YOLO_IMG_F32 && fmt != YOLO_IMG_F32_CHW) return fail(c, YOLO_ERR_INVALID, "bad image format");
    HIPCK(c, hipSetDevice(c->device));
    int r = stage_in(c, images, n, fmt, loc, scale); if (r) return r;
    r = run_network(c, n, lean && !det_out); if (r) return r;
    return det_out ? copy_out(c, det_out, c->d_det, (size_t)n * c->rows * c->attrs * 4, out_loc) : YOLO_OK;
}

int yolo_forward(yolo_ctx *c, const void *images, int n, int fmt, int loc, float scale, float *det_out, int out_loc)
{
    return forward_impl(c, images, n, fmt, loc, scale, det_out, out_loc, false);
}

// One image at its own size -> the network input (`fill`, which `fill_name` names in the message) -> forward -> the decoded tensor.  `name`: the entry point.
// A host image gets a device copy of its own for the call, freed once the stream has drained -- also when the fill or the forward failed
typedef hipError_t (*FillOne)(yolo_ctx *c, const void *src, int h, int w, void *dst, int dt);
static int forward_one(yolo_ctx *c, const char *name, const char *fill_name, FillOne fill, const void *image, int h, int w, size_t bytes, int loc, float *det_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = need_image(c, name)) return r;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "%s before weights were loaded", name);
    if (!image || h < 1 || w < 1) return fail(c, YOLO_ERR_INVALID, "bad image");
    HIPCK(c, hipSetDevice(c->device));
    const void *src = image; void *tmp = nullptr;
    if (loc == YOLO_HOST) {
        HIPCK(c, hipMalloc(&tmp, bytes));
        HIPCK(c, hipMemcpyAsync(tmp, image, bytes, hipMemcpyHostToDevice, c->stream)); src = tmp;
    }
    auto [dst, dt] = input_fill_dst(c);
    hipError_t e = fill(c, src, h, w, dst, dt);
    if (e == hipSuccess) e = input_filled(c, (size_t)c->in_h * c->in_w);
    int r = e == hipSuccess ? run_network(c, 1) : fail(c, YOLO_ERR_HIP, "%s: %s", fill_name, hipGetErrorString(e));
    if (tmp) { hipStreamSynchronize(c->stream); hipFree(tmp); }
    if (r) return r;
    return det_out ? copy_out(c, det_out, c->d_det, (size_t)c->rows * c->attrs * 4, out_loc) : YOLO_OK;
}

int yolo_forward_image_u8(yolo_ctx *c, const uint8_t *image, int h, int w, int loc, float *det_out, int out_loc)
{
    const FillOne fill = [](yolo_ctx *c, const void *src, int h, int w, void *dst, int dt) { return launch_resize_u8((const uint8_t *)src, h, w, c->in_h, c->in_w, dst, dt, fill_stride(c), 8, c->stream, c->in_mul, c->in_add, c->in_c); };
    return forward_one(c, "yolo_forward_image_u8", "resize", fill, image, h, w, (size_t)h * w * (c ? c->in_c : 3), loc, det_out, out_loc);
}

int yolo_forward_letterbox_chw(yolo_ctx *c, const float *image_chw, int w, int h, int loc, float *det_out, int out_loc)
{
    const FillOne fill = [](yolo_ctx *c, const void *src, int h, int w, void *dst, int dt) { return launch_letterbox_chw((const float *)src, w, h, c->in_h, c->in_w, dst, dt, fill_stride(c), c->stream, c->in_c); };
    return forward_one(c, "yolo_forward_letterbox_chw", "letterbox", fill, image_chw, h, w, (size_t)h * w * (c ? c->in_c : 3) * 4, loc, det_out, out_loc);
}

static int postprocess_impl(yolo_ctx *c, int n, float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode,
                            yolo_box *boxes_out, int32_t *counts_out, int32_t *rows_out, int out_loc, const PostGeom *geom)
{
    if (int r = need_detector(c, "yolo_postprocess")) return r;
    if (n < 1 || n > c->last_n) return fail(c, YOLO_ERR_STATE, "postprocess of %d images but the last forward ran %d", n, c->last_n);
    HIPCK(c, hipSetDevice(c->device));
    if (c->tree_head >= 0) {
        // a softmax-tree head: score = objectness, label = hierarchy_top_prediction at the context's hier_thresh.  After a full decode
        // the rows are scored here; after the descent form they already are
        if (nms_mode == YOLO_NMS_NUMPY_V3) return fail(c, YOLO_ERR_UNSUPPORTED, "YOLO_NMS_NUMPY_V3 over a softmax-tree head");
        if (!c->det_valid && (score_thr < c->lean_thr || c->hier_thresh != c->lean_hier))
            return fail(c, YOLO_ERR_STATE, "the last forward ran through yolo_detect* with score threshold %g and hier_thresh %g; other values need yolo_forward", c->lean_thr, c->lean_hier);
        if (c->det_valid) if (int r = score_tree_rows(c, n)) return r;
        c->scores_mode = 2;
        return post(c, c->d_det, n, c->rows, c->attrs, score_thr, iou_thr, max_out, nms_mode, select_mode,
                    nms_mode == YOLO_NMS_PER_CLASS ? c->in_h : 0, nms_mode == YOLO_NMS_PER_CLASS ? c->in_w : 0, 1, boxes_out, counts_out, out_loc, rows_out, geom);
    }
    const int want = nms_mode == YOLO_NMS_NUMPY_V3 ? 1 : 0;
    if (!c->det_valid && score_thr < c->lean_thr)
        return fail(c, YOLO_ERR_STATE, "the last forward ran through yolo_detect* with score threshold %g and pruned the scores below it; a lower threshold needs yolo_forward", c->lean_thr);
    if (!c->det_valid && want != c->scores_mode)
        return fail(c, YOLO_ERR_STATE, "the last forward ran through yolo_detect* without materialising the decoded tensor; this NMS flavour needs it (call yolo_forward)");
    const int ready = c->scores_mode == want;
    c->scores_mode = want;
    return post(c, c->d_det, n, c->rows, c->attrs, score_thr, iou_thr, max_out, nms_mode, select_mode,
                nms_mode == YOLO_NMS_PER_CLASS ? c->in_h : 0, nms_mode == YOLO_NMS_PER_CLASS ? c->in_w : 0, ready, boxes_out, counts_out, out_loc, rows_out, geom);
}

int yolo_postprocess_rows(yolo_ctx *c, int n, float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode,
                          yolo_box *boxes_out, int32_t *counts_out, int32_t *rows_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    return postprocess_impl(c, n, score_thr, iou_thr, max_out, nms_mode, select_mode, boxes_out, counts_out, rows_out, out_loc, nullptr);
}

int yolo_postprocess(yolo_ctx *c, int n, float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode,
                     yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    return yolo_postprocess_rows(c, n, score_thr, iou_thr, max_out, nms_mode, select_mode, boxes_out, counts_out, nullptr, out_loc);
}

int yolo_detect(yolo_ctx *c, const void *images, int n, int fmt, int loc, float scale, float score_thr, float iou_thr,
                int max_out, int nms_mode, int select_mode, yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = post_args_ok(c, max_out, nms_mode, select_mode)) return r;      // before the forward: a decode whose NMS never runs leaves the lean list counter set
    int r = forward_impl(c, images, n, fmt, loc, scale, nullptr, YOLO_DEVICE, nms_mode != YOLO_NMS_NUMPY_V3, score_thr); if (r) return r;
    return yolo_postprocess(c, n, score_thr, iou_thr, max_out, nms_mode, select_mode, boxes_out, counts_out, out_loc);
}

// ---- the captured detect step (yolo_ctx::graph).  One call of step `g` with the checked arguments `k`: the first call with a key runs `eager` (forward + threshold + NMS from k), the second
//      captures it, later ones replay; a stream that cannot be captured stays eager (-1).  *replayed: a graph launch ran, so what an eager call writes on the host is the caller's to write (forward_done) ----
using GraphKey = yolo_ctx::GraphKey;
typedef int (*GraphEager)(yolo_ctx *c, const GraphKey &k);
static int graph_step(yolo_ctx *c, yolo_ctx::GraphStep &g, const GraphKey &k, GraphEager eager, bool *replayed)
{
    if (memcmp(&k, &g.key, sizeof k) != 0) {
        if (g.exec) { hipGraphExecDestroy(g.exec); g.exec = nullptr; }
        g.key = k; if (g.state >= 0) g.state = 0;
    }
    if (g.state <= 0) { int r = eager(c, k); if (r == YOLO_OK && g.state == 0) g.state = 1; return r; }
    HIPCK(c, hipSetDevice(c->device));
    if (g.state == 1) {
        hipGraph_t gr = nullptr;
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { (void)hipGetLastError(); g.state = -1; return eager(c, k); }
        int r = eager(c, k);
        hipError_t e = hipStreamEndCapture(c->stream, &gr);
        if (r != YOLO_OK || e != hipSuccess || !gr) { (void)hipGetLastError(); if (gr) hipGraphDestroy(gr); g.state = -1; return r ? r : eager(c, k); }
        e = hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0);
        hipGraphDestroy(gr);
        if (e != hipSuccess) { (void)hipGetLastError(); g.exec = nullptr; g.state = -1; return eager(c, k); }
        g.state = 2;
    }
    // the captured step holds no reset of the lean decode's list counter (its NMS node leaves it at zero): a step that failed between its decode and its NMS since then left it set
    if (c->lean_cnt_dirty) { HIPCK(c, hipMemsetAsync(c->d_lean_cnt, 0, 4, c->stream)); c->lean_cnt_dirty = false; }
    HIPCK(c, hipGraphLaunch(g.exec, c->stream));
    *replayed = true;
    return YOLO_OK;
}

int yolo_detect_graph(yolo_ctx *c, const void *images, int n, int fmt, float scale, float score_thr, float iou_thr, int max_out,
                      int nms_mode, int select_mode, yolo_box *boxes_out, int32_t *counts_out)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!images || !boxes_out || !counts_out) return fail(c, YOLO_ERR_INVALID, "yolo_detect_graph needs device pointers for images, boxes_out and counts_out");
    if (int r = post_args_ok(c, max_out, nms_mode, select_mode)) return r;
    GraphKey k; memset(&k, 0, sizeof k);
    k.src = images; k.n = n; k.fmt = fmt; k.scale = scale; k.st = score_thr; k.it = iou_thr; k.mo = max_out; k.nm = nms_mode; k.sm = select_mode; k.bo = boxes_out; k.co = counts_out;
    const GraphEager eager = [](yolo_ctx *c, const GraphKey &k) -> int {
        int r = forward_impl(c, k.src, k.n, k.fmt, YOLO_DEVICE, k.scale, nullptr, YOLO_DEVICE, k.nm != YOLO_NMS_NUMPY_V3, k.st); if (r) return r;
        return yolo_postprocess(c, k.n, k.st, k.it, k.mo, k.nm, k.sm, (yolo_box *)k.bo, (int32_t *)k.co, YOLO_DEVICE);
    };
    bool replayed = false;
    if (int r = graph_step(c, c->graph[0], k, eager, &replayed)) return r;
    if (replayed) { c->lean_thr = score_thr; forward_done(c, n, nms_mode != YOLO_NMS_NUMPY_V3, nms_mode == YOLO_NMS_NUMPY_V3 ? 1 : 0); }      // (not stem_u8: kept, NOTEBOOK 2026-10-19)
    return YOLO_OK;
}

// ---- ragged batches of native-size images: one fit launch over a descriptor table, then the ordinary forward; the box mapping of the
//      postprocess reads the same table ("Ragged batches") ----
static_assert(sizeof(ImgDesc) == sizeof(yolo_image_desc) && sizeof(yolo_image_desc) == 16, "yolo_image_desc is the device table's row");

// one image's place in the packed buffer
static int desc_check(yolo_ctx *c, int i, const yolo_image_desc &d, size_t bytes)
{
    if (d.h < 1 || d.w < 1) return fail(c, YOLO_ERR_INVALID, "image %d: %d x %d", i, (int)d.h, (int)d.w);
    const uint64_t need = (uint64_t)d.h * (uint64_t)d.w * (uint64_t)c->in_c;
    if (d.offset > bytes || need > bytes - d.offset)
        return fail(c, YOLO_ERR_INVALID, "image %d: %d x %d x %d bytes at offset %llu end past the %zu-byte buffer", i, (int)d.h, (int)d.w, c->in_c, (unsigned long long)d.offset, bytes);
    return YOLO_OK;
}

// a fit the ragged entry points know, and one this network's images can take
static int fit_check(yolo_ctx *c, int fit, const char *who)
{
    if (fit < YOLO_FIT_STRETCH || fit > YOLO_FIT_CENTER_CROP) return fail(c, YOLO_ERR_INVALID, "bad fit %d", fit);
    // the cv2 fits restate cv2.resize of an RGB / BGR image: an image of another channel count has no such meaning
    if (c->in_c != 3 && (fit == YOLO_FIT_CV2 || fit == YOLO_FIT_CV2_BGR))
        return fail(c, YOLO_ERR_UNSUPPORTED, "%s: %s is not served for a network of %d planes ([net] yolo_input=planes): it fits an RGB / BGR image", who, fit == YOLO_FIT_CV2 ? "YOLO_FIT_CV2" : "YOLO_FIT_CV2_BGR", c->in_c);
    return YOLO_OK;
}

// one image of a ragged batch: its place in the buffer, its pitch, and what `fit` needs of its size (fit < 0: no fit is asked)
static int image_check(yolo_ctx *c, int i, const yolo_image_desc &d, size_t bytes, int fit)
{
    if (int r = desc_check(c, i, d, bytes)) return r;
    if ((uint64_t)d.w * (uint64_t)c->in_c > 0xffffffffull) return fail(c, YOLO_ERR_INVALID, "image %d: a row of %d pixels of %d bytes does not fit a 32-bit pitch", i, (int)d.w, c->in_c);
    if (fit == YOLO_FIT_LETTERBOX) {
        int nw, nh; letterbox_dims(c->in_w, c->in_h, d.w, d.h, &nw, &nh);
        if (nw < 1 || nh < 1) return fail(c, YOLO_ERR_INVALID, "image %d: %d x %d letterboxes to less than one pixel", i, (int)d.h, (int)d.w);
    }
    if (fit == YOLO_FIT_CENTER_CROP && !resize_min_ok(c->in_w, d.w, d.h))
        return fail(c, YOLO_ERR_INVALID, "image %d: %d x %d: its longer side times the network width %d does not fit an int (darknet's resize_min)", i, (int)d.h, (int)d.w, c->in_w);
    return YOLO_OK;
}

// everything a ragged batch is refused for, before any launch
static int images_check(yolo_ctx *c, const void *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit)
{
    if (int r = need_image(c, "forward of images")) return r;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "forward of images before weights were loaded");
    if (n < 1 || n > c->max_batch) return fail(c, YOLO_ERR_INVALID, "batch %d outside 1..%d", n, c->max_batch);
    if (!pixels || !descs) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    if (int r = fit_check(c, fit, "yolo_*_images_u8 / yolo_detect_images_graph")) return r;
    if (bytes < (size_t)c->in_c || bytes > 0xffffffffull) return fail(c, YOLO_ERR_INVALID, "packed buffer of %zu bytes (%d .. 2^32 - 1)", bytes, c->in_c);
    for (int i = 0; i < n; ++i) if (int r = image_check(c, i, descs[i], bytes, fit)) return r;
    return YOLO_OK;
}

// the centre crop discards part of the image: it is a classifier's fit (and a plain forward's).  The entry points that map results back to the image refuse it
static int crop_fit_refused(yolo_ctx *c, int fit, const char *who, const char *what)
{
    if (fit != YOLO_FIT_CENTER_CROP) return YOLO_OK;
    return fail(c, YOLO_ERR_UNSUPPORTED, "%s: YOLO_FIT_CENTER_CROP is not served: %s cannot be mapped back through a crop that discards part of the image", who, what);
}

static int detect_images_check(yolo_ctx *c, int fit, int max_out, int nms_mode, int select_mode, int units)
{
    if (int r = crop_fit_refused(c, fit, "yolo_detect_images", "boxes")) return r;
    if (int r = post_args_ok(c, max_out, nms_mode, select_mode)) return r;
    if (units != YOLO_UNITS_NETWORK && units != YOLO_UNITS_SOURCE_PIXELS) return fail(c, YOLO_ERR_INVALID, "bad units %d", units);
    if (fit == YOLO_FIT_LETTERBOX)
        for (auto &L : c->layers) if (L.type == L_DETECT) return fail(c, YOLO_ERR_UNSUPPORTED, "letterbox box mapping of a [detection] head (darknet v1 does not letterbox)");
    return YOLO_OK;
}

// the device step of a checked batch: (descriptor upload,) fit, network.  pixels: device memory
static int images_step(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, bool upload, bool lean, float score_thr)
{
    c->lean_thr = score_thr;
    if (upload) HIPCK(c, hipMemcpyAsync(c->d_descs, descs, (size_t)n * sizeof(ImgDesc), hipMemcpyHostToDevice, c->stream));
    auto [dst, dt] = input_fill_dst(c);
    HIPCK(c, launch_fit_images(pixels, bytes, c->d_descs, n, fit, c->in_h, c->in_w, dst, dt, fill_stride(c), c->in_mul, c->in_add, c->stream, c->in_c));
    HIPCK(c, input_filled(c, (size_t)n * c->in_h * c->in_w));
    return run_network(c, n, lean, fit);
}

// the packed buffer on the device: a host buffer is staged with one host-to-device copy (d_pix: grown, never shrunk)
static int stage_pixels(yolo_ctx *c, const uint8_t *pixels, size_t bytes, int loc, const uint8_t **src)
{
    *src = pixels;
    if (loc != YOLO_HOST) return YOLO_OK;
    if (bytes > c->pix_cap) {
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (c->d_pix) HIPCK(c, hipFree(c->d_pix));
        c->d_pix = nullptr; c->pix_cap = 0;
        HIPCK(c, hipMalloc(&c->d_pix, bytes)); c->pix_cap = bytes;
    }
    HIPCK(c, hipMemcpyAsync(c->d_pix, pixels, bytes, hipMemcpyHostToDevice, c->stream));
    *src = (const uint8_t *)c->d_pix;
    return YOLO_OK;
}

static int forward_images_impl(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc,
                               float *det_out, int out_loc, bool lean, float score_thr)
{
    if (int r = images_check(c, pixels, bytes, descs, n, fit)) return r;
    HIPCK(c, hipSetDevice(c->device));
    const uint8_t *src = nullptr;
    if (int r = stage_pixels(c, pixels, bytes, loc, &src)) return r;
    if (int r = images_step(c, src, bytes, descs, n, fit, true, lean && !det_out, score_thr)) return r;
    return det_out ? copy_out(c, det_out, c->d_det, (size_t)n * c->rows * c->attrs * 4, out_loc) : YOLO_OK;
}

int yolo_forward_images_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc,
                           float *det_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    return forward_images_impl(c, pixels, bytes, descs, n, fit, loc, det_out, out_loc, false, 0.f);
}

int yolo_detect_images_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc,
                          float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                          yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = detect_images_check(c, fit, max_out, nms_mode, select_mode, units)) return r;
    if (int r = forward_images_impl(c, pixels, bytes, descs, n, fit, loc, nullptr, YOLO_DEVICE, nms_mode != YOLO_NMS_NUMPY_V3, score_thr)) return r;
    const PostGeom g{fit, units == YOLO_UNITS_SOURCE_PIXELS};
    return postprocess_impl(c, n, score_thr, iou_thr, max_out, nms_mode, select_mode, boxes_out, counts_out, nullptr, out_loc, &g);
}

int yolo_detect_images_graph(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit,
                             float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                             yolo_box *boxes_out, int32_t *counts_out)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!pixels || !boxes_out || !counts_out) return fail(c, YOLO_ERR_INVALID, "yolo_detect_images_graph needs device pointers for pixels, boxes_out and counts_out");
    if (int r = detect_images_check(c, fit, max_out, nms_mode, select_mode, units)) return r;
    if (int r = images_check(c, pixels, bytes, descs, n, fit)) return r;
    GraphKey k; memset(&k, 0, sizeof k);
    k.src = pixels; k.bytes = bytes; k.n = n; k.fit = fit; k.units = units; k.st = score_thr; k.it = iou_thr; k.mo = max_out; k.nm = nms_mode; k.sm = select_mode; k.bo = boxes_out; k.co = counts_out;
    HIPCK(c, hipSetDevice(c->device));
    // this call's sizes and offsets: into the device table, on the context stream, ahead of the step that reads them (never captured)
    HIPCK(c, hipMemcpyAsync(c->d_descs, descs, (size_t)n * sizeof(ImgDesc), hipMemcpyHostToDevice, c->stream));
    const GraphEager eager = [](yolo_ctx *c, const GraphKey &k) -> int {
        if (int r = images_step(c, (const uint8_t *)k.src, k.bytes, nullptr, k.n, k.fit, false, k.nm != YOLO_NMS_NUMPY_V3, k.st)) return r;
        const PostGeom g{k.fit, k.units == YOLO_UNITS_SOURCE_PIXELS};
        return postprocess_impl(c, k.n, k.st, k.it, k.mo, k.nm, k.sm, (yolo_box *)k.bo, (int32_t *)k.co, nullptr, YOLO_DEVICE, &g);
    };
    bool replayed = false;
    if (int r = graph_step(c, c->graph[1], k, eager, &replayed)) return r;
    if (replayed) { c->lean_thr = score_thr; c->stem_u8 = nullptr; forward_done(c, n, nms_mode != YOLO_NMS_NUMPY_V3, nms_mode == YOLO_NMS_NUMPY_V3 ? 1 : 0, fit); }
    return YOLO_OK;
}

// ---- decoded video frames: NV12 / I420 / pitched RGB / BGR surfaces described in place by yolo_frame_desc.  The fit launch reads the frame table
//      and converts while it fits; d_descs receives {plane 0's offset, h, w} of the same frames, so everything behind the fit -- run_network, frame averaging,
//      recurrent state, the box mapping of the postprocess -- is the image path's ----
static_assert(sizeof(FrameDesc) == sizeof(yolo_frame_desc) && offsetof(FrameDesc, pitch) == offsetof(yolo_frame_desc, pitch) && offsetof(FrameDesc, h) == offsetof(yolo_frame_desc, h) &&
              offsetof(FrameDesc, w) == offsetof(yolo_frame_desc, w) && offsetof(FrameDesc, format) == offsetof(yolo_frame_desc, format) && offsetof(FrameDesc, matrix) == offsetof(yolo_frame_desc, matrix),
              "yolo_frame_desc is the frame table's row");
static_assert(PIX_NV12 == YOLO_PIX_NV12 && PIX_I420 == YOLO_PIX_I420 && PIX_RGB24 == YOLO_PIX_RGB24 && PIX_BGR24 == YOLO_PIX_BGR24 && MATRIX_BT601 == YOLO_MATRIX_BT601 &&
              MATRIX_BT709 == YOLO_MATRIX_BT709 && MATRIX_BT601_FULL == YOLO_MATRIX_BT601_FULL && PIX_JPEG_GREY == YOLO_PIX_JPEG_GREY && PIX_JPEG_444 == YOLO_PIX_JPEG_444 &&
              PIX_JPEG_422 == YOLO_PIX_JPEG_422 && PIX_JPEG_420 == YOLO_PIX_JPEG_420 && PIX_JPEG_440 == YOLO_PIX_JPEG_440, "the kernels' format and matrix codes are the public ones");

int yolo_frame_to_rgb_host(const yolo_frame_desc *desc, const uint8_t *pixels, size_t bytes, uint8_t *rgb_out)
{
    if (!desc || !pixels || !rgb_out) { g_op_err = "yolo_frame_to_rgb_host: desc / pixels / rgb_out == NULL"; return YOLO_ERR_INVALID; }
    if (int r = frame_desc_check(*desc, bytes, 0, g_op_err)) { g_op_err = "yolo_frame_to_rgb_host: " + g_op_err; return r; }
    FrameDesc f; memcpy(&f, desc, sizeof f);
    const ColorMatrix m = color_matrix(f.matrix);
    for (int y = 0; y < f.h; ++y)
        for (int x = 0; x < f.w; ++x) {
            unsigned o[3]; int v[3];
            if (pix_is_jpeg(f.format)) jpeg_frame_rgb(f, y, x, [&](unsigned off) { return (int)pixels[off]; }, v);
            else {
                frame_sample_offsets(f, y, x, o);
                if (f.format >= PIX_RGB24) for (int k = 0; k < 3; ++k) v[k] = pixels[o[k]];
                else yuv_to_rgb(m, pixels[o[0]], pixels[o[1]], pixels[o[2]], v);
            }
            uint8_t *q = rgb_out + ((size_t)y * f.w + x) * 3;
            q[0] = (uint8_t)v[0]; q[1] = (uint8_t)v[1]; q[2] = (uint8_t)v[2];
        }
    return YOLO_OK;
}

// one frame of a batch: its descriptor, and what `fit` needs of its size (fit < 0: no fit is asked), as image_check
static int frame_check(yolo_ctx *c, int i, const yolo_frame_desc &d, size_t bytes, int fit)
{
    std::string msg;
    if (int r = frame_desc_check(d, bytes, i, msg)) return fail(c, r, "%s", msg.c_str());
    if (fit == YOLO_FIT_LETTERBOX) {
        int nw, nh; letterbox_dims(c->in_w, c->in_h, d.w, d.h, &nw, &nh);
        if (nw < 1 || nh < 1) return fail(c, YOLO_ERR_INVALID, "frame %d: %d x %d letterboxes to less than one pixel", i, (int)d.h, (int)d.w);
    }
    if (fit == YOLO_FIT_CENTER_CROP && !resize_min_ok(c->in_w, d.w, d.h))
        return fail(c, YOLO_ERR_INVALID, "frame %d: %d x %d: its longer side times the network width %d does not fit an int (darknet's resize_min)", i, (int)d.h, (int)d.w, c->in_w);
    return YOLO_OK;
}

// everything a batch of frames is refused for, before any launch: images_check's list, the frame descriptors, and what a frame cannot mean
static int frames_refusals(yolo_ctx *c, bool have_pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit);
static int frames_check(yolo_ctx *c, const void *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit) { return frames_refusals(c, pixels != nullptr, bytes, descs, n, fit); }
// the same for a buffer of `bytes` bytes that is not read here (have_pixels: the caller holds one) -- the JPEG forms ask before their surface holds anything
static int frames_refusals(yolo_ctx *c, bool have_pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit)
{
    static const char *const who = "yolo_*_frames_u8 / yolo_detect_frames_graph";
    if (int r = need_image(c, "forward of frames")) return r;
    if (c->in_c != 3) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: a network of %d planes ([net] yolo_input=planes) is not served: a frame is an RGB image after its conversion", who, c->in_c);
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "forward of frames before weights were loaded");
    if (n < 1 || n > c->max_batch) return fail(c, YOLO_ERR_INVALID, "batch %d outside 1..%d", n, c->max_batch);
    if (!have_pixels || !descs) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    if (int r = fit_check(c, fit, who)) return r;
    if (fit == YOLO_FIT_CV2_BGR) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: YOLO_FIT_CV2_BGR is not served for frames: a frame's format states its channel order (YOLO_PIX_BGR24 with YOLO_FIT_CV2)", who);
    if (bytes < 1 || bytes > 0xffffffffull) return fail(c, YOLO_ERR_INVALID, "packed buffer of %zu bytes (1 .. 2^32 - 1)", bytes);
    for (int i = 0; i < n; ++i) if (int r = frame_check(c, i, descs[i], bytes, fit)) return r;
    return YOLO_OK;
}

// this call's frame table and the {offset, h, w} table the box mapping reads: onto the device, on the context stream
static int frames_upload(yolo_ctx *c, const yolo_frame_desc *descs, int n)
{
    c->h_geom.resize((size_t)c->max_batch);
    for (int i = 0; i < n; ++i) c->h_geom[i] = ImgDesc{descs[i].offset[0], descs[i].h, descs[i].w};
    HIPCK(c, hipMemcpyAsync(c->d_frames, descs, (size_t)n * sizeof(FrameDesc), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_descs, c->h_geom.data(), (size_t)n * sizeof(ImgDesc), hipMemcpyHostToDevice, c->stream));
    return YOLO_OK;
}

// the device step of a checked batch of frames whose tables are on the device: fit, network.  pixels: device memory
static int frames_step(yolo_ctx *c, const uint8_t *pixels, size_t bytes, int n, int fit, bool lean, float score_thr)
{
    c->lean_thr = score_thr;
    auto [dst, dt] = input_fill_dst(c);
    HIPCK(c, launch_fit_frames(pixels, bytes, c->d_frames, n, fit, c->in_h, c->in_w, dst, dt, fill_stride(c), c->in_mul, c->in_add, c->stream));
    HIPCK(c, input_filled(c, (size_t)n * c->in_h * c->in_w));
    return run_network(c, n, lean, fit);
}

static int forward_frames_impl(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc,
                               float *det_out, int out_loc, bool lean, float score_thr)
{
    if (int r = frames_check(c, pixels, bytes, descs, n, fit)) return r;
    HIPCK(c, hipSetDevice(c->device));
    const uint8_t *src = nullptr;
    if (int r = stage_pixels(c, pixels, bytes, loc, &src)) return r;
    if (int r = frames_upload(c, descs, n)) return r;
    if (int r = frames_step(c, src, bytes, n, fit, lean && !det_out, score_thr)) return r;
    return det_out ? copy_out(c, det_out, c->d_det, (size_t)n * c->rows * c->attrs * 4, out_loc) : YOLO_OK;
}

int yolo_forward_frames_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc,
                           float *det_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    return forward_frames_impl(c, pixels, bytes, descs, n, fit, loc, det_out, out_loc, false, 0.f);
}

int yolo_detect_frames_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc,
                          float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                          yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = detect_images_check(c, fit, max_out, nms_mode, select_mode, units)) return r;
    if (int r = forward_frames_impl(c, pixels, bytes, descs, n, fit, loc, nullptr, YOLO_DEVICE, nms_mode != YOLO_NMS_NUMPY_V3, score_thr)) return r;
    const PostGeom g{fit, units == YOLO_UNITS_SOURCE_PIXELS};
    return postprocess_impl(c, n, score_thr, iou_thr, max_out, nms_mode, select_mode, boxes_out, counts_out, nullptr, out_loc, &g);
}

int yolo_detect_frames_graph(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit,
                             float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int units,
                             yolo_box *boxes_out, int32_t *counts_out)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!pixels || !boxes_out || !counts_out) return fail(c, YOLO_ERR_INVALID, "yolo_detect_frames_graph needs device pointers for pixels, boxes_out and counts_out");
    if (int r = detect_images_check(c, fit, max_out, nms_mode, select_mode, units)) return r;
    if (int r = frames_check(c, pixels, bytes, descs, n, fit)) return r;
    GraphKey k; memset(&k, 0, sizeof k);
    k.src = pixels; k.bytes = bytes; k.n = n; k.fit = fit; k.units = units; k.st = score_thr; k.it = iou_thr; k.mo = max_out; k.nm = nms_mode; k.sm = select_mode; k.bo = boxes_out; k.co = counts_out;
    HIPCK(c, hipSetDevice(c->device));
    // this call's frames: into the device tables, on the context stream, ahead of the step that reads them (never captured)
    if (int r = frames_upload(c, descs, n)) return r;
    const GraphEager eager = [](yolo_ctx *c, const GraphKey &k) -> int {
        if (int r = frames_step(c, (const uint8_t *)k.src, k.bytes, k.n, k.fit, k.nm != YOLO_NMS_NUMPY_V3, k.st)) return r;
        const PostGeom g{k.fit, k.units == YOLO_UNITS_SOURCE_PIXELS};
        return postprocess_impl(c, k.n, k.st, k.it, k.mo, k.nm, k.sm, (yolo_box *)k.bo, (int32_t *)k.co, nullptr, YOLO_DEVICE, &g);
    };
    bool replayed = false;
    if (int r = graph_step(c, c->graph[2], k, eager, &replayed)) return r;
    if (replayed) { c->lean_thr = score_thr; c->stem_u8 = nullptr; forward_done(c, n, nms_mode != YOLO_NMS_NUMPY_V3, nms_mode == YOLO_NMS_NUMPY_V3 ? 1 : 0, fit); }
    return YOLO_OK;
}

// ---- tiled detection of images larger than the network input ("Tiled detection"): the window grid, then per chunk of max_batch windows one
//      fit launch over the window table + the network + the cross-window merge, and ONE k_nms_image launch over every image's merged list ----
namespace {
// one axis of the grid: image extent L, tile extent T, overlap O
struct TileAxis {
    int L, T, S, n;
    TileAxis(int L_, int T_, int O) : L(L_), T(T_), S(T_ - O), n(L_ <= T_ ? 1 : (int)(((long long)L_ - T_ + S - 1) / S) + 1) {}
    int start(int k) const { return L <= T ? 0 : (int)std::min<long long>((long long)k * S, L - T); }
    int extent() const { return L <= T ? L : T; }
};
bool tile_args_ok(int img_h, int img_w, int tile_h, int tile_w, int overlap_h, int overlap_w)
{
    return img_h >= 1 && img_w >= 1 && tile_h >= 1 && tile_w >= 1 && overlap_h >= 0 && overlap_w >= 0 && overlap_h < tile_h && overlap_w < tile_w;
}
// the carving of yolo_ctx::d_tile for a call of `images` images, `nwin` windows, `cap` merged rows per image and max_out records: every array 256-byte aligned
struct TileSlab {
    WinDesc *wins; ImgDesc *descs; unsigned long long *overflow; float *scores; int *labels; float4 *box; int *cand; unsigned long long *keys; float4 *sbox; int *slabel; float *sscore;
    yolo_box *boxes; int *counts, *wcount, *run[2], *total; FrameDesc *frames; size_t bytes, nan_fill;      // nan_fill: bytes from `overflow` to the end of `scores`, set to all ones before the first step
    TileSlab(char *base, size_t images, size_t nwin, size_t cap, size_t pow2, size_t max_out, size_t max_batch, size_t nframes)      // nframes: rows of the frame table (yolo_detect_tiled_frames_u8), 0 for images
    {
        size_t off = 0;
        auto take = [&](size_t n) { const uintptr_t p = (uintptr_t)base + off; off += (n + 255) & ~(size_t)255; return (void *)p; };      // (base == nullptr: the sizes only)
        wins = (WinDesc *)take(nwin * sizeof(WinDesc)); descs = (ImgDesc *)take(images * sizeof(ImgDesc));
        overflow = (unsigned long long *)take(8); scores = (float *)take(images * cap * 4); nan_fill = (size_t)((char *)scores - (char *)overflow) + images * cap * 4;
        labels = (int *)take(images * cap * 4); box = (float4 *)take(images * cap * 16); cand = (int *)take(images * cap * 4); keys = (unsigned long long *)take(images * pow2 * 8);
        sbox = (float4 *)take(images * cap * 16); slabel = (int *)take(images * cap * 4); sscore = (float *)take(images * cap * 4);
        boxes = (yolo_box *)take(images * max_out * sizeof(yolo_box)); counts = (int *)take(images * 4); wcount = (int *)take(max_batch * 4);
        run[0] = (int *)take(images * 4); run[1] = (int *)take(images * 4); total = (int *)take(images * 4);
        frames = (FrameDesc *)take(nframes * sizeof(FrameDesc));
        bytes = off;
    }
};
struct StreamDrain { yolo_ctx *c; ~StreamDrain() { hipStreamSynchronize(c->stream); } };      // host tables handed to asynchronous copies outlive them on every return path
}

int yolo_tile_windows(int img_h, int img_w, int tile_h, int tile_w, int overlap_h, int overlap_w, yolo_tile_window *out, int cap, int *count)
{
    if (!count) { g_op_err = "yolo_tile_windows: count == NULL"; return YOLO_ERR_INVALID; }
    *count = 0;
    if (!tile_args_ok(img_h, img_w, tile_h, tile_w, overlap_h, overlap_w) || cap < 0 || (cap > 0 && !out)) {
        g_op_err = "yolo_tile_windows: image, tile extents >= 1 and 0 <= overlap < tile are needed (and out for cap > 0)"; return YOLO_ERR_INVALID;
    }
    const TileAxis ay(img_h, tile_h, overlap_h), ax(img_w, tile_w, overlap_w);
    if ((long long)ay.n * ax.n > 0x7fffffffLL) { g_op_err = "yolo_tile_windows: 2^31 windows or more"; return YOLO_ERR_INVALID; }
    *count = ay.n * ax.n;
    for (int k = 0; k < std::min(cap, *count); ++k) out[k] = yolo_tile_window{ay.start(k / ax.n), ax.start(k % ax.n), ay.extent(), ax.extent()};
    return YOLO_OK;
}

static int frame_check(yolo_ctx *c, int i, const yolo_frame_desc &d, size_t bytes, int fit);

// what tiled_refusals leaves for the device part: the window table, {plane 0's offset, h, w} of every frame (frames only: what the relative form divides by),
// the windows of the image that has the most
struct TiledWindows { std::vector<WinDesc> wins; std::vector<yolo_image_desc> geom; int most = 0; };

// Every refusal of tiled detection, and the window table: no device work.  `bytes`: the size of the packed buffer the windows will be cut from -- the buffer
// itself is not read, so yolo_detect_tiled_jpegs asks before its surface holds anything
static int tiled_refusals(yolo_ctx *c, const char *who, size_t bytes, const yolo_image_desc *descs, const yolo_frame_desc *frames, int n_images, int tile_h, int tile_w,
                          int overlap_h, int overlap_w, int fit, int max_out, int nms_mode, int select_mode, int relative, const void *boxes_out, const void *counts_out,
                          TiledWindows &out)
{
    std::vector<WinDesc> &wins = out.wins;
    std::vector<yolo_image_desc> &geom = out.geom;
    int &most = out.most;
    wins.clear(); geom.clear(); most = 0;
    if (int r = need_detector(c, who)) return r;
    if (c->in_c != 3) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: a network of %d planes ([net] yolo_input=planes) is not served: windows are cut from RGB images", who, c->in_c);
    if (frames && fit == YOLO_FIT_CV2_BGR) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: YOLO_FIT_CV2_BGR is not served for frames: a frame's format states its channel order", who);
    if (c->avg_k > 1) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: not served while frame averaging is on (yolo_set_frame_average(%d)): a batch slot holds a window, not a stream; set it to 1 first", who, c->avg_k);
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "%s before weights were loaded", who);
    static const char *const fit_names[] = {"YOLO_FIT_STRETCH", "YOLO_FIT_LETTERBOX", "YOLO_FIT_CV2", "YOLO_FIT_CV2_BGR", "YOLO_FIT_CENTER_CROP"};
    if (fit < YOLO_FIT_STRETCH || fit > YOLO_FIT_CENTER_CROP) return fail(c, YOLO_ERR_INVALID, "bad fit %d", fit);
    if (fit != YOLO_FIT_STRETCH && fit != YOLO_FIT_LETTERBOX)
        return fail(c, YOLO_ERR_UNSUPPORTED, "%s: %s is not served: a window is fitted by YOLO_FIT_STRETCH or YOLO_FIT_LETTERBOX", who, fit_names[fit]);
    if (int r = post_args_ok(c, max_out, nms_mode, select_mode)) return r;
    if (nms_mode != YOLO_NMS_TF && nms_mode != YOLO_NMS_DARKNET)
        return fail(c, YOLO_ERR_UNSUPPORTED, "%s: %s is not served: the merged candidates of an image go through YOLO_NMS_TF or YOLO_NMS_DARKNET", who,
                    nms_mode == YOLO_NMS_PER_CLASS ? "YOLO_NMS_PER_CLASS" : nms_mode == YOLO_NMS_TF_V1 ? "YOLO_NMS_TF_V1" : "YOLO_NMS_NUMPY_V3");
    if (c->tree_head >= 0) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: a softmax-tree head is not served", who);
    if (fit == YOLO_FIT_LETTERBOX)
        for (auto &L : c->layers) if (L.type == L_DETECT) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: letterbox box mapping of a [detection] head (darknet v1 does not letterbox)", who);
    if (relative != 0 && relative != 1) return fail(c, YOLO_ERR_INVALID, "bad relative %d", relative);
    if (!boxes_out || !counts_out) return fail(c, YOLO_ERR_INVALID, "boxes_out / counts_out == NULL");
    if (n_images < 1) return fail(c, YOLO_ERR_INVALID, "%d images", n_images);
    if (!descs && !frames) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    if (bytes < 3 || bytes > 0xffffffffull) return fail(c, YOLO_ERR_INVALID, "packed buffer of %zu bytes (3 .. 2^32 - 1)", bytes);
    if (tile_h == 0 && tile_w == 0) { tile_h = c->in_h; tile_w = c->in_w; }
    if (!tile_args_ok(1, 1, tile_h, tile_w, overlap_h, overlap_w))
        return fail(c, YOLO_ERR_INVALID, "%s: tile %d x %d with overlap %d x %d: extents >= 1 and 0 <= overlap < tile are needed", who, tile_h, tile_w, overlap_h, overlap_w);
    try {
        if (frames) {
            for (int i = 0; i < n_images; ++i) {
                if (int r = frame_check(c, i, frames[i], bytes, -1)) return r;
                geom.push_back(yolo_image_desc{frames[i].offset[0], frames[i].h, frames[i].w});
            }
            descs = geom.data();
        }
        for (int i = 0; i < n_images; ++i) {
            const yolo_image_desc &d = descs[i];
            if (!frames) if (int r = desc_check(c, i, d, bytes)) return r;
            if ((uint64_t)d.w * 3u > 0x7fffffffull) return fail(c, YOLO_ERR_INVALID, "image %d: a row of %d pixels does not fit a 32-bit pitch", i, (int)d.w);
            const TileAxis ay(d.h, tile_h, overlap_h), ax(d.w, tile_w, overlap_w);
            if ((long long)ay.n * ax.n + (long long)wins.size() > 0x7fffffffLL) return fail(c, YOLO_ERR_INVALID, "image %d: 2^31 windows or more", i);
            most = std::max(most, ay.n * ax.n);
            for (int k = 0; k < ay.n * ax.n; ++k) {
                WinDesc w; w.y0 = ay.start(k / ax.n); w.x0 = ax.start(k % ax.n); w.h = ay.extent(); w.w = ax.extent(); w.pitch = d.w * 3; w.image = i;
                w.offset = d.offset + (uint64_t)w.y0 * (uint64_t)w.pitch + (uint64_t)w.x0 * 3u;
                if (frames) { w.offset = 0; w.pitch = 0; }          // a frame's window is (y0, x0, h, w) of frame `image`: the fit reads the frame table
                if (fit == YOLO_FIT_LETTERBOX) {
                    int nw, nh; letterbox_dims(c->in_w, c->in_h, w.w, w.h, &nw, &nh);
                    if (nw < 1 || nh < 1) return fail(c, YOLO_ERR_INVALID, "image %d: its %d x %d window letterboxes to less than one pixel", i, w.h, w.w);
                }
                wins.push_back(w);
            }
        }
    } catch (const std::bad_alloc &) { return fail(c, YOLO_ERR_NOMEM, "%s: the window table", who); }
    return YOLO_OK;
}

// the device part of tiled detection over a window table that passed tiled_refusals: pixels[bytes] holds the images (descs) or the frames (frames, descs == NULL)
static int tiled_run(yolo_ctx *c, const char *who, const TiledWindows &tw, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, const yolo_frame_desc *frames,
                     int n_images, int fit, int loc, float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative, yolo_box *boxes_out,
                     int32_t *counts_out, int out_loc)
{
    if (!pixels) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    const std::vector<WinDesc> &wins = tw.wins;
    const int most = tw.most;
    if (frames) descs = tw.geom.data();
    const int nwin = (int)wins.size();
    const size_t cap = (size_t)std::min<long long>(TILE_MERGE_CAP, (long long)most * c->rows);
    size_t pow2 = 1; while (pow2 < cap) pow2 <<= 1;
    const TileSlab need(nullptr, n_images, nwin, cap, pow2, max_out, c->max_batch, frames ? n_images : 0);

    // ---- device ----
    HIPCK(c, hipSetDevice(c->device));
    const uint8_t *src = nullptr;
    if (int r = stage_pixels(c, pixels, bytes, loc, &src)) return r;
    if (need.bytes > c->tile_cap) {
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (c->d_tile) HIPCK(c, hipFree(c->d_tile));
        c->d_tile = nullptr; c->tile_cap = 0;
        HIPCK(c, hipMalloc(&c->d_tile, need.bytes)); c->tile_cap = need.bytes;
    }
    const TileSlab t((char *)c->d_tile, n_images, nwin, cap, pow2, max_out, c->max_batch, frames ? n_images : 0);
    StreamDrain drain{c};
    HIPCK(c, hipMemcpyAsync(t.wins, wins.data(), (size_t)nwin * sizeof(WinDesc), hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipMemcpyAsync(t.descs, descs, (size_t)n_images * sizeof(ImgDesc), hipMemcpyHostToDevice, c->stream));
    if (frames) HIPCK(c, hipMemcpyAsync(t.frames, frames, (size_t)n_images * sizeof(FrameDesc), hipMemcpyHostToDevice, c->stream));
    // the overflow word starts as all ones; so does every merged score: a NaN, which neither `>` nor `>=` lets through the NMS's own threshold
    HIPCK(c, hipMemsetAsync(t.overflow, 0xff, t.nan_fill, c->stream));
    c->lean_thr = score_thr;
    TileMergeArgs m; memset(&m, 0, sizeof m);
    m.wins = t.wins; m.nwin = nwin; m.rows = c->rows; m.attrs = c->attrs; m.scores = c->d_scores; m.labels = c->d_labels; m.score_thr = score_thr; m.select_mode = select_mode;
    m.fit = fit; m.netw = c->in_w; m.neth = c->in_h; m.centre = nms_mode == YOLO_NMS_DARKNET; m.cap = (int)cap;
    m.net_pixels = c->decode == YOLO_DECODE_PIXEL;          // [region] / [detection] heads always decode normalised boxes
    for (auto &L : c->layers) if (L.type == L_REGION || L.type == L_DETECT) m.net_pixels = 0;
    m.m_scores = t.scores; m.m_labels = t.labels; m.m_box = t.box; m.wcount = t.wcount; m.total = t.total; m.overflow = t.overflow;
    for (int first = 0, step = 0; first < nwin; first += c->max_batch, ++step) {
        const int nb = std::min(c->max_batch, nwin - first);
        auto [dst, dt] = input_fill_dst(c);
        if (frames) HIPCK(c, launch_fit_frame_windows(src, bytes, t.frames, t.wins + first, nb, fit, c->in_h, c->in_w, dst, dt, 8, c->in_mul, c->in_add, c->stream));
        else HIPCK(c, launch_fit_windows(src, bytes, t.wins + first, nb, fit, c->in_h, c->in_w, dst, dt, 8, c->in_mul, c->in_add, c->stream));
        HIPCK(c, input_filled(c, (size_t)nb * c->in_h * c->in_w));
        if (int r = run_network(c, nb, true)) return r;
        m.first = first; m.nb = nb; m.det = c->d_det; m.box4 = c->det_valid ? nullptr : c->d_box4;
        m.run_in = t.run[step & 1]; m.run_out = t.run[(step + 1) & 1];
        HIPCK(c, launch_tile_merge(m, c->stream));
    }
    // one NMS launch over the merged lists: rows that hold the box in the form the flavour reads, scores and labels beside them
    PostArgs p; memset(&p, 0, sizeof p);
    p.box4 = (const float *)t.box; p.n = n_images; p.rows = (int)cap; p.attrs = 4; p.score_thr = score_thr; p.iou_thr = iou_thr; p.max_out = max_out;
    p.nms_mode = nms_mode; p.select_mode = select_mode; p.scores_ready = 1; p.corners_in = 1;
    p.scores = t.scores; p.labels = t.labels; p.cand = t.cand; p.keys = t.keys; p.rows_pow2 = (int)pow2; p.sbox = t.sbox; p.slabel = t.slabel; p.sscore = t.sscore;
    p.boxes_out = t.boxes; p.counts_out = t.counts;
    if (c->lean_cnt_dirty) p.zero_word = c->d_lean_cnt;
    HIPCK(c, launch_postprocess(p, c->stream));
    c->lean_cnt_dirty = false;
    if (relative) HIPCK(c, launch_tile_relative(t.boxes, t.counts, max_out, t.descs, n_images, c->stream));
    unsigned long long over = 0;
    if (int r = copy_out(c, &over, t.overflow, 8, YOLO_HOST)) return r;          // (synchronises)
    if (over != ~0ull)
        return fail(c, YOLO_ERR_UNSUPPORTED, "%s: image %u yields %u candidates above the score threshold, more than the %zu one NMS launch serves; raise score_thr or enlarge the tile",
                    who, (unsigned)(over >> 32), (unsigned)(over & 0xffffffffu), cap);
    if (int r = copy_out(c, boxes_out, t.boxes, (size_t)n_images * max_out * sizeof(yolo_box), out_loc)) return r;
    return copy_out(c, counts_out, t.counts, (size_t)n_images * 4, out_loc);
}

// yolo_detect_tiled_u8 (descs: packed RGB images) and yolo_detect_tiled_frames_u8 (frames: decoded video frames, descs == NULL): the same steps over windows of either
static int detect_tiled_impl(yolo_ctx *c, const char *who, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, const yolo_frame_desc *frames, int n_images,
                             int tile_h, int tile_w, int overlap_h, int overlap_w, int fit, int loc, float score_thr, float iou_thr, int max_out, int nms_mode,
                             int select_mode, int relative, yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    TiledWindows tw;
    if (int r = tiled_refusals(c, who, bytes, descs, frames, n_images, tile_h, tile_w, overlap_h, overlap_w, fit, max_out, nms_mode, select_mode, relative, boxes_out, counts_out, tw)) return r;
    return tiled_run(c, who, tw, pixels, bytes, descs, frames, n_images, fit, loc, score_thr, iou_thr, max_out, nms_mode, select_mode, relative, boxes_out, counts_out, out_loc);
}

int yolo_detect_tiled_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n_images, int tile_h, int tile_w, int overlap_h,
                         int overlap_w, int fit, int loc, float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative,
                         yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    return detect_tiled_impl(c, "yolo_detect_tiled_u8", pixels, bytes, descs, nullptr, n_images, tile_h, tile_w, overlap_h, overlap_w, fit, loc, score_thr, iou_thr, max_out,
                             nms_mode, select_mode, relative, boxes_out, counts_out, out_loc);
}

int yolo_detect_tiled_frames_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n_images, int tile_h, int tile_w, int overlap_h,
                                int overlap_w, int fit, int loc, float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative,
                                yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (c && !descs) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    return detect_tiled_impl(c, "yolo_detect_tiled_frames_u8", pixels, bytes, nullptr, descs, n_images, tile_h, tile_w, overlap_h, overlap_w, fit, loc, score_thr, iou_thr, max_out,
                             nms_mode, select_mode, relative, boxes_out, counts_out, out_loc);
}

// ---- JPEG files: host entropy stage (yolo_jpeg.cpp) -> one upload -> one IDCT launch (jpeg_ops.hip) -> a frame table over the context's surface,
//      which the frames entry points above read as they read any frame ----
}  // extern "C"
namespace yolo_impl {

// where a parsed file's planes lie in a surface that has `surface` bytes in front of them, and its blocks in a coefficient array that has `block` blocks: the
// frame descriptor, the IDCT's table rows (f.comps of them), the surface's and the array's new ends.  Planes begin at multiples of 256 bytes
void jpeg_place(const JpegFile &f, size_t &surface, size_t &block, yolo_frame_desc *desc, JpegPlane *rows)
{
    memset(desc, 0, sizeof *desc);
    desc->h = f.h; desc->w = f.w; desc->format = f.format; desc->matrix = 0;
    for (int p = 0; p < f.comps; ++p) {
        surface = (surface + 255) & ~(size_t)255;
        desc->offset[p] = surface; desc->pitch[p] = (uint64_t)f.bw[p] * 8;
        rows[p] = JpegPlane{(unsigned)(block + f.block0[p]), (unsigned)f.bw[p], (unsigned)surface, (unsigned)f.bw[p] * 8u};
        surface += (size_t)f.bw[p] * 8 * (size_t)f.bh[p] * 8;
    }
    block += f.blocks;
}

// the whole decode of one parsed file on the host: entropy stage, the IDCT of every block into a surface, the frame rule over it
static int jpeg_to_rgb_host(const uint8_t *file, size_t bytes, const JpegFile &f, uint8_t *rgb_out, std::string &msg)
{
    yolo_frame_desc d; JpegPlane rows[3]; size_t surface = 0, block = 0;
    jpeg_place(f, surface, block, &d, rows);
    std::vector<int16_t> coef; std::vector<uint8_t> planes;
    try { coef.resize(f.blocks * 64); planes.resize(surface); } catch (const std::bad_alloc &) { msg = "file 0: no memory for its " + std::to_string(f.blocks) + " blocks"; return YOLO_ERR_NOMEM; }
    if (int r = jpeg_decode(file, bytes, 0, f, coef.data(), msg)) return r;
    for (int p = 0; p < f.comps; ++p)
        for (size_t i = 0; i < (size_t)f.bw[p] * f.bh[p]; ++i)
            jpeg_idct_block(coef.data() + (f.block0[p] + i) * 64, planes.data() + rows[p].offset + (i / f.bw[p]) * 8 * rows[p].pitch + (i % f.bw[p]) * 8, rows[p].pitch);
    return yolo_frame_to_rgb_host(&d, planes.data(), planes.size(), rgb_out);
}

// headers and layout of a batch, into c->jpeg: no device work.  view_bytes: the surface's capacity once this batch fits it
static int jpegs_plan(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n)
{
    if (!files || !bytes) return fail(c, YOLO_ERR_INVALID, "files / bytes == NULL");
    if (n < 1 || n > 65536) return fail(c, YOLO_ERR_INVALID, "%d files (1 .. 65536)", n);
    yolo_ctx::JpegBatch &J = c->jpeg;
    try { J.files.resize((size_t)n); J.descs.resize((size_t)n); J.planes.clear(); J.planes.reserve(3 * (size_t)n); J.first_block.resize((size_t)n); }
    catch (const std::bad_alloc &) { return fail(c, YOLO_ERR_NOMEM, "the table of %d files", n); }
    J.blocks = 0; J.surface = 0;
    std::string msg;
    for (int i = 0; i < n; ++i) {
        if (int r = jpeg_parse(files[i], bytes[i], i, &J.files[i], msg)) return fail(c, r, "%s", msg.c_str());
        JpegPlane rows[3];
        J.first_block[i] = J.blocks;
        jpeg_place(J.files[i], J.surface, J.blocks, &J.descs[i], rows);
        for (int p = 0; p < J.files[i].comps; ++p) J.planes.push_back(rows[p]);
        if (J.surface > 0xffffffffull || J.blocks > 0xfffffff0ull) return fail(c, YOLO_ERR_UNSUPPORTED, "file %d: the component planes of files 0 .. %d pass 2^32 - 1 bytes; decode fewer files per call", i, i);
    }
    const size_t step = (size_t)4 << 20;
    J.view_bytes = std::max(c->jpeg_cap, std::min<size_t>((J.surface + step - 1) / step * step, 0xffffffffull));
    return YOLO_OK;
}

// what every decode needs before its entropy stage: the staging of {plane table, coefficients} and its device copy (`need` bytes), the surface, the events; the
// plane table at the staging's head
static int jpegs_buffers(yolo_ctx *c, size_t need)
{
    yolo_ctx::JpegBatch &J = c->jpeg;
    if (c->jpeg_up_pending) { HIPCK(c, hipEventSynchronize(c->jpeg_up)); c->jpeg_up_pending = false; }          // the staging is free again
    if (need > c->jin_cap || J.view_bytes > c->jpeg_cap) HIPCK(c, hipStreamSynchronize(c->stream));             // nothing in flight reads what moves
    if (need > c->jin_cap) {
        if (c->h_jin) HIPCK(c, hipHostFree(c->h_jin));
        if (c->d_jin) HIPCK(c, hipFree(c->d_jin));
        c->h_jin = c->d_jin = nullptr; c->jin_cap = 0;
        const size_t cap = need + need / 4;
        HIPCK(c, hipHostMalloc(&c->h_jin, cap, hipHostMallocDefault));
        HIPCK(c, hipMalloc(&c->d_jin, cap));
        c->jin_cap = cap;
    }
    if (J.view_bytes > c->jpeg_cap) {
        if (c->d_jpeg) HIPCK(c, hipFree(c->d_jpeg));
        c->d_jpeg = nullptr; c->jpeg_cap = 0;
        HIPCK(c, hipMalloc((void **)&c->d_jpeg, J.view_bytes));
        c->jpeg_cap = J.view_bytes;
    }
    if (!c->jpeg_up) HIPCK(c, hipEventCreateWithFlags(&c->jpeg_up, hipEventDisableTiming));
    if (!c->jpeg_t[0]) for (auto &ev : c->jpeg_t) HIPCK(c, hipEventCreate(&ev));
    memcpy(c->h_jin, J.planes.data(), J.planes.size() * sizeof(JpegPlane));
    return YOLO_OK;
}

// YOLO_JPEG_ENTROPY_AUTO with at least one eligible file (c->jpeg_iv[i] non-empty: file i's intervals).  The others go through the host stage into their ranges of
// the staging; the eligible ones are decoded by k_jpeg_entropy into theirs of the device array; one IDCT launch; the status words come back and are waited for.
// A file with a non-zero word is decoded again by the host stage, whose verdict stands
static int jpegs_run_device(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n)
{
    yolo_ctx::JpegBatch &J = c->jpeg;
    JpegEntropyPlan &P = c->jent;
    const size_t table = (J.planes.size() * sizeof(JpegPlane) + 255) & ~(size_t)255, need = table + J.blocks * 128;
    if (int r = jpegs_buffers(c, need)) return r;
    std::vector<int> host, dev;
    try {
        P.clear();
        for (int i = 0; i < n; ++i)
            if (c->jpeg_iv[i].empty()) host.push_back(i);
            else { dev.push_back(i); P.add(J.files[i], bytes[i], c->jpeg_iv[i], J.first_block[i]); }
    } catch (const std::bad_alloc &) { return fail(c, YOLO_ERR_NOMEM, "the interval table of %d files", n); }
    const size_t slots = P.iv.size(), at_wg = (P.files.size() * sizeof(JpegDevFile) + 15) & ~(size_t)15, at_iv = (at_wg + P.wg_file.size() * 4 + 15) & ~(size_t)15,
                 at_status = at_iv + slots * sizeof(JpegInterval), jst = at_status + slots * 4;
    if (slots > 0x7fffffc0ull) return fail(c, YOLO_ERR_UNSUPPORTED, "%zu restart intervals in one batch; decode fewer files per call", slots);
    if (jst > c->jst_cap || P.stream_bytes > c->jstream_cap) HIPCK(c, hipStreamSynchronize(c->stream));
    if (jst > c->jst_cap) {
        if (c->h_jst) HIPCK(c, hipHostFree(c->h_jst));
        if (c->d_jst) HIPCK(c, hipFree(c->d_jst));
        c->h_jst = c->d_jst = nullptr; c->jst_cap = 0;
        const size_t cap = jst + jst / 4;
        HIPCK(c, hipHostMalloc(&c->h_jst, cap, hipHostMallocDefault));
        HIPCK(c, hipMalloc(&c->d_jst, cap));
        c->jst_cap = cap;
    }
    if (P.stream_bytes > c->jstream_cap) {
        if (c->d_jstream) HIPCK(c, hipFree(c->d_jstream));
        c->d_jstream = nullptr; c->jstream_cap = 0;
        const size_t cap = P.stream_bytes + P.stream_bytes / 4;
        HIPCK(c, hipMalloc((void **)&c->d_jstream, cap));
        c->jstream_cap = cap;
    }
    memcpy(c->h_jst, P.files.data(), P.files.size() * sizeof(JpegDevFile));
    memcpy((char *)c->h_jst + at_wg, P.wg_file.data(), P.wg_file.size() * 4);
    memcpy((char *)c->h_jst + at_iv, P.iv.data(), slots * sizeof(JpegInterval));
    int16_t *const h_coef = (int16_t *)((char *)c->h_jin + table), *const d_coef = (int16_t *)((char *)c->d_jin + table);
    std::string msg;
    const auto t0 = std::chrono::steady_clock::now();
    if (!host.empty() && jpeg_decode_some(files, bytes, host.data(), (int)host.size(), J.files.data(), J.first_block.data(), h_coef, msg)) {
        // the batch has a malformed file: the verdict is the host stage's over the WHOLE batch, which names the lowest index that fails
        const int r = jpeg_decode_batch(files, bytes, n, J.files.data(), J.first_block.data(), h_coef, msg);
        return fail(c, r ? r : YOLO_ERR_INVALID, "%s", msg.c_str());
    }
    c->jpeg_entropy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // files i .. j - 1 of a list that are neighbours in the batch share one copy of their blocks
    const auto runs = [&](const std::vector<int> &list, const auto &each) -> hipError_t {
        for (size_t i = 0; i < list.size();) {
            size_t j = i + 1;
            while (j < list.size() && list[j] == list[j - 1] + 1) ++j;
            const size_t b0 = J.first_block[list[i]], b1 = J.first_block[list[j - 1]] + J.files[list[j - 1]].blocks;
            if (hipError_t e = each(b0 * 64, (b1 - b0) * 128)) return e;
            i = j;
        }
        return hipSuccess;
    };
    size_t up = table + jst - slots * 4 + P.stream_bytes;
    for (int i : host) up += J.files[i].blocks * 128;
    c->jpeg_upload_bytes = up;
    HIPCK(c, hipEventRecord(c->jpeg_t[0], c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_jin, c->h_jin, table, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, runs(host, [&](size_t at, size_t len) { return hipMemcpyAsync(d_coef + at, h_coef + at, len, hipMemcpyHostToDevice, c->stream); }));
    HIPCK(c, hipMemcpyAsync(c->d_jst, c->h_jst, at_status, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_up, c->stream));
    c->jpeg_up_pending = true;
    // (the files' bytes come from the caller's pageable memory: the runtime stages them, and the call waits for the stream below before it returns)
    for (size_t k = 0; k < dev.size(); ++k) HIPCK(c, hipMemcpyAsync(c->d_jstream + P.files[k].stream0, files[dev[k]], bytes[dev[k]], hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_t[1], c->stream));
    uint32_t *const d_status = (uint32_t *)((char *)c->d_jst + at_status);
    const uint32_t *const h_status = (const uint32_t *)((const char *)c->h_jst + at_status);
    HIPCK(c, launch_jpeg_entropy(c->d_jstream, c->jstream_cap, (const JpegDevFile *)c->d_jst, (int)P.files.size(), (const uint32_t *)((const char *)c->d_jst + at_wg),
                                 (const JpegInterval *)((const char *)c->d_jst + at_iv), slots, d_coef, J.blocks, d_status, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_t[3], c->stream));
    HIPCK(c, launch_jpeg_idct(d_coef, (const JpegPlane *)c->d_jin, (int)J.planes.size(), J.blocks, c->d_jpeg, c->jpeg_cap, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_t[2], c->stream));
    HIPCK(c, hipMemcpyAsync((char *)c->h_jst + at_status, d_status, slots * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    c->jpeg_up_pending = false;
    c->je_dev_files = (int)dev.size(); c->je_host_files = (int)host.size(); c->je_stream_bytes = P.stream_bytes;
    std::vector<int> again;
    for (size_t k = 0; k < dev.size(); ++k) {
        bool clean = true;
        for (size_t i = P.first_slot[k]; clean && i < P.first_slot[k + 1]; ++i) clean = h_status[i] == 0;
        if (clean) c->je_intervals += (int)c->jpeg_iv[dev[k]].size(); else again.push_back(dev[k]);          // (a file handed back counts as the host's, its intervals too)
    }
    if (again.empty()) return YOLO_OK;
    // failed or doubtful intervals: those files again, in full, by the host stage -- served, or refused in its words --, and the IDCT again over the batch
    if (int r = jpeg_decode_some(files, bytes, again.data(), (int)again.size(), J.files.data(), J.first_block.data(), h_coef, msg)) return fail(c, r, "%s", msg.c_str());
    HIPCK(c, runs(again, [&](size_t at, size_t len) { return hipMemcpyAsync(d_coef + at, h_coef + at, len, hipMemcpyHostToDevice, c->stream); }));
    HIPCK(c, hipEventRecord(c->jpeg_up, c->stream));
    c->jpeg_up_pending = true;
    HIPCK(c, launch_jpeg_idct(d_coef, (const JpegPlane *)c->d_jin, (int)J.planes.size(), J.blocks, c->d_jpeg, c->jpeg_cap, c->stream));
    c->je_dev_files -= (int)again.size(); c->je_host_files += (int)again.size();
    return YOLO_OK;
}

// the planned batch onto the device: buffers, entropy stage into pinned memory, one upload, one launch
static int jpegs_run(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n)
{
    yolo_ctx::JpegBatch &J = c->jpeg;
    HIPCK(c, hipSetDevice(c->device));
    c->je_dev_files = 0; c->je_host_files = n; c->je_intervals = 0; c->je_scan_ms = 0; c->je_stream_bytes = 0;
    if (c->jpeg_entropy_mode == YOLO_JPEG_ENTROPY_AUTO) {
        const auto t0 = std::chrono::steady_clock::now();
        bool any = false;
        try {
            c->jpeg_iv.resize((size_t)n);
            for (int i = 0; i < n; ++i) any |= jpeg_intervals(files[i], bytes[i], J.files[i], c->jpeg_iv[i]);
        } catch (const std::bad_alloc &) { return fail(c, YOLO_ERR_NOMEM, "the interval table of %d files", n); }
        c->je_scan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (any) return jpegs_run_device(c, files, bytes, n);
    }
    const size_t table = (J.planes.size() * sizeof(JpegPlane) + 255) & ~(size_t)255, need = table + J.blocks * 128;
    if (int r = jpegs_buffers(c, need)) return r;
    std::string msg;
    const auto t0 = std::chrono::steady_clock::now();
    if (int r = jpeg_decode_batch(files, bytes, n, J.files.data(), J.first_block.data(), (int16_t *)((char *)c->h_jin + table), msg)) return fail(c, r, "%s", msg.c_str());
    c->jpeg_entropy_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->jpeg_upload_bytes = need;
    HIPCK(c, hipEventRecord(c->jpeg_t[0], c->stream));
    HIPCK(c, hipMemcpyAsync(c->d_jin, c->h_jin, need, hipMemcpyHostToDevice, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_up, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_t[1], c->stream));
    c->jpeg_up_pending = true;
    HIPCK(c, launch_jpeg_idct((const int16_t *)((const char *)c->d_jin + table), (const JpegPlane *)c->d_jin, (int)J.planes.size(), J.blocks, c->d_jpeg, c->jpeg_cap, c->stream));
    HIPCK(c, hipEventRecord(c->jpeg_t[2], c->stream));
    return YOLO_OK;
}

}  // namespace yolo_impl
extern "C" {

int yolo_jpeg_info(const uint8_t *file, size_t bytes, struct yolo_jpeg_info *out)
{
    if (!file || !out) { g_op_err = "yolo_jpeg_info: file / out == NULL"; return YOLO_ERR_INVALID; }
    JpegFile f;
    if (int r = jpeg_parse(file, bytes, 0, &f, g_op_err)) return r;
    memset(out, 0, sizeof *out);
    out->h = f.h; out->w = f.w; out->components = f.comps; out->hs = f.hs; out->vs = f.vs; out->format = f.format; out->restart_interval = f.restart;
    out->mcus_w = f.mcux; out->mcus_h = f.mcuy;
    for (int p = 0; p < f.comps; ++p) { out->plane_w[p] = f.bw[p] * 8; out->plane_h[p] = f.bh[p] * 8; out->blocks[p] = f.bw[p] * f.bh[p]; }
    return YOLO_OK;
}

int yolo_jpeg_coefficients(const uint8_t *file, size_t bytes, int16_t *coef_out, size_t cap_blocks)
{
    if (!file || !coef_out) { g_op_err = "yolo_jpeg_coefficients: file / coef_out == NULL"; return YOLO_ERR_INVALID; }
    JpegFile f;
    if (int r = jpeg_parse(file, bytes, 0, &f, g_op_err)) return r;
    if (cap_blocks < f.blocks) { g_op_err = "yolo_jpeg_coefficients: file 0: its " + std::to_string(f.blocks) + " blocks do not fit coef_out's " + std::to_string(cap_blocks); return YOLO_ERR_INVALID; }
    return jpeg_decode(file, bytes, 0, f, coef_out, g_op_err);
}

int yolo_jpeg_to_rgb_host(const uint8_t *file, size_t bytes, uint8_t *rgb_out, size_t cap)
{
    if (!file || !rgb_out) { g_op_err = "yolo_jpeg_to_rgb_host: file / rgb_out == NULL"; return YOLO_ERR_INVALID; }
    JpegFile f;
    if (int r = jpeg_parse(file, bytes, 0, &f, g_op_err)) return r;
    if (cap < (size_t)f.h * f.w * 3) { g_op_err = "yolo_jpeg_to_rgb_host: file 0: " + std::to_string(f.h) + " x " + std::to_string(f.w) + " x 3 bytes do not fit rgb_out's " + std::to_string(cap); return YOLO_ERR_INVALID; }
    return jpeg_to_rgb_host(file, bytes, f, rgb_out, g_op_err);
}

int yolo_decode_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, yolo_frame_desc *descs_out, const uint8_t **device_pixels, size_t *device_bytes)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!descs_out || !device_pixels || !device_bytes) return fail(c, YOLO_ERR_INVALID, "yolo_decode_jpegs: descs_out / device_pixels / device_bytes == NULL");
    if (int r = jpegs_plan(c, files, bytes, n)) return r;
    if (int r = jpegs_run(c, files, bytes, n)) return r;
    memcpy(descs_out, c->jpeg.descs.data(), (size_t)n * sizeof(yolo_frame_desc));
    *device_pixels = c->d_jpeg; *device_bytes = c->jpeg_cap;
    return YOLO_OK;
}

int yolo_jpeg_decode_times(yolo_ctx *c, double *entropy_ms, double *upload_ms, double *idct_ms, size_t *upload_bytes)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!c->jpeg_t[0] || !c->jpeg_upload_bytes) return fail(c, YOLO_ERR_STATE, "yolo_jpeg_decode_times before any decode on this context");
    HIPCK(c, hipSetDevice(c->device));
    HIPCK(c, hipEventSynchronize(c->jpeg_t[2]));
    float up = 0.f, idct = 0.f;
    HIPCK(c, hipEventElapsedTime(&up, c->jpeg_t[0], c->jpeg_t[1]));
    HIPCK(c, hipEventElapsedTime(&idct, c->jpeg_t[c->je_stream_bytes ? 3 : 1], c->jpeg_t[2]));          // (behind the device's entropy stage where the decode ran one)
    if (entropy_ms) *entropy_ms = c->jpeg_entropy_ms;
    if (upload_ms) *upload_ms = up;
    if (idct_ms) *idct_ms = idct;
    if (upload_bytes) *upload_bytes = c->jpeg_upload_bytes;
    return YOLO_OK;
}

int yolo_set_jpeg_entropy(yolo_ctx *c, int mode)
{
    if (!c) return YOLO_ERR_INVALID;
    if (mode != YOLO_JPEG_ENTROPY_HOST && mode != YOLO_JPEG_ENTROPY_AUTO) return fail(c, YOLO_ERR_INVALID, "yolo_set_jpeg_entropy: mode %d (YOLO_JPEG_ENTROPY_HOST or YOLO_JPEG_ENTROPY_AUTO)", mode);
    c->jpeg_entropy_mode = mode;
    return YOLO_OK;
}

int yolo_jpeg_entropy(yolo_ctx *c) { return c ? c->jpeg_entropy_mode : YOLO_ERR_INVALID; }

int yolo_jpeg_entropy_times(yolo_ctx *c, int *device_files, int *host_files, int *intervals, double *scan_ms, double *device_ms, size_t *stream_bytes)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!c->jpeg_t[0] || !c->jpeg_upload_bytes) return fail(c, YOLO_ERR_STATE, "yolo_jpeg_entropy_times before any decode on this context");
    float dev = 0.f;
    if (c->je_stream_bytes) {
        HIPCK(c, hipSetDevice(c->device));
        HIPCK(c, hipEventSynchronize(c->jpeg_t[3]));
        HIPCK(c, hipEventElapsedTime(&dev, c->jpeg_t[1], c->jpeg_t[3]));
    }
    if (device_files) *device_files = c->je_dev_files;
    if (host_files) *host_files = c->je_host_files;
    if (intervals) *intervals = c->je_intervals;
    if (scan_ms) *scan_ms = c->je_scan_ms;
    if (device_ms) *device_ms = dev;
    if (stream_bytes) *stream_bytes = c->je_stream_bytes;
    return YOLO_OK;
}

int yolo_jpeg_intervals(const uint8_t *file, size_t bytes, uint32_t *begin_out, uint32_t *end_out, size_t cap, size_t *n_out)
{
    if (!file || !n_out) { g_op_err = "yolo_jpeg_intervals: file / n_out == NULL"; return YOLO_ERR_INVALID; }
    *n_out = 0;
    JpegFile f;
    if (int r = jpeg_parse(file, bytes, 0, &f, g_op_err)) return r;
    std::vector<JpegInterval> iv;
    try { if (!jpeg_intervals(file, bytes, f, iv)) return YOLO_OK; } catch (const std::bad_alloc &) { g_op_err = "yolo_jpeg_intervals: file 0: no memory for its intervals"; return YOLO_ERR_NOMEM; }
    *n_out = iv.size();
    if (!begin_out && !end_out) return YOLO_OK;
    if (cap < iv.size()) { g_op_err = "yolo_jpeg_intervals: file 0: its " + std::to_string(iv.size()) + " intervals do not fit the " + std::to_string(cap) + " of begin_out / end_out"; return YOLO_ERR_INVALID; }
    for (size_t i = 0; i < iv.size(); ++i) { if (begin_out) begin_out[i] = iv[i].begin; if (end_out) end_out[i] = iv[i].end; }
    return YOLO_OK;
}

int yolo_forward_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, int fit, float *det_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = jpegs_plan(c, files, bytes, n)) return r;
    // what the frames form would refuse, asked before the IDCT launch
    if (int r = frames_refusals(c, true, c->jpeg.view_bytes, c->jpeg.descs.data(), n, fit)) return r;
    if (int r = jpegs_run(c, files, bytes, n)) return r;
    return yolo_forward_frames_u8(c, c->d_jpeg, c->jpeg_cap, c->jpeg.descs.data(), n, fit, YOLO_DEVICE, det_out, out_loc);
}

int yolo_detect_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, int fit, float score_thr, float iou_thr, int max_out, int nms_mode,
                      int select_mode, int units, yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = jpegs_plan(c, files, bytes, n)) return r;
    if (int r = detect_images_check(c, fit, max_out, nms_mode, select_mode, units)) return r;
    if (int r = frames_refusals(c, true, c->jpeg.view_bytes, c->jpeg.descs.data(), n, fit)) return r;
    if (int r = jpegs_run(c, files, bytes, n)) return r;
    return yolo_detect_frames_u8(c, c->d_jpeg, c->jpeg_cap, c->jpeg.descs.data(), n, fit, YOLO_DEVICE, score_thr, iou_thr, max_out, nms_mode, select_mode, units, boxes_out, counts_out, out_loc);
}

int yolo_detect_tiled_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n_images, int tile_h, int tile_w, int overlap_h, int overlap_w, int fit,
                            float score_thr, float iou_thr, int max_out, int nms_mode, int select_mode, int relative, yolo_box *boxes_out, int32_t *counts_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = jpegs_plan(c, files, bytes, n_images)) return r;
    static const char *const who = "yolo_detect_tiled_jpegs";
    TiledWindows tw;          // every refusal of the tiled form and its window table before the IDCT launch, the device part after it
    if (int r = tiled_refusals(c, who, c->jpeg.view_bytes, nullptr, c->jpeg.descs.data(), n_images, tile_h, tile_w, overlap_h, overlap_w, fit, max_out, nms_mode, select_mode,
                               relative, boxes_out, counts_out, tw)) return r;
    if (int r = jpegs_run(c, files, bytes, n_images)) return r;
    return tiled_run(c, who, tw, c->d_jpeg, c->jpeg_cap, nullptr, c->jpeg.descs.data(), n_images, fit, YOLO_DEVICE, score_thr, iou_thr, max_out, nms_mode, select_mode, relative,
                     boxes_out, counts_out, out_loc);
}

// ---- classifier contexts: forward + tail; the [softmax] launch of the output layer selects the top_k itself (run_layer) ----
static int classify_check(yolo_ctx *c, int top_k, const int32_t *classes_out, const float *probs_out)
{
    if (int r = need_image(c, "yolo_classify")) return r;
    if (c->map_layer >= 0) return fail(c, YOLO_ERR_INVALID, "yolo_classify: the network is a map network ([net] yolo_output=map); use yolo_output_map / yolo_label_map");
    if (c->cls_layer < 0) return fail(c, YOLO_ERR_INVALID, "yolo_classify: the network is a detector (its output layer is not a [softmax])");
    const Layer &L = c->layers[c->cls_layer];
    if (top_k < 0 || top_k > CLS_TOPK_MAX || top_k > L.C) return fail(c, YOLO_ERR_INVALID, "top_k %d outside 0..%d", top_k, L.C < CLS_TOPK_MAX ? L.C : CLS_TOPK_MAX);
    if (top_k > 0 && L.groups != 1) return fail(c, YOLO_ERR_INVALID, "top_k needs a [softmax] with groups=1 (this one has groups=%d)", L.groups);
    if (!probs_out || (top_k > 0 && !classes_out)) return fail(c, YOLO_ERR_INVALID, "classes_out / probs_out == NULL");
    return YOLO_OK;
}

static int classify_out(yolo_ctx *c, int n, int top_k, int32_t *classes_out, float *probs_out, int out_loc)
{
    const Layer &L = c->layers[c->cls_layer];
    if (top_k == 0) return copy_out(c, probs_out, L.out.ptr, (size_t)n * L.C * 4, out_loc);
    if (int r = copy_out(c, classes_out, c->d_cls_idx, (size_t)n * top_k * 4, out_loc)) return r;
    return copy_out(c, probs_out, c->d_cls_prob, (size_t)n * top_k * 4, out_loc);
}

int yolo_classify(yolo_ctx *c, const void *images, int n, int fmt, int loc, float scale, int top_k, int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = classify_check(c, top_k, classes_out, probs_out)) return r;
    c->cls_topk = top_k; c->cls_mode = c->hierarchy_mode;
    const int r = forward_impl(c, images, n, fmt, loc, scale, nullptr, YOLO_DEVICE, false);
    c->cls_topk = 0; c->cls_mode = 0;
    if (r) return r;
    return classify_out(c, n, top_k, classes_out, probs_out, out_loc);
}

int yolo_classify_images_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n, int fit, int loc, int top_k,
                            int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = classify_check(c, top_k, classes_out, probs_out)) return r;
    c->cls_topk = top_k; c->cls_mode = c->hierarchy_mode;
    const int r = forward_images_impl(c, pixels, bytes, descs, n, fit, loc, nullptr, YOLO_DEVICE, false, 0.f);
    c->cls_topk = 0; c->cls_mode = 0;
    if (r) return r;
    return classify_out(c, n, top_k, classes_out, probs_out, out_loc);
}

// ... over decoded video frames: the frame fit of yolo_forward_frames_u8, the same tail
int yolo_classify_frames_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc, int top_k,
                            int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = classify_check(c, top_k, classes_out, probs_out)) return r;
    c->cls_topk = top_k; c->cls_mode = c->hierarchy_mode;
    const int r = forward_frames_impl(c, pixels, bytes, descs, n, fit, loc, nullptr, YOLO_DEVICE, false, 0.f);
    c->cls_topk = 0; c->cls_mode = 0;
    if (r) return r;
    return classify_out(c, n, top_k, classes_out, probs_out, out_loc);
}

// ... and over JPEG files: every refusal before the IDCT launch, then the frame form over the context's surface
int yolo_classify_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, int fit, int top_k, int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = classify_check(c, top_k, classes_out, probs_out)) return r;
    if (int r = jpegs_plan(c, files, bytes, n)) return r;
    if (int r = frames_refusals(c, true, c->jpeg.view_bytes, c->jpeg.descs.data(), n, fit)) return r;
    if (int r = jpegs_run(c, files, bytes, n)) return r;
    return yolo_classify_frames_u8(c, c->d_jpeg, c->jpeg_cap, c->jpeg.descs.data(), n, fit, YOLO_DEVICE, top_k, classes_out, probs_out, out_loc);
}

// ---- multi-view classification: darknet's `classifier valid10` (ten crops) and test_cifar_multi (the image and its mirror) on the
//      device.  Slots are ordered image * K + view and run max_batch per step: one fit launch over the view table straight from the source bytes, the
//      network, one device copy of the step's rows behind the rows of the steps before; after the last step ONE launch adds every image's K rows in view
//      order, scales them and selects the top-k ----
namespace {
const yolo_view ten_crop_views[5] = {{-1, -1, 0, 0}, {-1, 1, 0, 0}, {0, 0, 0, 0}, {1, -1, 0, 0}, {1, 1, 0, 0}};      // (dy, dx) in units of `shift`: classifier.c:273-277
int view_count(int views) { return views == YOLO_VIEWS_FLIP ? 2 : views == YOLO_VIEWS_TEN_CROP ? 10 : 0; }
yolo_view view_at(int views, int shift, int v)
{
    if (views == YOLO_VIEWS_FLIP) return yolo_view{0, 0, v, 0};
    const yolo_view u = ten_crop_views[v % 5];
    return yolo_view{u.dy * shift, u.dx * shift, v / 5, 0};
}
// the carving of yolo_ctx::d_views for a call of `images` images of K views and `len` classes: every array 256-byte aligned
struct ViewSlab {
    ViewDesc *views; float *rows, *sums, *work, *topk; int *cls; FrameDesc *frames; size_t bytes;
    ViewSlab(char *base, size_t images, size_t K, size_t len, size_t nframes)      // nframes: rows of the frame table (yolo_classify_views_frames_u8), 0 for images
    {
        size_t off = 0;
        auto take = [&](size_t n) { const uintptr_t p = (uintptr_t)base + off; off += (n + 255) & ~(size_t)255; return (void *)p; };      // (base == nullptr: the sizes only)
        views = (ViewDesc *)take(images * K * sizeof(ViewDesc)); rows = (float *)take(images * K * len * 4); sums = (float *)take(images * len * 4);
        work = (float *)take(images * len * 4); cls = (int *)take(images * CLS_TOPK_MAX * 4); topk = (float *)take(images * CLS_TOPK_MAX * 4);
        frames = (FrameDesc *)take(nframes * sizeof(FrameDesc));
        bytes = off;
    }
};
}

int yolo_view_table(int views, int shift, yolo_view *out, int cap, int *count)
{
    if (!count) { g_op_err = "yolo_view_table: count == NULL"; return YOLO_ERR_INVALID; }
    *count = 0;
    const int K = view_count(views);
    if (!K || shift < 0 || cap < 0 || (cap > 0 && !out)) { g_op_err = "yolo_view_table: views YOLO_VIEWS_FLIP or YOLO_VIEWS_TEN_CROP and shift >= 0 are needed (and out for cap > 0)"; return YOLO_ERR_INVALID; }
    *count = K;
    for (int v = 0; v < std::min(cap, K); ++v) out[v] = view_at(views, shift, v);
    return YOLO_OK;
}

// what views_refusals leaves for the device part: the view table in slot order, K
struct ViewPlan { std::vector<ViewDesc> table; int K = 0; bool ten = false; };

// Every refusal of multi-view classification, and the view table: no device work.  descs: packed images; frames (descs == NULL): decoded video frames, whose view
// rows name their frame by its index.  `bytes`: the size of the buffer the views will be read from -- the buffer itself is not read, so the JPEG form asks before
// its surface holds anything (have_pixels: the caller holds one)
static int views_refusals(yolo_ctx *c, const char *who, bool have_pixels, size_t bytes, const yolo_image_desc *descs, const yolo_frame_desc *frames, int n_images, int views,
                          int fit, int shift, int top_k, const int32_t *classes_out, const float *probs_out, ViewPlan &out)
{
    if (int r = classify_check(c, top_k, classes_out, probs_out)) return r;
    if (frames && c->in_c != 3) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: a network of %d planes ([net] yolo_input=planes) is not served: a frame is an RGB image after its conversion", who, c->in_c);
    if (!c->states.empty())
        return fail(c, YOLO_ERR_UNSUPPORTED, "%s: a network with recurrent state (%d state tensors) is not served: a batch slot is a stream there, not a view of an image", who, (int)c->states.size());
    if (c->dtype == YOLO_FP8) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: the fp8 configuration is not served", who);
    const int K = view_count(views);
    if (!K) return fail(c, YOLO_ERR_INVALID, "%s: bad views %d (YOLO_VIEWS_FLIP or YOLO_VIEWS_TEN_CROP)", who, views);
    if (shift < 0) return fail(c, YOLO_ERR_INVALID, "%s: shift %d < 0", who, shift);
    const bool ten = views == YOLO_VIEWS_TEN_CROP;
    if (!ten) {
        if (int r = fit_check(c, fit, who)) return r;
        if (frames && fit == YOLO_FIT_CV2_BGR) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: YOLO_FIT_CV2_BGR is not served for frames: a frame's format states its channel order (YOLO_PIX_BGR24 with YOLO_FIT_CV2)", who);
    } else {
        // resize_image divides by the resized extent - 1; the crop's coordinates y + shift, x + shift stay below the resized extents
        if ((long long)c->in_w + shift > 0x7fffffffLL || (long long)c->in_h + shift > 0x7fffffffLL)
            return fail(c, YOLO_ERR_INVALID, "%s: the network input %d x %d enlarged by shift %d does not fit an int", who, c->in_h, c->in_w, shift);
        if (c->in_w + shift < 2 || c->in_h + shift < 2)
            return fail(c, YOLO_ERR_INVALID, "%s: the resized image of %d x %d (network input + shift) is less than 2 pixels wide or high (darknet's resize_image divides by the extent - 1)", who, c->in_h + shift, c->in_w + shift);
    }
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "%s before weights were loaded", who);
    if (n_images < 1 || n_images > 0x7fffffff / K) return fail(c, YOLO_ERR_INVALID, "%s: %d images (1 .. %d)", who, n_images, 0x7fffffff / K);
    if (!have_pixels || (!descs && !frames)) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    if (frames) {
        if (bytes < 1 || bytes > 0xffffffffull) return fail(c, YOLO_ERR_INVALID, "packed buffer of %zu bytes (1 .. 2^32 - 1)", bytes);
        for (int i = 0; i < n_images; ++i) if (int r = frame_check(c, i, frames[i], bytes, ten ? -1 : fit)) return r;
    } else {
        if (bytes < (size_t)c->in_c || bytes > 0xffffffffull) return fail(c, YOLO_ERR_INVALID, "packed buffer of %zu bytes (%d .. 2^32 - 1)", bytes, c->in_c);
        for (int i = 0; i < n_images; ++i) if (int r = image_check(c, i, descs[i], bytes, ten ? -1 : fit)) return r;
    }
    const int nslots = n_images * K;
    try {
        out.table.resize(nslots);
    } catch (const std::bad_alloc &) { return fail(c, YOLO_ERR_NOMEM, "%s: the view table", who); }
    for (int i = 0; i < nslots; ++i) {
        const yolo_view v = view_at(views, shift, i % K);
        // a frame's view names its frame by index: the fit reads the frame table
        if (frames) out.table[i] = ViewDesc{(unsigned long long)(i / K), frames[i / K].h, frames[i / K].w, v.dy, v.dx, v.flip, shift};
        else out.table[i] = ViewDesc{descs[i / K].offset, descs[i / K].h, descs[i / K].w, v.dy, v.dx, v.flip, shift};
    }
    out.K = K; out.ten = ten;
    return YOLO_OK;
}

// the device part over a view table that passed views_refusals: pixels[bytes] holds the images, or the frames (frames != NULL: the call's own frame table goes
// into the slab -- n_images is not bound by max_batch, which is what the context's d_frames holds)
static int views_run(yolo_ctx *c, const ViewPlan &plan, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *frames, int n_images, int fit, int loc, float scale,
                     int top_k, int32_t *classes_out, float *probs_out, int out_loc)
{
    const Layer &L = c->layers[c->cls_layer];
    const int K = plan.K, nslots = n_images * K;
    const ViewSlab need(nullptr, n_images, K, L.C, frames ? n_images : 0);

    HIPCK(c, hipSetDevice(c->device));
    const uint8_t *src = nullptr;
    if (int r = stage_pixels(c, pixels, bytes, loc, &src)) return r;          // the source bytes go up once, whatever K is
    if (need.bytes > c->views_cap) {
        HIPCK(c, hipStreamSynchronize(c->stream));
        if (c->d_views) HIPCK(c, hipFree(c->d_views));
        c->d_views = nullptr; c->views_cap = 0;
        HIPCK(c, hipMalloc(&c->d_views, need.bytes)); c->views_cap = need.bytes;
    }
    const ViewSlab t((char *)c->d_views, n_images, K, L.C, frames ? n_images : 0);
    StreamDrain drain{c};
    HIPCK(c, hipMemcpyAsync(t.views, plan.table.data(), (size_t)nslots * sizeof(ViewDesc), hipMemcpyHostToDevice, c->stream));
    if (frames) HIPCK(c, hipMemcpyAsync(t.frames, frames, (size_t)n_images * sizeof(FrameDesc), hipMemcpyHostToDevice, c->stream));
    c->lean_thr = 0.f; c->cls_topk = 0; c->cls_mode = c->hierarchy_mode;
    struct ModeReset { yolo_ctx *c; ~ModeReset() { c->cls_mode = 0; } } reset{c};
    const int kfit = plan.ten ? FIT_TEN_CROP : fit;
    for (int first = 0; first < nslots; first += c->max_batch) {
        const int nb = std::min(c->max_batch, nslots - first);
        auto [dst, dt] = input_fill_dst(c);
        if (frames) HIPCK(c, launch_fit_frame_views(src, bytes, t.frames, t.views + first, nb, kfit, c->in_h, c->in_w, dst, dt, fill_stride(c), c->in_mul, c->in_add, c->stream));
        else HIPCK(c, launch_fit_views(src, bytes, t.views + first, nb, kfit, c->in_h, c->in_w, dst, dt, fill_stride(c), c->in_mul, c->in_add, c->stream, c->in_c));
        HIPCK(c, input_filled(c, (size_t)nb * c->in_h * c->in_w));
        if (int r = run_network(c, nb, false)) return r;
        // the step's rows behind those of the steps before: a device copy on the context stream, no host synchronisation
        HIPCK(c, hipMemcpy2DAsync(t.rows + (size_t)first * L.C, (size_t)L.C * 4, L.out.ptr, (size_t)L.out.stride * 4, (size_t)L.C * 4, nb, hipMemcpyDeviceToDevice, c->stream));
    }
    ViewReduceArgs a; memset(&a, 0, sizeof a);
    a.rows = t.rows; a.n = n_images; a.views = K; a.len = L.C; a.scale = scale; a.sums = t.sums; a.work = t.work; a.top_k = top_k; a.cls = t.cls; a.topk = t.topk;
    HIPCK(c, launch_view_reduce(a, c->stream));
    if (top_k == 0) return copy_out(c, probs_out, t.sums, (size_t)n_images * L.C * 4, out_loc);
    if (int r = copy_out(c, classes_out, t.cls, (size_t)n_images * top_k * 4, out_loc)) return r;
    return copy_out(c, probs_out, t.topk, (size_t)n_images * top_k * 4, out_loc);
}

int yolo_classify_views_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_image_desc *descs, int n_images, int views, int fit, int shift, int loc,
                           float scale, int top_k, int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    ViewPlan plan;
    if (int r = views_refusals(c, "yolo_classify_views_u8", pixels != nullptr, bytes, descs, nullptr, n_images, views, fit, shift, top_k, classes_out, probs_out, plan)) return r;
    return views_run(c, plan, pixels, bytes, nullptr, n_images, fit, loc, scale, top_k, classes_out, probs_out, out_loc);
}

int yolo_classify_views_frames_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n_images, int views, int fit, int shift, int loc,
                                  float scale, int top_k, int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!descs) return fail(c, YOLO_ERR_INVALID, "pixels / descs == NULL");
    ViewPlan plan;
    if (int r = views_refusals(c, "yolo_classify_views_frames_u8", pixels != nullptr, bytes, nullptr, descs, n_images, views, fit, shift, top_k, classes_out, probs_out, plan)) return r;
    return views_run(c, plan, pixels, bytes, descs, n_images, fit, loc, scale, top_k, classes_out, probs_out, out_loc);
}

// one decode batch for all n_images files, every refusal before the IDCT launch
int yolo_classify_views_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n_images, int views, int fit, int shift, float scale, int top_k,
                              int32_t *classes_out, float *probs_out, int out_loc)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = jpegs_plan(c, files, bytes, n_images)) return r;
    ViewPlan plan;
    if (int r = views_refusals(c, "yolo_classify_views_jpegs", true, c->jpeg.view_bytes, nullptr, c->jpeg.descs.data(), n_images, views, fit, shift, top_k, classes_out, probs_out, plan)) return r;
    if (int r = jpegs_run(c, files, bytes, n_images)) return r;
    return views_run(c, plan, c->d_jpeg, c->jpeg_cap, c->jpeg.descs.data(), n_images, fit, YOLO_DEVICE, scale, top_k, classes_out, probs_out, out_loc);
}

// ---- map contexts: the ragged native-size path.  One fit launch and one forward, as yolo_detect_images_u8, then ONE kernel that writes every
//      image's labels at that image's own size (launch_segment_labels) ----
// what a segment entry point is refused for before it looks at its images: no device work
static int segment_refusals(yolo_ctx *c, const char *who, int fit, const uint8_t *labels_u8)
{
    if (int r = need_map(c, who)) return r;
    if (int r = crop_fit_refused(c, fit, who, "labels")) return r;
    if (!labels_u8) return fail(c, YOLO_ERR_INVALID, "labels_u8 == NULL");
    if (c->layers[c->map_layer].C > 255) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: a map of %d channels (uint8 labels hold at most 255 classes)", who, c->layers[c->map_layer].C);
    return YOLO_OK;
}

// behind the forward of n images whose {offset, h, w} lie in d_descs: image i's labels at its own size at off[i] of a `total`-byte label buffer, to the host
static int segment_labels_out(yolo_ctx *c, int n, int fit, float thresh, const std::vector<unsigned long long> &off, size_t total, bool placed, uint8_t *labels_u8)
{
    const Layer &M = c->layers[c->map_layer];
    if (!c->d_label_off) HIPCK(c, hipMalloc((void **)&c->d_label_off, (size_t)c->max_batch * 8));
    HIPCK(c, hipMemcpyAsync(c->d_label_off, off.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    const float *map = nullptr; int map_stride = 0;
    if (int r = map_f32_view(c, n, &map, &map_stride)) return r;
    if (int r = map_labels_room(c, total)) return r;
    if (placed) HIPCK(c, hipMemsetAsync(c->d_map_labels, 0, total, c->stream));          // (gaps a caller's placement leaves)
    HIPCK(c, launch_segment_labels(map, map_stride, M.H, M.W, M.C, thresh, c->d_descs, c->d_label_off, n, fit, c->in_h, c->in_w, c->d_map_labels, c->stream));
    return copy_out(c, labels_u8, c->d_map_labels, total, YOLO_HOST);          // (synchronises: `off` outlives its asynchronous copy)
}

int yolo_segment_images_u8(yolo_ctx *c, const uint8_t *pixels, const yolo_image_desc *descs, int n, int fit, float thresh, uint8_t *labels_u8,
                           const uint64_t *label_offsets)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = segment_refusals(c, "yolo_segment_images_u8", fit, labels_u8)) return r;
    if (!descs || n < 1 || n > c->max_batch) return fail(c, YOLO_ERR_INVALID, "batch %d outside 1..%d", n, c->max_batch);
    // the packed buffer ends where its last image ends; the labels lie back to back in image order unless the caller places them
    size_t bytes = 0, total = 0;
    std::vector<unsigned long long> off(n);
    for (int i = 0; i < n; ++i) {
        if (descs[i].h < 1 || descs[i].w < 1) return fail(c, YOLO_ERR_INVALID, "image %d: %d x %d", i, (int)descs[i].h, (int)descs[i].w);
        const size_t px = (size_t)descs[i].h * (size_t)descs[i].w;
        bytes = std::max(bytes, (size_t)descs[i].offset + px * c->in_c);
        off[i] = label_offsets ? label_offsets[i] : total;
        total = std::max(total, (size_t)off[i] + px);
    }
    if (int r = forward_images_impl(c, pixels, bytes, descs, n, fit, YOLO_HOST, nullptr, YOLO_DEVICE, false, 0.f)) return r;
    return segment_labels_out(c, n, fit, thresh, off, total, label_offsets != nullptr, labels_u8);
}

// ... over decoded video frames: the frame fit, the forward, then the same label kernel over the {plane 0's offset, h, w} table frames_upload
// leaves in d_descs -- labels at each FRAME's own h x w.  pixels: host or device (loc)
int yolo_segment_frames_u8(yolo_ctx *c, const uint8_t *pixels, size_t bytes, const yolo_frame_desc *descs, int n, int fit, int loc, float thresh, uint8_t *labels_u8,
                           const uint64_t *label_offsets)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = segment_refusals(c, "yolo_segment_frames_u8", fit, labels_u8)) return r;
    if (int r = frames_check(c, pixels, bytes, descs, n, fit)) return r;
    size_t total = 0;
    std::vector<unsigned long long> off(n);
    for (int i = 0; i < n; ++i) {
        const size_t px = (size_t)descs[i].h * (size_t)descs[i].w;
        off[i] = label_offsets ? label_offsets[i] : total;
        total = std::max(total, (size_t)off[i] + px);
    }
    HIPCK(c, hipSetDevice(c->device));
    const uint8_t *src = nullptr;
    if (int r = stage_pixels(c, pixels, bytes, loc, &src)) return r;
    if (int r = frames_upload(c, descs, n)) return r;
    if (int r = frames_step(c, src, bytes, n, fit, false, 0.f)) return r;
    return segment_labels_out(c, n, fit, thresh, off, total, label_offsets != nullptr, labels_u8);
}

// ... and over JPEG files: every refusal before the IDCT launch, then the frame form over the context's surface
int yolo_segment_jpegs(yolo_ctx *c, const uint8_t *const *files, const size_t *bytes, int n, int fit, float thresh, uint8_t *labels_u8, const uint64_t *label_offsets)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = segment_refusals(c, "yolo_segment_jpegs", fit, labels_u8)) return r;
    if (int r = jpegs_plan(c, files, bytes, n)) return r;
    if (int r = frames_refusals(c, true, c->jpeg.view_bytes, c->jpeg.descs.data(), n, fit)) return r;
    if (int r = jpegs_run(c, files, bytes, n)) return r;
    return yolo_segment_frames_u8(c, c->d_jpeg, c->jpeg_cap, c->jpeg.descs.data(), n, fit, YOLO_DEVICE, thresh, labels_u8, label_offsets);
}

// ---- vector-input networks: one step over fp32 rows; many steps over tokens, the sampler's token fed back on the device ----
int yolo_vector_inputs(const yolo_ctx *c) { return c ? c->vec_n : YOLO_ERR_INVALID; }

static int need_vector(yolo_ctx *c, const char *what)
{
    if (!c->vec_n) return fail(c, YOLO_ERR_INVALID, "%s: the network reads images, not vectors ([net] yolo_input=vector with inputs=N declares a vector-input network); use yolo_forward* / yolo_detect* / yolo_classify*", what);
    return YOLO_OK;
}

int yolo_forward_vectors(yolo_ctx *c, const float *x, int n, int loc, float *out, size_t out_floats)
{
    if (!c) return YOLO_ERR_INVALID;
    if (int r = need_vector(c, "yolo_forward_vectors")) return r;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "yolo_forward_vectors before weights were loaded");
    if (n < 1 || n > c->max_batch) return fail(c, YOLO_ERR_INVALID, "batch %d outside 1..%d", n, c->max_batch);
    if (!x) return fail(c, YOLO_ERR_INVALID, "x == NULL");
    const Layer &O = c->layers[c->cls_layer];          // (the planner asks for a [softmax] output layer: dense fp32 rows)
    if (out && out_floats < (size_t)n * O.C) return fail(c, YOLO_ERR_INVALID, "output buffer too small (%zu < %zu floats)", out_floats, (size_t)n * O.C);
    HIPCK(c, hipSetDevice(c->device));
    const float *src = x;
    if (loc == YOLO_HOST) { HIPCK(c, hipMemcpyAsync(c->d_stage, x, (size_t)n * c->vec_n * 4, hipMemcpyHostToDevice, c->stream)); src = (const float *)c->d_stage; }
    HIPCK(c, launch_vector_in(src, n, c->vec_n, c->input.ptr, c->input.stride, c->input.dt, c->stream));
    if (int r = run_network(c, n)) return r;
    return out ? copy_out(c, out, O.out.ptr, (size_t)n * O.C * 4, YOLO_HOST) : YOLO_OK;
}

int yolo_set_temperature(yolo_ctx *c, float t)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!(t > 0.f) || !std::isfinite(t)) return fail(c, YOLO_ERR_INVALID, "yolo_set_temperature: the temperature must be finite and > 0");
    for (Layer &L : c->layers) if (L.type == L_SOFTMAX) L.temperature = t;
    drop_graph(c);          // a captured step holds the old value as a kernel argument
    return YOLO_OK;
}

int yolo_reset_temperature(yolo_ctx *c)
{
    if (!c) return YOLO_ERR_INVALID;
    for (Layer &L : c->layers) if (L.type == L_SOFTMAX) L.temperature = L.cfg_temperature;
    drop_graph(c);
    return YOLO_OK;
}

int yolo_sequence(yolo_ctx *c, int n, int steps, const int32_t *tokens, int forced, const float *uniforms, float clip,
                  int32_t *tokens_out, float *probs_out, int loc)
{
    static const char *const who = "yolo_sequence";
    if (!c) return YOLO_ERR_INVALID;
    // ---- every refusal, before any launch: a refused call changes no state ----
    if (int r = need_vector(c, who)) return r;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "%s before weights were loaded", who);
    const int N = c->vec_n;
    const Layer &O = c->layers[c->cls_layer];
    if (c->cls_layer != output_layer(c) || O.C != N || O.groups != 1 || O.tree >= 0)
        return fail(c, YOLO_ERR_UNSUPPORTED, "%s: the output layer must be a plain [softmax] over as many classes as the network has inputs (%d): the sampled token is the next input", who, N);
    if (N > CLS_SOFTMAX_MAX) return fail(c, YOLO_ERR_UNSUPPORTED, "%s: %d classes (the sampler stages at most %d)", who, N, CLS_SOFTMAX_MAX);
    if (n < 1 || n > c->max_batch) return fail(c, YOLO_ERR_INVALID, "%s: %d streams outside 1..%d", who, n, c->max_batch);
    if (steps < 1 || steps > (1 << 24)) return fail(c, YOLO_ERR_INVALID, "%s: %d steps outside 1..%d", who, steps, 1 << 24);
    if (forced < 1 || forced > steps) return fail(c, YOLO_ERR_INVALID, "%s: forced = %d outside 1..steps (%d)", who, forced, steps);
    if (!tokens) return fail(c, YOLO_ERR_INVALID, "%s: tokens == NULL", who);
    if (!uniforms && steps > forced) return fail(c, YOLO_ERR_INVALID, "%s: uniforms == NULL with steps (%d) > forced (%d): the steps behind the forced ones feed sampled tokens", who, steps, forced);
    if (uniforms && !tokens_out) return fail(c, YOLO_ERR_INVALID, "%s: tokens_out == NULL", who);
    if (loc != YOLO_HOST && loc != YOLO_DEVICE) return fail(c, YOLO_ERR_INVALID, "%s: bad loc %d", who, loc);
    if (loc == YOLO_HOST)
        for (size_t k = 0; k < (size_t)forced * n; ++k)
            if (tokens[k] < 0 || tokens[k] >= N) return fail(c, YOLO_ERR_INVALID, "%s: token %d (step %zu, stream %zu) outside 0..%d", who, (int)tokens[k], k / n, k % n, N - 1);
    const size_t sampled = uniforms ? (size_t)(steps - forced + 1) * n : 0, row = (size_t)n * N;

    // ---- device ----
    HIPCK(c, hipSetDevice(c->device));
    const int32_t *d_tok = tokens; const float *d_uni = uniforms; int32_t *d_out = tokens_out; float *d_probs = probs_out;
    if (loc == YOLO_HOST) {          // the slab: forced tokens | uniforms | sampled tokens | probabilities, each 256-byte aligned
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t o_uni = up((size_t)forced * n * 4), o_out = o_uni + up(sampled * 4), o_probs = o_out + up(sampled * 4), need = o_probs + (probs_out ? (size_t)steps * row * 4 : 0);
        if (need > c->seq_cap) {
            HIPCK(c, hipStreamSynchronize(c->stream));
            if (c->d_seq) HIPCK(c, hipFree(c->d_seq));
            c->d_seq = nullptr; c->seq_cap = 0;
            HIPCK(c, hipMalloc(&c->d_seq, need)); c->seq_cap = need;
        }
        char *base = (char *)c->d_seq;
        HIPCK(c, hipMemcpyAsync(base, tokens, (size_t)forced * n * 4, hipMemcpyHostToDevice, c->stream));
        if (uniforms) HIPCK(c, hipMemcpyAsync(base + o_uni, uniforms, sampled * 4, hipMemcpyHostToDevice, c->stream));
        d_tok = (const int32_t *)base; d_uni = (const float *)(base + o_uni); d_out = (int32_t *)(base + o_out); d_probs = probs_out ? (float *)(base + o_probs) : nullptr;
    }
    c->lean = false;
    for (int t = 0; t < steps; ++t) {
        if (t < forced) HIPCK(c, launch_token_in(d_tok + (size_t)t * n, n, N, c->input.ptr, c->input.stride, c->input.dt, c->stream));
        if (int r = run_layers(c, n)) return r;
        float *pt = d_probs ? d_probs + (size_t)t * row : nullptr;
        if (uniforms && t >= forced - 1) {
            SampleArgs a; memset(&a, 0, sizeof a);
            a.probs = (const float *)O.out.ptr; a.p_stride = O.out.stride; a.n = n; a.len = N; a.uniforms = d_uni + (size_t)(t - forced + 1) * n; a.clip = clip;
            a.tokens_out = d_out + (size_t)(t - forced + 1) * n; a.next_rows = c->input.ptr; a.row_stride = c->input.stride; a.dt = c->input.dt; a.probs_out = pt;
            HIPCK(c, launch_sample(a, c->stream));
        } else if (pt) HIPCK(c, hipMemcpy2DAsync(pt, (size_t)N * 4, O.out.ptr, (size_t)O.out.stride * 4, (size_t)N * 4, (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    }
    forward_done(c, n, false);
    if (loc != YOLO_HOST) return YOLO_OK;
    if (probs_out) HIPCK(c, hipMemcpyAsync(probs_out, d_probs, (size_t)steps * row * 4, hipMemcpyDeviceToHost, c->stream));
    if (sampled) HIPCK(c, hipMemcpyAsync(tokens_out, d_out, sampled * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCK(c, hipStreamSynchronize(c->stream));
    return YOLO_OK;
}

float yolo_fit_unit_value(int fit, int value)
{
    if (fit < YOLO_FIT_STRETCH || fit > YOLO_FIT_CENTER_CROP || value < 0 || value > 255) return NAN;
    return fit_unit_value(fit, (unsigned)value);
}

// the timing entry points' events: destroyed on every return path
namespace { struct EventSet {
    std::vector<hipEvent_t> e; bool ok = true;
    explicit EventSet(int n) { e.reserve(n); for (int i = 0; i < n; ++i) { hipEvent_t x; if (hipEventCreate(&x) != hipSuccess) { ok = false; break; } e.push_back(x); } }
    ~EventSet() { for (auto x : e) hipEventDestroy(x); }
    EventSet(const EventSet &) = delete; EventSet &operator=(const EventSet &) = delete;
}; }

int yolo_time_forward(yolo_ctx *c, int n, int iters, float *total_ms, float *conv_ms)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "weights not loaded");
    if (n < 1 || n > c->max_batch || iters < 1) return fail(c, YOLO_ERR_INVALID, "bad n/iters");
    HIPCK(c, hipSetDevice(c->device));
    EventSet evs(2); if (!evs.ok) return fail(c, YOLO_ERR_HIP, "hipEventCreate failed");
    hipEvent_t e0 = evs.e[0], e1 = evs.e[1];
    if (int r = state_keep(c)) return r;          // the passes below are steps of no stream: every state is handed back as it was found
    StateGuard guard{c};
    c->lean = false;
    if (c->stem_u8 && n > c->stem_u8_n) c->stem_u8 = nullptr;      // the staged uint8 buffer holds fewer images: the stem reads c->input instead
    if (total_ms) {
        HIPCK(c, hipEventRecord(e0, c->stream));
        for (int it = 0; it < iters; ++it) { int r = run_network(c, n); if (r) return r; }
        HIPCK(c, hipEventRecord(e1, c->stream)); HIPCK(c, hipEventSynchronize(e1));
        float ms = 0; HIPCK(c, hipEventElapsedTime(&ms, e0, e1)); *total_ms = ms / iters;
    }
    if (conv_ms) {
        // conv time = (all layers) - (all layers except the convs), each timed as ONE event pair around `iters` passes:
        // events around every conv would add a record-to-record gap per launch (+5 % here), and calibrating that gap away
        // over-corrects; the difference of two bulk timings agrees with rocprofv3's kernel trace to ~1 %
        float all_ms = 0, rest_ms = 0;
        for (int pass = 0; pass < 2; ++pass) {
            HIPCK(c, hipEventRecord(e0, c->stream));
            for (int it = 0; it < iters; ++it) { int r = run_layers(c, n, pass == 1); if (r) return r; }        // (the forward's own launch sequence)
            HIPCK(c, hipEventRecord(e1, c->stream)); HIPCK(c, hipEventSynchronize(e1));
            float ms = 0; HIPCK(c, hipEventElapsedTime(&ms, e0, e1)); (pass == 0 ? all_ms : rest_ms) = ms / iters;
        }
        *conv_ms = all_ms - rest_ms;
        forward_done(c, n, false);
    }
    return YOLO_OK;
}

int yolo_time_layers(yolo_ctx *c, int n, int iters, float *ms_out)
{
    if (!c || !ms_out) return YOLO_ERR_INVALID;
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "weights not loaded");
    if (n < 1 || n > c->max_batch || iters < 1) return fail(c, YOLO_ERR_INVALID, "bad n/iters");
    HIPCK(c, hipSetDevice(c->device));
    const int NL = (int)c->layers.size();
    c->lean = false; c->det_valid = true;      // (det_valid ahead of the passes, so also when one fails: kept, NOTEBOOK 2026-10-19)
    if (c->stem_u8 && n > c->stem_u8_n) c->stem_u8 = nullptr;      // see yolo_time_forward
    EventSet evs(NL + 1); if (!evs.ok) return fail(c, YOLO_ERR_HIP, "hipEventCreate failed");
    std::vector<hipEvent_t> &ev = evs.e;
    if (int r = state_keep(c)) return r;          // see yolo_time_forward
    StateGuard guard{c};
    std::vector<double> acc(NL, 0.0);
    for (int it = 0; it < iters; ++it) {
        HIPCK(c, hipEventRecord(ev[0], c->stream));
        if (int r = run_layers(c, n, false, &ev)) return r;
        HIPCK(c, hipStreamSynchronize(c->stream));
        for (int i = 0; i < NL; ++i) { float ms = 0; HIPCK(c, hipEventElapsedTime(&ms, ev[i], ev[i + 1])); acc[i] += ms; }
    }
    for (int i = 0; i < NL; ++i) ms_out[i] = (float)(acc[i] / iters);
    forward_done(c, n, false, -1);          // scores_mode is left as it was
    return YOLO_OK;
}

}  // extern "C"
