// Single-operator entry points of libyolo_hip.so (yolo_op_*): one kernel on caller-provided host tensors, for the parity tests.
#include "yolo_ctx.h"

namespace yolo_impl {

// a throw-away context for the single-operator entry points
struct OpScope {
    hipStream_t s = nullptr; std::vector<void *> bufs; int rc = YOLO_OK; std::string err;
    explicit OpScope(int device) { if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&s) != hipSuccess) rc = YOLO_ERR_HIP; }
    ~OpScope() { for (void *p : bufs) hipFree(p); if (s) hipStreamDestroy(s); }
    void *alloc(size_t bytes) { void *p = nullptr; if (hipMalloc(&p, bytes + 256) != hipSuccess) { rc = YOLO_ERR_NOMEM; return nullptr; } hipMemsetAsync(p, 0, bytes + 256, s); bufs.push_back(p); return p; }
    void *upload(const void *h, size_t bytes) { void *p = alloc(bytes); if (p && hipMemcpyAsync(p, h, bytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = YOLO_ERR_HIP; return p; }
    int download(void *h, const void *d, size_t bytes) { if (hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = YOLO_ERR_HIP; return rc; }
    bool ok(hipError_t e) { if (e != hipSuccess) { rc = YOLO_ERR_HIP; err = hipGetErrorString(e); } return e == hipSuccess; }
};
thread_local std::string g_op_err;

TView make_view(void *p, int n, int h, int w, int c, int stride, int dt) { TView v; v.ptr = p; v.n = n; v.h = h; v.w = w; v.c = c; v.stride = stride; v.dt = dt; return v; }

// a tree for the single operators: read, checked against the row length (len < 0: any), uploaded into the scope
static int op_tree(OpScope &S, const char *what, const char *tree_path, int len, Tree &t)
{
    std::string err;
    if (int r = load_tree(tree_path ? tree_path : "", t, err)) { g_op_err = std::string(what) + ": " + err; return r; }
    if (len >= 0 && t.n != len) { g_op_err = std::string(what) + ": the tree has " + std::to_string(t.n) + " nodes, the rows " + std::to_string(len) + " values"; return YOLO_ERR_INVALID; }
    size_t at[7];
    const std::vector<int> all = pack_tree(t, at);
    const int *d = (const int *)S.upload(all.data(), all.size() * 4);
    if (S.rc) { g_op_err = std::string(what) + ": allocation failed"; return S.rc; }
    t.dev = tree_dev(t, d, at);
    return YOLO_OK;
}

}  // namespace yolo_impl

// darknet's activation names (DN/activations.c get_activation) in the order of ACT_* / YOLO_ACT_*
int act_from_name(const char *name)
{
    static const char *const names[ACT_COUNT] = {"linear", "leaky", "relu", "relie", "logistic", "loggy", "elu", "ramp", "tanh", "plse", "stair", "hardtan", "lhtan"};
    for (int k = 0; name && k < ACT_COUNT; ++k) if (!strcmp(name, names[k])) return k;
    return -1;
}

// The body behind the three side-conv operators (SideConvArgs, kernels.h): x [n,h,w,cin] fp32 NHWC, the filters in the order of darknet's weight files, bias [cout]
// or NULL.  The operands are stored as `dtype` first; out_f32 != 0: the fp32 ("head") store of a 16-bit kernel.  An activation outside the slope family runs
// as the planner plans it: a linear epilogue, then k_activate on the output.  What a kind brings: its name and the phrases of its messages, `invalid` (a
// message of its own for arguments it alone checks, or NULL), `served` (its size / stride / padding rule), and two callables --
//   pack(dt, act, b0, wbuf, bv, sv) -> its argument struct with the geometry filled, the filters packed into wbuf, the bias into bv and, an xnor conv, the scale into sv
//   launch(a, d_sv, stream): its launcher (d_sv: the uploaded sv, NULL where sv stayed empty)
struct SideOp { const char *name, *kind, *invalid; bool served; const char *served_text; };
template <class Pack, class Launch>
static int op_side_conv(const SideOp &op, const float *x, int n, int h, int w, int cin, const float *filters, const float *bias, int cout, int act, int dtype, int out_f32,
                        float *out, int device, Pack pack, Launch launch)
{
    const std::string name = op.name;
    if (!x || !filters || !out || n < 1 || h < 1 || w < 1 || cin < 1 || cout < 1 || act < 0 || act >= ACT_COUNT) { g_op_err = name + ": bad arguments"; return YOLO_ERR_INVALID; }
    if (op.invalid) { g_op_err = name + ": " + op.invalid; return YOLO_ERR_INVALID; }
    if (dtype != YOLO_FP32 && dtype != YOLO_BF16 && dtype != YOLO_FP16) { g_op_err = name + ": dtype (fp32, bf16 or fp16; the fp8 and split-fp16 configurations do not serve " + op.kind + ")"; return YOLO_ERR_UNSUPPORTED; }
    if (!op.served) { g_op_err = name + ": served are " + op.served_text; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = name + ": no HIP device"; return S.rc; }
    const int dt = dtype == YOLO_FP32 ? DT_F32 : dtype == YOLO_FP16 ? DT_F16 : DT_BF16, odt = (out_f32 || dt == DT_F32) ? DT_F32 : dt;
    std::vector<float> b0(cout, 0.f); if (bias) memcpy(b0.data(), bias, (size_t)cout * 4);
    std::vector<uint8_t> wbuf; std::vector<float> bv, sv;
    auto a = pack(dt, act_is_slope(act) ? act : ACT_LINEAR, b0.data(), wbuf, bv, sv);
    const int cin_pad = roundup(cin, 8), cs = roundup(cout, odt == DT_F32 && dt != DT_F32 ? 4 : 8);
    const size_t pin = (size_t)n * h * w, pout = (size_t)n * a.Ho * a.Wo;
    void *d_w = S.upload(wbuf.data(), wbuf.size()); float *d_s = sv.empty() ? nullptr : (float *)S.upload(sv.data(), sv.size() * 4), *d_b = (float *)S.upload(bv.data(), bv.size() * 4);
    float *d_x32 = (float *)S.upload(x, pin * cin * 4);
    void *d_x = S.alloc(pin * cin_pad * dt_size(dt)), *d_o = S.alloc(pout * cs * dt_size(odt)); float *d_o32 = (float *)S.alloc(pout * cout * 4);
    if (S.rc) { g_op_err = name + ": allocation failed"; return S.rc; }
    if (!S.ok(launch_from_f32(d_x32, make_view(d_x, n, h, w, cin, cin_pad, dt), S.s))) { g_op_err = S.err; return S.rc; }
    a.in = d_x; a.in_stride = cin_pad; a.in_dt = dt; a.wt = d_w; a.bias = d_b; a.out = d_o; a.out_stride = cs; a.out_dt = odt; a.N = n; a.Cstore = cs;
    const TView vo = make_view(d_o, n, a.Ho, a.Wo, cout, cs, odt);
    if (!S.ok(launch(a, d_s, S.s))) { g_op_err = name + " launch: " + S.err; return S.rc; }
    if (!act_is_slope(act) && !S.ok(launch_activate(vo, false, act, S.s))) { g_op_err = name + " activation: " + S.err; return S.rc; }
    if (!S.ok(launch_to_f32(vo, d_o32, S.s))) { g_op_err = S.err; return S.rc; }
    S.download(out, d_o32, pout * cout * 4);
    if (S.rc) g_op_err = name + ": " + std::string(hipGetErrorString(hipGetLastError()));
    return S.rc;
}
// the Layer the packers read
static Layer side_op_layer(LType type, int cin, int cout, int size, int stride, int padding, int groups, int dt)
{
    Layer L; L.type = type; L.filters = cout; L.size = size; L.stride = stride; L.pad = padding; L.bn = 0; L.in_dt = dt; L.groups = groups;
    L.cin = cin; L.cin_pad = roundup(cin, 8);
    return L;
}

extern "C" {

int yolo_activation_code(const char *name) { return act_from_name(name); }

// the storage forms of yolo_op_activate / yolo_op_shortcut: a dense fp32 host tensor -> the device view of `dtype` (fp16x2: interleaved pairs of
// whole 32-channel groups) and back
namespace {
struct OpTensor { void *d = nullptr; TView v; int cp = 0; bool pair = false; };
bool op_tensor(OpScope &S, const float *host, int n, int h, int w, int c, int dtype, OpTensor &t)
{
    const size_t npix = (size_t)n * h * w;
    t.pair = dtype == YOLO_FP16X2;
    const int dt = dtype == YOLO_FP32 ? DT_F32 : dtype == YOLO_BF16 ? DT_BF16 : DT_F16;
    t.cp = roundup(c, t.pair ? 32 : 8);
    const int stride = t.pair ? 2 * t.cp : t.cp;
    t.d = S.alloc(npix * stride * dt_size(dt));
    t.v = make_view(t.d, n, h, w, c, stride, dt);
    if (!host) return !S.rc;
    float *d32 = (float *)S.alloc(npix * t.cp * 4);
    if (S.rc) return false;
    if (!S.ok(hipMemcpy2DAsync(d32, (size_t)t.cp * 4, host, (size_t)c * 4, (size_t)c * 4, npix, hipMemcpyHostToDevice, S.s))) return false;
    if (t.pair) return S.ok(launch_split_from_f32(d32, t.cp, t.d, stride, t.cp, npix, S.s));
    TView dst = t.v; dst.c = t.cp;
    return S.ok(launch_from_f32(d32, dst, S.s));
}
int op_tensor_out(OpScope &S, const OpTensor &t, float *host)
{
    const size_t npix = (size_t)t.v.n * t.v.h * t.v.w;
    float *d32 = (float *)S.alloc(npix * t.cp * 4);
    if (S.rc) return S.rc;
    TView all = t.v; all.c = t.cp;
    if (!S.ok(t.pair ? launch_split_to_f32(t.d, t.v.stride, t.cp, d32, t.cp, npix, S.s) : launch_to_f32(all, d32, S.s))) return S.rc;
    if (hipMemcpy2DAsync(host, (size_t)t.v.c * 4, d32, (size_t)t.cp * 4, (size_t)t.v.c * 4, npix, hipMemcpyDeviceToHost, S.s) != hipSuccess || hipStreamSynchronize(S.s) != hipSuccess) S.rc = YOLO_ERR_HIP;
    return S.rc;
}
bool op_dtype_ok(int dtype) { return dtype == YOLO_FP32 || dtype == YOLO_BF16 || dtype == YOLO_FP16 || dtype == YOLO_FP16X2; }
}  // namespace

int yolo_op_activate(const float *x, int n, int h, int w, int c, int act, int dtype, float *out, int device)
{
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 1 || act < 0 || act >= ACT_COUNT) { g_op_err = "activate: bad arguments"; return YOLO_ERR_INVALID; }
    if (!op_dtype_ok(dtype)) { g_op_err = "activate: dtype (fp32, bf16, fp16 or fp16x2)"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "activate: no HIP device"; return S.rc; }
    OpTensor t;
    if (!op_tensor(S, x, n, h, w, c, dtype, t) || !S.ok(launch_activate(t.v, t.pair, act, S.s)) || op_tensor_out(S, t, out)) { g_op_err = "activate: " + (S.err.empty() ? std::string("allocation or copy failed") : S.err); return S.rc ? S.rc : YOLO_ERR_HIP; }
    return YOLO_OK;
}

int yolo_op_shortcut(const float *x, int n, int h2, int w2, int c2, const float *from, int h1, int w1, int c1, int act, int dtype, float *out, int device)
{
    if (!x || !from || !out || n < 1 || h1 < 1 || w1 < 1 || c1 < 1 || h2 < 1 || w2 < 1 || c2 < 1 || act < 0 || act >= ACT_COUNT) { g_op_err = "shortcut: bad arguments"; return YOLO_ERR_INVALID; }
    if (!op_dtype_ok(dtype)) { g_op_err = "shortcut: dtype (fp32, bf16, fp16 or fp16x2)"; return YOLO_ERR_UNSUPPORTED; }
    if (!shortcut_geom(w1, h1, c1, w2, h2, c2).ok) { g_op_err = "shortcut: darknet requires w1 / w2 == h1 / h2 and w2 / w1 == h2 / h1"; return YOLO_ERR_UNSUPPORTED; }
    if (dtype == YOLO_FP16X2 && (c1 % 32 || c2 % 32)) { g_op_err = "shortcut (fp16x2): channel counts must be multiples of 32"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "shortcut: no HIP device"; return S.rc; }
    OpTensor a, b, o;
    if (!op_tensor(S, x, n, h2, w2, c2, dtype, a) || !op_tensor(S, from, n, h1, w1, c1, dtype, b) || !op_tensor(S, nullptr, n, h2, w2, c2, dtype, o) ||
        !S.ok(launch_shortcut(a.v, b.v, o.v, a.pair, act, S.s)) || op_tensor_out(S, o, out)) { g_op_err = "shortcut: " + (S.err.empty() ? std::string("allocation or copy failed") : S.err); return S.rc ? S.rc : YOLO_ERR_HIP; }
    return YOLO_OK;
}

// ---- single operators -----------------------------------------------------------------------
// yolo_op_conv2d for dtype YOLO_FP16X2: x (and the residual) enter as interleaved split-fp16 pairs (32 hi | 32 lo per 32-channel group), the
// filters as W_hi 32 | W_lo 32 rows, the conv runs the pair K loop with the SPLIT epilogue, the shortcut (if any) folded into it or
// (YOLO_SPLIT_UNFUSED) as the separate k_add_split launch of that configuration; the result is joined to fp32
static int op_conv2d_split(const float *x, int n, int h, int w, int cin, const float *w_hwio, const float *bias, int k, int stride,
                           int cout, int act, const float *residual, float *out, int tile_cfg, int device)
{
    if (cin % 8 || cout % 8) { g_op_err = "conv2d (fp16x2): channel counts must be multiples of 8"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) { g_op_err = "conv2d: no HIP device"; return S.rc; }
    const int cpi = roundup(cin, 32), cpo = roundup(cout, 32);
    Layer L; L.type = L_CONV; L.filters = cout; L.size = k; L.stride = stride; L.pad = k / 2; L.bn = 0; L.act = act; L.in_dt = DT_F16;
    L.cin = cin; L.cin_pad = 2 * cpi; L.kpad = k * k * L.cin_pad; L.cout_pad = roundup(cout, 256);
    const int ho = (h + 2 * L.pad - k) / stride + 1, wo = (w + 2 * L.pad - k) / stride + 1;
    std::vector<float> oihw((size_t)cout * cin * k * k), b0(cout, 0.f);
    for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw) for (int ci = 0; ci < cin; ++ci) for (int o = 0; o < cout; ++o)
        oihw[(((size_t)o * cin + ci) * k + kh) * k + kw] = w_hwio[(((size_t)kh * k + kw) * cin + ci) * cout + o];
    if (bias) memcpy(b0.data(), bias, (size_t)cout * 4);
    std::vector<uint8_t> wbuf; std::vector<float> bv, osc; pack_conv(L, b0.data(), oihw.data(), DT_F16, nullptr, wbuf, bv, osc, YOLO_SEM_TF, 2);
    void *d_w = S.upload(wbuf.data(), wbuf.size()); float *d_b = (float *)S.upload(bv.data(), bv.size() * 4);
    const size_t pin = (size_t)n * h * w, pout = (size_t)n * ho * wo;
    // fp32 images padded to whole 32-channel groups (zeros): the split kernels read whole groups
    auto upload_padded = [&](const float *src, size_t npix, int c, int cp) -> float * {
        float *d = (float *)S.alloc(npix * cp * 4);
        if (d && hipMemcpy2DAsync(d, (size_t)cp * 4, src, (size_t)c * 4, (size_t)c * 4, npix, hipMemcpyHostToDevice, S.s) != hipSuccess) S.rc = YOLO_ERR_HIP;
        return d;
    };
    float *d_x32 = upload_padded(x, pin, cin, cpi);
    void *d_x = S.alloc(pin * 2 * cpi * 2), *d_o = S.alloc(pout * 2 * cpo * 2), *d_z = S.alloc(4096);
    float *d_o32 = (float *)S.alloc(pout * cpo * 4);
    if (S.rc) { g_op_err = "conv2d: allocation failed"; return S.rc; }
    if (!S.ok(launch_split_from_f32(d_x32, cpi, d_x, 2 * cpi, cpi, pin, S.s))) { g_op_err = S.err; return S.rc; }
    ConvArgs a; memset(&a, 0, sizeof a);
    a.in = d_x; a.in_stride = 2 * cpi; a.wt = d_w; a.bias = d_b; a.out = d_o; a.out_stride = 2 * cpo; a.out_dt = DT_F16; a.in_dt = DT_F16;
    a.split = 1; a.pairk = 1; a.out_inv_scale = a.res_scale = a.mid_scale = a.mid_inv_scale = 1.f;
    a.N = n; a.H = h; a.W = w; a.Cin_pad = L.cin_pad; a.Ho = ho; a.Wo = wo; a.Cout = cout;
    a.ksize = k; a.stride = stride; a.pad = L.pad; a.Kpad = L.kpad; a.kchunk = conv_kchunk(L.cin_pad, DT_F16); a.act = act; a.zeros = d_z;
    conv_finalize(a);
    const int cfg = tile_cfg >= 0 ? tile_cfg : 6;
    if (!conv_cfg_runs(a, cfg)) { g_op_err = "conv2d (fp16x2): tile config not instantiated for split storage / not applicable to this shape"; return YOLO_ERR_UNSUPPORTED; }
    // the shortcut: fused into the conv's epilogue, or (YOLO_SPLIT_UNFUSED, the parity tests' A/B) as the separate launch a keep_layers plan makes
    void *d_r = nullptr;
    if (residual) {
        float *d_r32 = upload_padded(residual, pout, cout, cpo); d_r = S.alloc(pout * 2 * cpo * 2);
        if (S.rc) return S.rc;
        if (!S.ok(launch_split_from_f32(d_r32, cpo, d_r, 2 * cpo, cpo, pout, S.s))) { g_op_err = S.err; return S.rc; }
        if (!getenv("YOLO_SPLIT_UNFUSED")) { a.res = d_r; a.res_stride = 2 * cpo; }
    }
    if (!S.ok(launch_conv_bf16(a, cfg, S.s))) { g_op_err = "conv2d launch: " + S.err; return S.rc; }
    if (residual && !a.res && !S.ok(launch_add_split(d_o, 2 * cpo, d_r, 2 * cpo, d_o, 2 * cpo, cpo, pout, S.s))) { g_op_err = S.err; return S.rc; }
    if (!S.ok(launch_split_to_f32(d_o, 2 * cpo, cpo, d_o32, cpo, pout, S.s))) { g_op_err = S.err; return S.rc; }
    if (hipMemcpy2DAsync(out, (size_t)cout * 4, d_o32, (size_t)cpo * 4, (size_t)cout * 4, pout, hipMemcpyDeviceToHost, S.s) != hipSuccess || hipStreamSynchronize(S.s) != hipSuccess) S.rc = YOLO_ERR_HIP;
    if (S.rc) g_op_err = "conv2d: " + std::string(hipGetErrorString(hipGetLastError()));
    return S.rc;
}

int yolo_op_conv_num_cfgs(void) { return conv_num_cfgs(); }

// the dense conv on host tensors with an explicit padding (yolo_op_conv2d: padding = k / 2): k 1..CONV_MAX_SIZE in fp32, bf16 and fp16; the
// e4m3 and split-fp16 kernels keep k = 1 and 3 with padding k / 2
static int op_conv2d_any(const float *x, int n, int h, int w, int cin, const float *w_hwio, const float *bias, int k, int stride, int padding,
                         int cout, int act, const float *residual, float *out, int dtype, int tile_cfg, int device)
{
    if (!x || !w_hwio || !out || n < 1 || h < 1 || w < 1 || cin < 1 || cout < 1) { g_op_err = "conv2d: bad arguments"; return YOLO_ERR_INVALID; }
    if (!conv_served(k, stride, padding, h, w)) { g_op_err = "conv2d: served are 1 <= size <= " + std::to_string(CONV_MAX_SIZE) + ", stride >= 1, padding >= 0 and a filter no larger than the padded input"; return YOLO_ERR_UNSUPPORTED; }
    if ((dtype == YOLO_FP16X2 || dtype == YOLO_FP8) && ((k != 1 && k != 3) || padding != k / 2)) { g_op_err = "conv2d: the fp8 and split-fp16 configurations serve sizes 1 and 3 with padding size / 2 only"; return YOLO_ERR_UNSUPPORTED; }
    if (dtype == YOLO_FP16X2) return op_conv2d_split(x, n, h, w, cin, w_hwio, bias, k, stride, cout, act, residual, out, tile_cfg, device);
    OpScope S(device); if (S.rc) { g_op_err = "conv2d: no HIP device"; return S.rc; }
    // dtype YOLO_FP8: x, residual and the result are e4m3 tensors of scale 1 (the inputs are quantised here first)
    const bool f32 = dtype == YOLO_FP32; const int dt = f32 ? DT_F32 : dtype == YOLO_FP8 ? DT_FP8 : dtype == YOLO_FP16 ? DT_F16 : DT_BF16; const size_t es = dt_size(dt);
    const int gr = dt == DT_FP8 ? 16 : 8;
    Layer L; L.type = L_CONV; L.filters = cout; L.size = k; L.stride = stride; L.pad = padding; L.bn = 0; L.act = act; L.in_dt = dt;
    L.cin = cin; L.cin_pad = roundup(cin, gr); L.kpad = roundup(k * k * L.cin_pad, dt == DT_FP8 ? 128 : 64); L.cout_pad = roundup(cout, 256);
    const int ho = (h + 2 * L.pad - k) / stride + 1, wo = (w + 2 * L.pad - k) / stride + 1;
    // HWIO -> OIHW for the common packer
    std::vector<float> oihw((size_t)cout * cin * k * k), b0(cout, 0.f);
    for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw) for (int ci = 0; ci < cin; ++ci) for (int o = 0; o < cout; ++o)
        oihw[(((size_t)o * cin + ci) * k + kh) * k + kw] = w_hwio[(((size_t)kh * k + kw) * cin + ci) * cout + o];
    if (bias) memcpy(b0.data(), bias, (size_t)cout * 4);
    std::vector<uint8_t> wbuf; std::vector<float> bv, osc; pack_conv(L, b0.data(), oihw.data(), dt, nullptr, wbuf, bv, osc);
    void *d_w = S.upload(wbuf.data(), wbuf.size()); float *d_b = (float *)S.upload(bv.data(), bv.size() * 4);
    float *d_sc = dt == DT_FP8 ? (float *)S.upload(osc.data(), osc.size() * 4) : nullptr;
    float *d_x32 = (float *)S.upload(x, (size_t)n * h * w * cin * 4);
    void *d_x = S.alloc((size_t)n * h * w * L.cin_pad * es);
    const int cstride = roundup(cout, gr);
    void *d_o = S.alloc((size_t)n * ho * wo * cstride * es); float *d_o32 = (float *)S.alloc((size_t)n * ho * wo * cout * 4);
    void *d_r = nullptr;
    void *d_z = S.alloc(4096);
    if (S.rc) { g_op_err = "conv2d: allocation failed"; return S.rc; }
    TView vx = make_view(d_x, n, h, w, cin, L.cin_pad, dt);
    if (!S.ok(launch_from_f32(d_x32, vx, S.s))) { g_op_err = S.err; return S.rc; }
    if (residual) {
        float *d_r32 = (float *)S.upload(residual, (size_t)n * ho * wo * cout * 4); d_r = S.alloc((size_t)n * ho * wo * cstride * es);
        if (S.rc) return S.rc;
        if (!S.ok(launch_from_f32(d_r32, make_view(d_r, n, ho, wo, cout, cstride, dt), S.s))) { g_op_err = S.err; return S.rc; }
    }
    ConvArgs a; memset(&a, 0, sizeof a);
    a.in = d_x; a.in_stride = L.cin_pad; a.wt = d_w; a.bias = d_b; a.out = d_o; a.out_stride = cstride; a.out_dt = dt; a.in_dt = dt;
    a.oscale = d_sc; a.out_inv_scale = a.res_scale = a.mid_scale = a.mid_inv_scale = 1.f;
    a.res = d_r; a.res_stride = cstride; a.N = n; a.H = h; a.W = w; a.Cin_pad = L.cin_pad; a.Ho = ho; a.Wo = wo; a.Cout = cout;
    a.ksize = k; a.stride = stride; a.pad = L.pad; a.Kpad = L.kpad; a.kchunk = conv_kchunk(L.cin_pad, dt); a.act = act; a.zeros = d_z;
    conv_finalize(a);
    // what filter_fragments gives such a layer of a network: the packed filters once more, in fragment order (YOLO_NO_FRAGW=1: not, as there)
    if ((dt == DT_BF16 || dt == DT_F16) && k == 3 && stride == 1 && padding == 1 && L.cin_pad % 64 == 0 && L.kpad == 9 * L.cin_pad && !getenv("YOLO_NO_FRAGW")) {
        std::vector<uint16_t> wfrag(wbuf.size() / 2);
        fragment_order((const uint16_t *)wbuf.data(), L.cout_pad, L.kpad, wfrag.data());
        a.wf = S.upload(wfrag.data(), wfrag.size() * 2);
    }
    const int cfg = tile_cfg >= 0 ? tile_cfg : conv_default_cfg(a);
    if (conv_cfg_is_halo(cfg) && (f32 || !conv_cfg_runs(a, cfg))) { g_op_err = "conv2d: tile config not applicable to this shape (halo-staged form: 3x3, stride 1, size a multiple of 13, whole channel chunks)"; return YOLO_ERR_UNSUPPORTED; }
    if (!f32 && conv_is_wide(a) && !conv_cfg_runs(a, cfg)) { g_op_err = "conv2d: tile config " + std::to_string(cfg) + " has no form for convs of more than 25 taps (row / column tap masks)"; return YOLO_ERR_UNSUPPORTED; }
    hipError_t e;
    if (dt != DT_F32 && dt != DT_F16 && getenv("YOLO_CONV_DIAG") && a.Cin_pad % (dt == DT_FP8 ? 128 : 64) == 0) {
        // developer diagnostic: phase cycle sums of the stamped p176c128_s2 build (YOLO_CONV_DIAG=free: of the free-running halo form
        // f176c256), printed to stderr
        const bool dwide = !strcmp(getenv("YOLO_CONV_DIAG"), "free4");        // four waves of 176 x 64
        const bool dfree = (dwide || !strcmp(getenv("YOLO_CONV_DIAG"), "free")) && conv_halo13_ok(a) && dt == DT_BF16;
        const int wv = dfree && !dwide ? 8 : 4;
        const long tiles = dfree ? (long)n * ((h + 12) / 13) * ((w + 12) / 13) * ((cout + 255) / 256) : (((long)n * ho * wo + 175) / 176) * ((cout + 127) / 128);
        a.dbg = (unsigned long long *)S.alloc((size_t)tiles * wv * 16 * 8);
        a.dbg_light = getenv("YOLO_CONV_DIAG_LIGHT") ? 1 : 0;      // stamps around the K loop only (the clock measurement)
        if (dfree && !dwide && getenv("YOLO_CONV_DIAG_TAIL") && cout == 256) {
            // time the fused 1x1 tail too: any 128 x 256 filter block will do (the main filters' first rows), output to scratch
            a.w2 = a.wt; a.w2f = a.wt; a.K2pad = a.Kpad; a.b2 = a.bias; a.act2 = ACT_LEAKY; a.out2_stride = 128;
            a.out2 = S.alloc((size_t)n * ho * wo * 128 * 2);
        }
        // long enough for the clock to settle under load: the CDNA4 guide asks for >= 2 s of back-to-back launches before the stamps are read
        // (YOLO_CONV_DIAG_REPS; the stamps of the LAST launch are what is downloaded)
        const int reps = getenv("YOLO_CONV_DIAG_REPS") ? atoi(getenv("YOLO_CONV_DIAG_REPS")) : 200;
        for (int rep = 0; rep < reps; ++rep) e = dfree ? launch_conv_halo13_diag(a, S.s, dwide ? 1 : 0) : launch_conv_diag(a, S.s);
        std::vector<unsigned long long> hd((size_t)tiles * wv * 16);
        S.download(hd.data(), a.dbg, hd.size() * 8);
        double sum[16] = {0}; size_t cnt = hd.size() / 16;
        const unsigned long long kt = hd[5] >> 40;
        for (size_t i = 0; i < cnt; ++i)
            for (int q = 0; q < 16; ++q) sum[q] += q == 5 ? (double)(hd[i * 16 + 5] & 0xffffffffffull) : (double)hd[i * 16 + q];
        for (double &v : sum) v /= cnt;
        std::vector<unsigned long long> kclk(cnt); for (size_t i = 0; i < cnt; ++i) kclk[i] = hd[i * 16 + 15];
        std::nth_element(kclk.begin(), kclk.begin() + cnt / 2, kclk.end()); const double kmed = cnt ? (double)kclk[cnt / 2] : 0.0;
        fprintf(stderr, "diag: waves %zu KT %llu | per K-step cycles: wait+barrier %.0f  issue %.0f  ds_read+mfma %.0f  (loop total/KT %.0f) | epilogue %.0f cycles | shader clock %.0f MHz (K loop alone %.0f MHz, median over waves %.0f)\n",
                cnt, kt, sum[0] / kt, sum[1] / kt, sum[2] / kt, sum[3] / kt, sum[4], sum[5], sum[15], kmed);
        fprintf(stderr, "diag: setup (first instruction -> prologue issued) %.0f | first wait (prologue data + barrier) %.0f | epilogue: barrier %.0f  acc->LDS + barrier %.0f  shortcut add + store issue %.0f  store drain %.0f\n",
                sum[6], sum[7], sum[8], sum[9], sum[10], sum[11]);
        if (a.w2) fprintf(stderr, "diag: fused 1x1 tail: barrier %.0f  fragments + MFMA + pack %.0f  barrier %.0f (then the tail's stores, in `store drain`)\n", sum[12], sum[13], sum[14]);
    } else
        e = f32 ? launch_conv_f32(a, S.s) : dt == DT_FP8 ? launch_conv_fp8(a, cfg, S.s) : launch_conv_bf16(a, cfg, S.s);
    if (!S.ok(e)) { g_op_err = "conv2d launch: " + S.err; return S.rc; }
    if (!S.ok(launch_to_f32(make_view(d_o, n, ho, wo, cout, cstride, dt), d_o32, S.s))) { g_op_err = S.err; return S.rc; }
    S.download(out, d_o32, (size_t)n * ho * wo * cout * 4);
    if (S.rc) g_op_err = "conv2d: " + std::string(hipGetErrorString(hipGetLastError()));
    return S.rc;
}

int yolo_op_conv2d(const float *x, int n, int h, int w, int cin, const float *w_hwio, const float *bias, int k, int stride,
                   int cout, int act, const float *residual, float *out, int dtype, int tile_cfg, int device)
{
    return op_conv2d_any(x, n, h, w, cin, w_hwio, bias, k, stride, k / 2, cout, act, residual, out, dtype, tile_cfg, device);
}

int yolo_op_conv2d_pad(const float *x, int n, int h, int w, int cin, const float *w_hwio, const float *bias, int k, int stride, int padding,
                       int cout, int act, const float *residual, float *out, int dtype, int tile_cfg, int device)
{
    return op_conv2d_any(x, n, h, w, cin, w_hwio, bias, k, stride, padding, cout, act, residual, out, dtype, tile_cfg, device);
}

// darknet's [deconvolutional]: w_iohw [cin][cout][size][size]
int yolo_op_deconv2d(const float *x, int n, int h, int w, int cin, const float *w_iohw, const float *bias, int size, int stride, int padding,
                     int cout, int act, int dtype, int out_f32, float *out, int device)
{
    const SideOp op = {"deconv2d", "[deconvolutional]", nullptr, deconv_served(size, stride, padding, h, w), "1 <= size <= 7, 1 <= stride <= 4, 0 <= padding < size and a positive output"};
    return op_side_conv(op, x, n, h, w, cin, w_iohw, bias, cout, act, dtype, out_f32, out, device,
        [&](int dt, int a, const float *b0, std::vector<uint8_t> &wbuf, std::vector<float> &bv, std::vector<float> &) {
            pack_deconv(side_op_layer(L_DECONV, cin, cout, size, stride, padding, 1, dt), b0, w_iohw, dt, wbuf, bv);
            return deconv_geometry(size, stride, padding, h, w, roundup(cin, 8), cout, a, dt); },
        [](const DeconvArgs &a, const float *, hipStream_t s) { return launch_deconv(a, s); });
}

// darknet's [convolutional] with groups=: w_oihw [cout][cin / groups][size][size].  groups == 1 runs the same kernel with one group
int yolo_op_conv2d_grouped(const float *x, int n, int h, int w, int cin, const float *w_oihw, const float *bias, int size, int stride, int padding,
                           int cout, int groups, int act, int dtype, int out_f32, float *out, int device)
{
    const SideOp op = {"conv2d_grouped", "groups=", (groups < 1 || cin % groups || cout % groups) ? "groups must be >= 1 and divide cin and cout" : nullptr,
                       gconv_served(size, stride, padding, h, w), "1 <= size <= 7, 1 <= stride <= 4, 0 <= padding < size and a positive output"};
    return op_side_conv(op, x, n, h, w, cin, w_oihw, bias, cout, act, dtype, out_f32, out, device,
        [&](int dt, int a, const float *b0, std::vector<uint8_t> &wbuf, std::vector<float> &bv, std::vector<float> &) {
            pack_gconv(side_op_layer(L_GCONV, cin, cout, size, stride, padding, groups, dt), b0, w_oihw, dt, wbuf, bv);
            return gconv_geometry(size, stride, padding, h, w, cin, cout, groups, a, dt); },
        [](const GConvArgs &a, const float *, hipStream_t s) { return launch_gconv(a, s); });
}

// darknet's [convolutional] with xnor=1: w_oihw [cout][cin][size][size].  The sign is taken of x as stored; the filters become alpha_f * sign(w)
int yolo_op_conv2d_xnor(const float *x, int n, int h, int w, int cin, const float *w_oihw, const float *bias, int size, int stride, int padding,
                        int cout, int act, int dtype, int out_f32, float *out, int device)
{
    const SideOp op = {"conv2d_xnor", "xnor=1", nullptr, xconv_served(size, stride, padding, h, w), "1 <= size <= 11, stride >= 1, padding >= 0 and a positive output"};
    return op_side_conv(op, x, n, h, w, cin, w_oihw, bias, cout, act, dtype, out_f32, out, device,
        [&](int dt, int a, const float *b0, std::vector<uint8_t> &wbuf, std::vector<float> &bv, std::vector<float> &sv) {
            pack_xconv(side_op_layer(L_XCONV, cin, cout, size, stride, padding, 1, dt), b0, w_oihw, wbuf, sv, bv);
            return xconv_geometry(size, stride, padding, h, w, cin, cout, a); },
        [](XConvArgs &a, const float *d_sv, hipStream_t s) { a.scale = d_sv; return launch_xconv(a, s); });
}

int yolo_op_l2norm(const float *x, int n, int h, int w, int c, int dtype, float *out, int device)
{
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 1) { g_op_err = "l2norm: bad arguments"; return YOLO_ERR_INVALID; }
    if (dtype != YOLO_FP32 && dtype != YOLO_BF16 && dtype != YOLO_FP16) { g_op_err = "l2norm: dtype (fp32, bf16 or fp16)"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "l2norm: no HIP device"; return S.rc; }
    OpTensor a, o;
    if (!op_tensor(S, x, n, h, w, c, dtype, a) || !op_tensor(S, nullptr, n, h, w, c, dtype, o) || !S.ok(launch_l2norm(a.v, o.v, S.s)) || op_tensor_out(S, o, out)) { g_op_err = "l2norm: " + (S.err.empty() ? std::string("allocation or copy failed") : S.err); return S.rc ? S.rc : YOLO_ERR_HIP; }
    return YOLO_OK;
}

int yolo_op_lrn(const float *x, int n, int h, int w, int c, int size, float alpha, float beta, float kappa, int dtype, float *out, int device)
{
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 1 || size < 1) { g_op_err = "lrn: bad arguments"; return YOLO_ERR_INVALID; }
    if (size > LRN_MAX_SIZE) { g_op_err = "lrn: size (1.." + std::to_string((int)LRN_MAX_SIZE) + " are served)"; return YOLO_ERR_UNSUPPORTED; }
    if (size / 2 > c) { g_op_err = "lrn: size / 2 must not exceed the channel count (the reference reads past the image)"; return YOLO_ERR_INVALID; }
    if (dtype != YOLO_FP32 && dtype != YOLO_BF16 && dtype != YOLO_FP16) { g_op_err = "lrn: dtype (fp32, bf16 or fp16)"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "lrn: no HIP device"; return S.rc; }
    OpTensor a, o;
    if (!op_tensor(S, x, n, h, w, c, dtype, a) || !op_tensor(S, nullptr, n, h, w, c, dtype, o) || !S.ok(launch_lrn(a.v, o.v, size, alpha, beta, kappa, S.s)) || op_tensor_out(S, o, out)) { g_op_err = "lrn: " + (S.err.empty() ? std::string("allocation or copy failed") : S.err); return S.rc ? S.rc : YOLO_ERR_HIP; }
    return YOLO_OK;
}

int yolo_op_upsample(const float *x, int n, int h, int w, int c, int stride, float scale, int dtype, float *out, int device)
{
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 1) { g_op_err = "upsample: bad arguments"; return YOLO_ERR_INVALID; }
    if (stride < 1 || stride > 8) { g_op_err = "upsample: stride (1..8; a stride below 1 is darknet's reverse mode, which is not served)"; return YOLO_ERR_UNSUPPORTED; }
    if (dtype != YOLO_FP32 && dtype != YOLO_BF16 && dtype != YOLO_FP16) { g_op_err = "upsample: dtype (fp32, bf16 or fp16)"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "upsample: no HIP device"; return S.rc; }
    OpTensor a, o;
    if (!op_tensor(S, x, n, h, w, c, dtype, a) || !op_tensor(S, nullptr, n, h * stride, w * stride, c, dtype, o) || !S.ok(launch_upsample_nearest(a.v, o.v, stride, scale, S.s)) || op_tensor_out(S, o, out)) { g_op_err = "upsample: " + (S.err.empty() ? std::string("allocation or copy failed") : S.err); return S.rc ? S.rc : YOLO_ERR_HIP; }
    return YOLO_OK;
}

int yolo_op_label_map(const float *map, int n, int h, int w, int c, float thresh, uint8_t *labels_out, int device)
{
    if (!map || !labels_out || n < 1 || h < 1 || w < 1 || c < 1) { g_op_err = "label_map: bad arguments"; return YOLO_ERR_INVALID; }
    if (c > 255) { g_op_err = "label_map: a map of " + std::to_string(c) + " channels (uint8 labels hold at most 255 classes; 255 itself means `below thresh`)"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "label_map: no HIP device"; return S.rc; }
    const size_t npix = (size_t)n * h * w;
    const float *d_m = (const float *)S.upload(map, npix * c * 4); uint8_t *d_l = (uint8_t *)S.alloc(npix);
    if (S.rc) { g_op_err = "label_map: allocation failed"; return S.rc; }
    if (!S.ok(launch_label_map(d_m, c, npix, c, thresh, d_l, S.s))) { g_op_err = "label_map: " + S.err; return S.rc; }
    return S.download(labels_out, d_l, npix);
}

static int ew_op(int kind, const float *x, int n, int h, int w, int c, int p0, int p1, int p2, float *out, int device)
{
    // any channel count: the tensors are stored as the planner stores them, bf16 with the pixel stride rounded up to whole 8-channel granules
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 1) { g_op_err = "op: bad arguments"; return YOLO_ERR_INVALID; }
    int ho = h, wo = w, co = c;
    if (kind == 0) { ho = 2 * h; wo = 2 * w; }
    else if (kind == 1) {
        if (p0 < 1 || h % p0 || w % p0) { g_op_err = "reorg: the stride must divide height and width"; return YOLO_ERR_INVALID; }
        if (p1 == YOLO_SEM_DARKNET && c < p0 * p0) { g_op_err = "reorg: darknet semantics need at least stride^2 channels"; return YOLO_ERR_INVALID; }
        ho = h / p0; wo = w / p0; co = c * p0 * p0;
    }
    else {
        if (p0 < 1 || p1 < 1) { g_op_err = "maxpool: size and stride must be positive"; return YOLO_ERR_INVALID; }
        int pad = (p0 - 1) / 2; ho = (h + 2 * pad) / p1; wo = (w + 2 * pad) / p1;
        if (ho < 1 || wo < 1) { g_op_err = "maxpool: no output pixel"; return YOLO_ERR_INVALID; }
    }
    OpScope S(device); if (S.rc) { g_op_err = "op: no HIP device"; return S.rc; }
    OpTensor a, o;
    bool ok = op_tensor(S, x, n, h, w, c, YOLO_BF16, a) && op_tensor(S, nullptr, n, ho, wo, co, YOLO_BF16, o);
    if (ok && kind == 0) ok = S.ok(launch_upsample2x(a.v, o.v, p0 == YOLO_SEM_TF, S.s));
    if (ok && kind == 1) ok = S.ok(launch_reorg(a.v, o.v, p0, p1 == YOLO_SEM_DARKNET, S.s));
    if (ok && kind == 2) ok = S.ok(launch_maxpool(a.v, o.v, p0, p1, (p0 - 1) / 2, S.s));
    if (!ok || op_tensor_out(S, o, out)) { g_op_err = "op: " + (S.err.empty() ? std::string("allocation or copy failed") : S.err); return S.rc ? S.rc : YOLO_ERR_HIP; }
    return YOLO_OK;
}
int yolo_op_upsample2x(const float *x, int n, int h, int w, int c, int semantics, float *out, int device) { return ew_op(0, x, n, h, w, c, semantics, 0, 0, out, device); }
int yolo_op_reorg(const float *x, int n, int h, int w, int c, int stride, int semantics, float *out, int device) { return ew_op(1, x, n, h, w, c, stride, semantics, 0, out, device); }
int yolo_op_maxpool(const float *x, int n, int h, int w, int c, int size, int stride, float *out, int device) { return ew_op(2, x, n, h, w, c, size, stride, 0, out, device); }

int yolo_op_avgpool(const float *x, int n, int h, int w, int c, int dtype, float *out, int device)
{
    if (!x || !out || n < 1 || h < 1 || w < 1 || c < 1) { g_op_err = "avgpool: bad arguments"; return YOLO_ERR_INVALID; }
    if (dtype != YOLO_FP32 && dtype != YOLO_BF16 && dtype != YOLO_FP16 && dtype != YOLO_FP16X2) { g_op_err = "avgpool: dtype (fp32, bf16, fp16 or fp16x2)"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "avgpool: no HIP device"; return S.rc; }
    const size_t npix = (size_t)n * h * w;
    float *d_o32 = (float *)S.alloc((size_t)n * c * 4);
    bool ok;
    if (dtype == YOLO_FP16X2) {          // fp32 padded to whole 32-channel groups -> interleaved pairs -> pool -> joined again
        const int cp = roundup(c, 32);
        float *d_x32 = (float *)S.alloc(npix * cp * 4), *d_j = (float *)S.alloc((size_t)n * cp * 4);
        void *d_x = S.alloc(npix * 2 * cp * 2), *d_o = S.alloc((size_t)n * 2 * cp * 2);
        if (S.rc) { g_op_err = "avgpool: allocation failed"; return S.rc; }
        ok = S.ok(hipMemcpy2DAsync(d_x32, (size_t)cp * 4, x, (size_t)c * 4, (size_t)c * 4, npix, hipMemcpyHostToDevice, S.s));
        ok = ok && S.ok(launch_split_from_f32(d_x32, cp, d_x, 2 * cp, cp, npix, S.s));
        ok = ok && S.ok(launch_avgpool(make_view(d_x, n, h, w, c, 2 * cp, DT_F16), true, make_view(d_o, n, 1, 1, c, 2 * cp, DT_F16), S.s));
        ok = ok && S.ok(launch_split_to_f32(d_o, 2 * cp, cp, d_j, cp, (size_t)n, S.s));
        ok = ok && S.ok(launch_to_f32(make_view(d_j, n, 1, 1, c, cp, DT_F32), d_o32, S.s));
    } else {
        const int dt = dtype == YOLO_FP32 ? DT_F32 : dtype == YOLO_FP16 ? DT_F16 : DT_BF16, cs = roundup(c, 8);
        float *d_x32 = (float *)S.upload(x, npix * c * 4);
        void *d_x = S.alloc(npix * cs * dt_size(dt)), *d_o = S.alloc((size_t)n * cs * dt_size(dt));
        if (S.rc) { g_op_err = "avgpool: allocation failed"; return S.rc; }
        ok = S.ok(launch_from_f32(d_x32, make_view(d_x, n, h, w, c, cs, dt), S.s));
        ok = ok && S.ok(launch_avgpool(make_view(d_x, n, h, w, c, cs, dt), false, make_view(d_o, n, 1, 1, c, cs, dt), S.s));
        ok = ok && S.ok(launch_to_f32(make_view(d_o, n, 1, 1, c, cs, dt), d_o32, S.s));
    }
    if (!ok) { g_op_err = "avgpool: " + S.err; return S.rc; }
    return S.download(out, d_o32, (size_t)n * c * 4);
}

int yolo_op_softmax(const float *x, int n, int len, int groups, float temperature, int top_k, float *probs_out,
                    int32_t *classes_out, float *topk_probs_out, int device)
{
    if (!x || !probs_out || n < 1 || len < 1 || groups < 1 || len % groups || !(temperature > 0.f)) { g_op_err = "softmax: bad arguments"; return YOLO_ERR_INVALID; }
    if (len / groups > CLS_SOFTMAX_MAX) { g_op_err = "softmax: more than 8192 logits in a group"; return YOLO_ERR_UNSUPPORTED; }
    if (top_k < 0 || top_k > CLS_TOPK_MAX || (top_k > 0 && (groups != 1 || !classes_out || !topk_probs_out))) { g_op_err = "softmax: top_k needs 1..32, groups == 1 and both output arrays"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) { g_op_err = "softmax: no HIP device"; return S.rc; }
    SoftmaxArgs a; memset(&a, 0, sizeof a);
    a.x = (const float *)S.upload(x, (size_t)n * len * 4); a.x_stride = len; a.n = n; a.groups = groups; a.len = len / groups; a.temperature = temperature;
    a.probs = (float *)S.alloc((size_t)n * len * 4); a.p_stride = len; a.top_k = top_k;
    a.cls = (int *)S.alloc((size_t)n * CLS_TOPK_MAX * 4); a.topk_probs = (float *)S.alloc((size_t)n * CLS_TOPK_MAX * 4);
    if (S.rc) { g_op_err = "softmax: allocation failed"; return S.rc; }
    if (!S.ok(launch_softmax_topk(a, S.s))) { g_op_err = "softmax: " + S.err; return S.rc; }
    if (top_k > 0) { S.download(classes_out, a.cls, (size_t)n * top_k * 4); S.download(topk_probs_out, a.topk_probs, (size_t)n * top_k * 4); }
    return S.download(probs_out, a.probs, (size_t)n * len * 4);
}

int yolo_op_view_reduce(const float *rows, int n, int views, int len, float scale, int top_k, float *sums_out, int32_t *classes_out, float *top_out, int device)
{
    if (!rows || !sums_out || n < 1 || len < 1 || views < 1 || views > VIEWS_MAX || (size_t)n * views > 0x7fffffffull) { g_op_err = "view_reduce: bad arguments (rows, sums_out, n >= 1, len >= 1, views 1..32)"; return YOLO_ERR_INVALID; }
    if (top_k < 0 || top_k > CLS_TOPK_MAX || top_k > len || (top_k > 0 && (!classes_out || !top_out))) { g_op_err = "view_reduce: top_k needs 0..min(32, len) and both output arrays"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) { g_op_err = "view_reduce: no HIP device"; return S.rc; }
    ViewReduceArgs a; memset(&a, 0, sizeof a);
    a.rows = (const float *)S.upload(rows, (size_t)n * views * len * 4); a.n = n; a.views = views; a.len = len; a.scale = scale; a.top_k = top_k;
    a.sums = (float *)S.alloc((size_t)n * len * 4); a.work = (float *)S.alloc((size_t)n * len * 4);
    a.cls = (int *)S.alloc((size_t)n * CLS_TOPK_MAX * 4); a.topk = (float *)S.alloc((size_t)n * CLS_TOPK_MAX * 4);
    if (S.rc) { g_op_err = "view_reduce: allocation failed"; return S.rc; }
    if (!S.ok(launch_view_reduce(a, S.s))) { g_op_err = "view_reduce: " + S.err; return S.rc; }
    if (top_k > 0) { S.download(classes_out, a.cls, (size_t)n * top_k * 4); S.download(top_out, a.topk, (size_t)n * top_k * 4); }
    return S.download(sums_out, a.sums, (size_t)n * len * 4);
}

int yolo_op_sample(const float *probs, int n, int len, const float *uniforms, float clip, int32_t *out, int device)
{
    if (!probs || !uniforms || !out || n < 1 || len < 1) { g_op_err = "sample: bad arguments"; return YOLO_ERR_INVALID; }
    if (len > CLS_SOFTMAX_MAX) { g_op_err = "sample: more than 8192 probabilities in a row"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "sample: no HIP device"; return S.rc; }
    SampleArgs a; memset(&a, 0, sizeof a);
    a.probs = (const float *)S.upload(probs, (size_t)n * len * 4); a.p_stride = len; a.n = n; a.len = len;
    a.uniforms = (const float *)S.upload(uniforms, (size_t)n * 4); a.clip = clip; a.tokens_out = (int32_t *)S.alloc((size_t)n * 4);
    if (S.rc) { g_op_err = "sample: allocation failed"; return S.rc; }
    if (!S.ok(launch_sample(a, S.s))) { g_op_err = "sample: " + S.err; return S.rc; }
    return S.download(out, a.tokens_out, (size_t)n * 4);
}

int yolo_op_tree_softmax(const float *x, int n, int len, const char *tree_path, float temperature, int mode, float *out, int device)
{
    if (!x || !out || n < 1 || len < 1 || !(temperature > 0.f) || mode < YOLO_HIER_CONDITIONAL || mode > YOLO_HIER_LEAVES) { g_op_err = "tree_softmax: bad arguments"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) { g_op_err = "tree_softmax: no HIP device"; return S.rc; }
    Tree t; if (int r = op_tree(S, "tree_softmax", tree_path, len, t)) return r;
    TreeRows rows{(const float *)S.upload(x, (size_t)n * len * 4), (size_t)n, 1, len, 0, 0};
    float *d_o = (float *)S.alloc((size_t)n * len * 4);
    if (S.rc) { g_op_err = "tree_softmax: allocation failed"; return S.rc; }
    if (!S.ok(launch_tree_softmax(t.dev, rows, temperature, mode, d_o, len, 0, nullptr, nullptr, S.s))) { g_op_err = "tree_softmax: " + S.err; return S.rc; }
    return S.download(out, d_o, (size_t)n * len * 4);
}

int yolo_op_tree_top(const float *x_logits, int n, const char *tree_path, float hier_thresh, int32_t *labels_out, int device)
{
    if (!x_logits || !labels_out || n < 1) { g_op_err = "tree_top: bad arguments"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) { g_op_err = "tree_top: no HIP device"; return S.rc; }
    Tree t; if (int r = op_tree(S, "tree_top", tree_path, -1, t)) return r;
    TreeRows rows{(const float *)S.upload(x_logits, (size_t)n * t.n * 4), (size_t)n, 1, t.n, 0, 0};
    int *d_l = (int *)S.alloc((size_t)n * 4);
    if (S.rc) { g_op_err = "tree_top: allocation failed"; return S.rc; }
    if (!S.ok(launch_tree_top(t.dev, rows, hier_thresh, d_l, S.s))) { g_op_err = "tree_top: " + S.err; return S.rc; }
    return S.download(labels_out, d_l, (size_t)n * 4);
}

int yolo_op_resize_u8_hw(const uint8_t *img, int h, int w, int out_h, int out_w, float post_scale, float *out, int device)
{
    if (!img || !out || h < 1 || w < 1 || out_h < 1 || out_w < 1 || (size_t)out_h * out_w > 0x7fffffffull) return YOLO_ERR_INVALID;
    OpScope S(device); if (S.rc) return S.rc;
    uint8_t *d_i = (uint8_t *)S.upload(img, (size_t)h * w * 3); float *d_o = (float *)S.alloc((size_t)out_h * out_w * 3 * 4);
    if (S.rc) return S.rc;
    if (!S.ok(launch_resize_u8(d_i, h, w, out_h, out_w, d_o, 1, 3, 3, S.s, post_scale))) { g_op_err = S.err; return S.rc; }
    return S.download(out, d_o, (size_t)out_h * out_w * 3 * 4);
}

int yolo_op_resize_u8(const uint8_t *img, int h, int w, int s, float post_scale, float *out, int device)
{
    return yolo_op_resize_u8_hw(img, h, w, s, s, post_scale, out, device);
}

int yolo_op_resize_cv2(const uint8_t *img, int h, int w, int oh, int ow, int swap_rb, float divisor, float *out, int device)
{
    if (!img || !out || h < 1 || w < 1 || oh < 1 || ow < 1 || !(divisor != 0.f)) { g_op_err = "resize_cv2: bad arguments"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) return S.rc;
    uint8_t *d_i = (uint8_t *)S.upload(img, (size_t)h * w * 3); float *d_o = (float *)S.alloc((size_t)oh * ow * 3 * 4);
    if (S.rc) return S.rc;
    if (!S.ok(launch_resize_cv2_u8(d_i, h, w, oh, ow, swap_rb, divisor, d_o, S.s))) { g_op_err = S.err; return S.rc; }
    return S.download(out, d_o, (size_t)oh * ow * 3 * 4);
}

int yolo_op_frame_to_rgb(const yolo_frame_desc *desc, const uint8_t *pixels, size_t bytes, uint8_t *rgb_out, int device)
{
    if (!desc || !pixels || !rgb_out) { g_op_err = "frame_to_rgb: desc / pixels / rgb_out == NULL"; return YOLO_ERR_INVALID; }
    if (int r = frame_desc_check(*desc, bytes, 0, g_op_err)) { g_op_err = "frame_to_rgb: " + g_op_err; return r; }
    OpScope S(device); if (S.rc) { g_op_err = "frame_to_rgb: no HIP device"; return S.rc; }
    FrameDesc f; memcpy(&f, desc, sizeof f);
    const size_t out_bytes = (size_t)f.h * f.w * 3;
    uint8_t *d_i = (uint8_t *)S.upload(pixels, bytes), *d_o = (uint8_t *)S.alloc(out_bytes);
    if (S.rc) { g_op_err = "frame_to_rgb: allocation failed"; return S.rc; }
    if (!S.ok(launch_frame_to_rgb(d_i, bytes, f, d_o, S.s))) { g_op_err = "frame_to_rgb: " + S.err; return S.rc; }
    return S.download(rgb_out, d_o, out_bytes);
}

// one JPEG file through the device stages: host entropy decode, k_jpeg_idct into a surface of its planes, k_frame_to_rgb over the frame those planes are
int yolo_op_jpeg_to_rgb(const uint8_t *file, size_t bytes, uint8_t *rgb_out, int device)
{
    if (!file || !rgb_out) { g_op_err = "jpeg_to_rgb: file / rgb_out == NULL"; return YOLO_ERR_INVALID; }
    JpegFile jf;
    if (int r = jpeg_parse(file, bytes, 0, &jf, g_op_err)) return r;
    yolo_frame_desc d; JpegPlane rows[3]; size_t surface = 0, block = 0;
    jpeg_place(jf, surface, block, &d, rows);
    if (surface > 0xffffffffull) { g_op_err = "jpeg_to_rgb: file 0: its component planes pass 2^32 - 1 bytes"; return YOLO_ERR_UNSUPPORTED; }
    std::vector<int16_t> coef;
    try { coef.resize(jf.blocks * 64); } catch (const std::bad_alloc &) { g_op_err = "jpeg_to_rgb: file 0: no memory for its blocks"; return YOLO_ERR_NOMEM; }
    if (int r = jpeg_decode(file, bytes, 0, jf, coef.data(), g_op_err)) return r;
    if (int r = frame_desc_check(d, surface, 0, g_op_err)) { g_op_err = "jpeg_to_rgb: " + g_op_err; return r; }
    OpScope S(device); if (S.rc) { g_op_err = "jpeg_to_rgb: no HIP device"; return S.rc; }
    FrameDesc f; memcpy(&f, &d, sizeof f);
    const size_t out_bytes = (size_t)f.h * f.w * 3;
    const int16_t *d_c = (const int16_t *)S.upload(coef.data(), coef.size() * 2);
    const JpegPlane *d_t = (const JpegPlane *)S.upload(rows, (size_t)jf.comps * sizeof(JpegPlane));
    uint8_t *d_p = (uint8_t *)S.alloc(surface), *d_o = (uint8_t *)S.alloc(out_bytes);
    if (S.rc) { g_op_err = "jpeg_to_rgb: allocation failed"; return S.rc; }
    if (!S.ok(launch_jpeg_idct(d_c, d_t, jf.comps, jf.blocks, d_p, surface, S.s))) { g_op_err = "jpeg_to_rgb: IDCT: " + S.err; return S.rc; }
    if (!S.ok(launch_frame_to_rgb(d_p, surface, f, d_o, S.s))) { g_op_err = "jpeg_to_rgb: " + S.err; return S.rc; }
    return S.download(rgb_out, d_o, out_bytes);
}

// one JPEG file through the device's entropy stage: interval scan, upload, k_jpeg_entropy, read-back.  A file the scan does not find eligible, or
// one with a failed or doubtful interval, is the host stage's: its coefficients, or its refusal
int yolo_op_jpeg_entropy(const uint8_t *file, size_t bytes, int16_t *coef_out, size_t cap_blocks, int device)
{
    if (!file || !coef_out) { g_op_err = "jpeg_entropy: file / coef_out == NULL"; return YOLO_ERR_INVALID; }
    JpegFile jf;
    if (int r = jpeg_parse(file, bytes, 0, &jf, g_op_err)) return r;
    if (!jf.restart) { g_op_err = "jpeg_entropy: file 0: no restart interval (DRI): the device's entropy stage decodes restart intervals"; return YOLO_ERR_UNSUPPORTED; }
    if (cap_blocks < jf.blocks) { g_op_err = "jpeg_entropy: file 0: its " + std::to_string(jf.blocks) + " blocks do not fit coef_out's " + std::to_string(cap_blocks); return YOLO_ERR_INVALID; }
    std::vector<JpegInterval> iv; JpegEntropyPlan P; std::vector<uint32_t> status;
    bool eligible = false;
    try { eligible = jpeg_intervals(file, bytes, jf, iv); if (eligible) { P.add(jf, bytes, iv, 0); status.resize(P.iv.size()); } }
    catch (const std::bad_alloc &) { g_op_err = "jpeg_entropy: file 0: no memory for its intervals"; return YOLO_ERR_NOMEM; }
    if (!eligible) return jpeg_decode(file, bytes, 0, jf, coef_out, g_op_err);
    OpScope S(device); if (S.rc) { g_op_err = "jpeg_entropy: no HIP device"; return S.rc; }
    const size_t slots = P.iv.size();
    uint8_t *d_s = (uint8_t *)S.alloc(P.stream_bytes);
    const JpegDevFile *d_f = (const JpegDevFile *)S.upload(P.files.data(), sizeof(JpegDevFile));
    const uint32_t *d_w = (const uint32_t *)S.upload(P.wg_file.data(), P.wg_file.size() * 4);
    const JpegInterval *d_i = (const JpegInterval *)S.upload(P.iv.data(), slots * sizeof(JpegInterval));
    int16_t *d_c = (int16_t *)S.alloc(jf.blocks * 128); uint32_t *d_st = (uint32_t *)S.alloc(slots * 4);
    if (S.rc) { g_op_err = "jpeg_entropy: allocation failed"; return S.rc; }
    if (!S.ok(hipMemcpyAsync(d_s, file, bytes, hipMemcpyHostToDevice, S.s))) { g_op_err = "jpeg_entropy: " + S.err; return S.rc; }
    if (!S.ok(launch_jpeg_entropy(d_s, P.stream_bytes, d_f, 1, d_w, d_i, slots, d_c, jf.blocks, d_st, S.s))) { g_op_err = "jpeg_entropy: " + S.err; return S.rc; }
    if (S.download(status.data(), d_st, slots * 4) || S.download(coef_out, d_c, jf.blocks * 128)) { g_op_err = "jpeg_entropy: " + std::string(hipGetErrorString(hipGetLastError())); return S.rc; }
    for (uint32_t st : status) if (st) return jpeg_decode(file, bytes, 0, jf, coef_out, g_op_err);
    return YOLO_OK;
}

int yolo_op_letterbox(const float *image_chw, int iw, int ih, int w, int h, int embed, float *out_chw, int device)
{
    if (!image_chw || !out_chw || iw < 1 || ih < 1 || w < 1 || h < 1) { g_op_err = "letterbox: bad arguments"; return YOLO_ERR_INVALID; }
    OpScope S(device); if (S.rc) { g_op_err = "letterbox: no HIP device"; return S.rc; }
    float *d_i = (float *)S.upload(image_chw, (size_t)iw * ih * 3 * 4), *d_o = (float *)S.alloc((size_t)w * h * 3 * 4);
    if (S.rc) return S.rc;
    if (!S.ok(launch_letterbox_planar(d_i, iw, ih, w, h, embed, d_o, S.s))) { g_op_err = S.err; return S.rc; }
    return S.download(out_chw, d_o, (size_t)w * h * 3 * 4);
}

int yolo_op_decode_hw(const float *raw, int n, int gh, int gw, int na, int classes, const float *anchors_wh, int img_h, int img_w, int decode,
                      int region, float *out, int device)
{
    if (!raw || !out || !anchors_wh || na < 1 || na > 16 || gh < 1 || gw < 1) return YOLO_ERR_INVALID;
    OpScope S(device); if (S.rc) return S.rc;
    const int attrs = 5 + classes; const size_t cnt = (size_t)n * gh * gw * na * attrs;
    float *d_r = (float *)S.upload(raw, cnt * 4), *d_o = (float *)S.alloc(cnt * 4);
    if (S.rc) return S.rc;
    DecodeArgs d; memset(&d, 0, sizeof d);
    d.raw = d_r; d.raw_stride = na * attrs; d.n = n; d.gh = gh; d.gw = gw; d.na = na; d.classes = classes; d.img_h = img_h; d.img_w = img_w; d.mode = decode; d.region = region;
    const int stride[2] = {img_w / gw, img_h / gh};          // along x (anchor widths), along y (anchor heights)
    for (int k = 0; k < 2 * na; ++k) d.anchors[k] = region ? anchors_wh[k] : (float)(1.0 * (double)anchors_wh[k] / (double)stride[k & 1]);
    d.det = d_o; d.rows_total = gh * gw * na; d.row_off = 0; d.reject_below = -INFINITY;
    if (!S.ok(launch_decode(d, nullptr, nullptr, S.s))) { g_op_err = S.err; return S.rc; }
    return S.download(out, d_o, cnt * 4);
}

int yolo_op_decode(const float *raw, int n, int g, int na, int classes, const float *anchors_wh, int img_size, int decode,
                   int region, float *out, int device)
{
    return yolo_op_decode_hw(raw, n, g, g, na, classes, anchors_wh, img_size, img_size, decode, region, out, device);
}

int yolo_op_detections_boxes(const float *det, int n, int rows, int attrs, float *out, int device)
{
    if (!det || !out || n < 1 || rows < 1 || attrs < 5) return YOLO_ERR_INVALID;
    OpScope S(device); if (S.rc) return S.rc;
    const size_t cnt = (size_t)n * rows * attrs;
    float *d_i = (float *)S.upload(det, cnt * 4), *d_o = (float *)S.alloc(cnt * 4);
    if (S.rc) return S.rc;
    if (!S.ok(launch_boxes_to_corners(d_i, d_o, (size_t)n * rows, attrs, S.s))) { g_op_err = S.err; return S.rc; }
    return S.download(out, d_o, cnt * 4);
}

int yolo_op_nms_detections(const float *boxes_xywh, float *prob, float *objectness, int n, int classes, float thresh, int by_objectness, int device)
{
    if (n == 0) return YOLO_OK;
    if (!boxes_xywh || !prob || !objectness || n < 0 || classes < 1) { g_op_err = "nms_detections: bad arguments"; return YOLO_ERR_INVALID; }
    if (n > 4096) { g_op_err = "nms_detections: more than 4096 detections"; return YOLO_ERR_UNSUPPORTED; }
    OpScope S(device); if (S.rc) { g_op_err = "nms_detections: no HIP device"; return S.rc; }
    float4 *d_b = (float4 *)S.upload(boxes_xywh, (size_t)n * 16);
    float *d_p = (float *)S.upload(prob, (size_t)n * classes * 4), *d_o = (float *)S.upload(objectness, (size_t)n * 4);
    if (S.rc) return S.rc;
    if (!S.ok(launch_nms_dets(d_b, d_p, d_o, n, classes, thresh, by_objectness ? 1 : 0, S.s))) { g_op_err = S.err; return S.rc; }
    S.download(prob, d_p, (size_t)n * classes * 4);
    return S.download(objectness, d_o, (size_t)n * 4);
}

int yolo_op_postprocess_rows(const float *det, int n, int rows, int attrs, float score_thr, float iou_thr, int max_out, int nms_mode,
                             int select_mode, yolo_box *boxes_out, int32_t *counts_out, int32_t *rows_out, int device)
{
    if (!det || !boxes_out || !counts_out || n < 1 || rows < 1 || rows > 32768 || attrs < 6 || max_out < 1) return YOLO_ERR_INVALID;
    OpScope S(device); if (S.rc) return S.rc;
    size_t nr = (size_t)n * rows; int p2 = 1; while (p2 < rows) p2 <<= 1;
    PostArgs p; memset(&p, 0, sizeof p);
    p.det = (const float *)S.upload(det, nr * attrs * 4); p.n = n; p.rows = rows; p.attrs = attrs; p.score_thr = score_thr; p.iou_thr = iou_thr;
    p.max_out = max_out; p.nms_mode = nms_mode & 0xff; p.select_mode = select_mode & 0xff; p.corners_in = (select_mode >> 8) & 1;
    // bits 8.. of nms_mode carry the image size for the V2 numpy flavour: (h << 8) | (w << 20)
    p.img_h = (nms_mode >> 8) & 0xfff; p.img_w = (nms_mode >> 20) & 0xfff;
    p.scores = (float *)S.alloc(nr * 4); p.labels = (int *)S.alloc(nr * 4); p.cand = (int *)S.alloc(nr * 4);
    p.keys = (unsigned long long *)S.alloc((size_t)n * p2 * 8); p.rows_pow2 = p2;
    p.sbox = (float4 *)S.alloc(nr * 16); p.slabel = (int *)S.alloc(nr * 4); p.sscore = (float *)S.alloc(nr * 4);
    p.boxes_out = S.alloc((size_t)n * max_out * sizeof(yolo_box)); p.counts_out = (int *)S.alloc((size_t)n * 4);
    if (rows_out) { p.srow = (int *)S.alloc(nr * 4); p.rows_out = (int *)S.alloc((size_t)n * max_out * 4); }
    if (S.rc) return S.rc;
    if (!S.ok(launch_postprocess(p, S.s))) { g_op_err = S.err; return S.rc; }
    S.download(boxes_out, p.boxes_out, (size_t)n * max_out * sizeof(yolo_box));
    if (rows_out) S.download(rows_out, p.rows_out, (size_t)n * max_out * 4);
    return S.download(counts_out, p.counts_out, (size_t)n * 4);
}

int yolo_op_postprocess(const float *det, int n, int rows, int attrs, float score_thr, float iou_thr, int max_out, int nms_mode,
                        int select_mode, yolo_box *boxes_out, int32_t *counts_out, int device)
{
    return yolo_op_postprocess_rows(det, n, rows, attrs, score_thr, iou_thr, max_out, nms_mode, select_mode, boxes_out, counts_out, nullptr, device);
}

}  // extern "C"
