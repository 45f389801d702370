// Parameters of libyolo_hip.so: batch-norm fold, filter packing (bf16 / fp16 / e4m3 / fp32 layouts), fp8 activation scales, the Darknet
// weight stream and the export artifact (8f-3).
#include "yolo_ctx.h"

namespace yolo_impl {

uint16_t f2bf(float f)
{
    uint32_t u; memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// float -> IEEE binary16 bits: round to nearest even, saturating at +-65504 (as the device's conversions do), NaN stays NaN
uint16_t f2h(float f)
{
    uint32_t u; memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    if (f != f) return (uint16_t)(sign | 0x7e00u);
    float a = fabsf(f);
    if (a >= 65504.f) return (uint16_t)(sign | 0x7bffu);
    if (a < ldexpf(1.f, -24) * 0.5f) return sign;                       // below half the smallest subnormal (ties to even: zero)
    int e; frexpf(a, &e); e -= 1;                                         // a in [2^e, 2^(e+1))
    if (e < -14) e = -14;                                                 // subnormals share the first binade's quantum
    const float quantum = ldexpf(1.f, e - 10);
    const float q = nearbyintf(a / quantum);                              // exact division, RNE under the default rounding mode
    const float v = q * quantum;
    if (v < ldexpf(1.f, -14)) return (uint16_t)(sign | (uint16_t)q);      // subnormal: q in 0..1023
    int e2; frexpf(v, &e2); e2 -= 1;
    const int m = (int)((v / ldexpf(1.f, e2) - 1.f) * 1024.f);
    return (uint16_t)(sign | ((e2 + 15) << 10) | m);
}

// float -> OCP e4m3 (e4m3fn) code: round to nearest even, saturate at +-448, NaN -> 0x7f
uint8_t f2e4m3(float f)
{
    uint32_t u; memcpy(&u, &f, 4);
    const uint8_t sign = (uint8_t)((u >> 31) << 7);
    if (f != f) return (uint8_t)(sign | 0x7f);
    float a = fabsf(f);
    if (a >= 448.f) return (uint8_t)(sign | 0x7e);
    int e; frexpf(a, &e); e -= 1;                          // a in [2^e, 2^(e+1))
    if (a == 0.f || e < -6) e = -6;                        // subnormal range shares the quantum of the first binade
    const float quantum = ldexpf(1.f, e - 3);
    const float q = nearbyintf(a / quantum);               // RNE under the default rounding mode; exact division
    const float v = q * quantum;
    if (v < ldexpf(1.f, -6)) return (uint8_t)(sign | (uint8_t)q);          // q in 0..7 (q == 8 is the first normal)
    int e2; frexpf(v, &e2); e2 -= 1;
    const int m = (int)((v / ldexpf(1.f, e2) - 1.f) * 8.f);
    return (uint8_t)(sign | ((e2 + 7) << 3) | m);
}

// fold + pack one conv's parameters (host).  w_oihw: [cout][cin][k][k].  wdt: element type of the packed filters.
// fp8: `in_scale` (per input channel, or null = 1) is folded into the filters first, then every output channel c is
// scaled so that its largest |w| maps to 448: code = e4m3(w * in_scale / osc[c]), osc[c] = max|w * in_scale| / 448.
// IEEE binary16 bits -> float (exact)
float h2f(uint16_t h)
{
    const int e = (h >> 10) & 31, m = h & 1023;
    float v = e == 0 ? ldexpf((float)m, -24) : e == 31 ? (m ? NAN : INFINITY) : ldexpf((float)(m | 1024), e - 25);
    return (h & 0x8000) ? -v : v;
}

// Batch norm as a per-filter scale (folded into the filters, or an xnor conv's epilogue scale) and bias.  TF: epsilon inside the sqrt
// (V3/yolo_v3.py:9).  darknet semantics follow the reference's CPU normalize (DN/blas.c:154: (x - mean) / (sqrt(var) + .000001f)), the code
// oracle/_ref is compiled from
static void fold_bn(int n, const float *beta, const float *gamma, const float *mean, const float *var, int semantics, float *scale, float *bias)
{
    for (int o = 0; o < n; ++o) {
        const float s = semantics == YOLO_SEM_DARKNET ? gamma[o] / (sqrtf(var[o]) + 1e-6f) : gamma[o] / sqrtf(var[o] + 1e-5f);
        scale[o] = s; bias[o] = beta[o] - mean[o] * s;
    }
}
// ... of a conv's parameter block [beta gamma mean var], or (bn == 0) its [bias]: scale 1
static void fold_bn(int bn, int n, const float *bn_or_bias, int semantics, float *scale, float *bias)
{
    if (bn) return fold_bn(n, bn_or_bias, bn_or_bias + n, bn_or_bias + 2 * (size_t)n, bn_or_bias + 3 * (size_t)n, semantics, scale, bias);
    for (int o = 0; o < n; ++o) { scale[o] = 1.f; bias[o] = bn_or_bias[o]; }
}

// filter element idx of a buffer of fp32 / fp16 / bf16 filters
static void put_elt(std::vector<uint8_t> &wbuf, size_t idx, float v, int dt)
{
    if (dt == DT_F32) { memcpy(&wbuf[idx * 4], &v, 4); return; }
    const uint16_t b = dt == DT_F16 ? f2h(v) : f2bf(v);
    memcpy(&wbuf[idx * 2], &b, 2);
}

void pack_conv(const Layer &L, const float *bn_or_bias, const float *w_oihw, int wdt, const float *in_scale,
               std::vector<uint8_t> &wbuf, std::vector<float> &bias, std::vector<float> &osc, int semantics, int split)
{
    const int n = L.filters, k = L.size, cin = L.cin;
    bias.assign(L.cout_pad, 0.f); osc.assign(L.cout_pad, 1.f);
    std::vector<float> scale(n);
    fold_bn(L.bn, n, bn_or_bias, semantics, scale.data(), bias.data());
    const size_t es = dt_size(wdt);
    wbuf.assign((size_t)L.cout_pad * L.kpad * es, 0);
    std::vector<float> row((size_t)cin * k * k);
    for (int o = 0; o < n; ++o) {
        float amax = 0.f;
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < k * k; ++t) {
                float v = w_oihw[((size_t)o * cin + ci) * k * k + t] * scale[o];
                if (wdt == DT_FP8 && in_scale) v *= in_scale[ci];
                row[(size_t)ci * k * k + t] = v; amax = std::max(amax, fabsf(v));
            }
        if (wdt == DT_FP8) osc[o] = amax > 0.f ? amax / FP8_MAX : 1.f;
        const int kc = conv_kchunk(L.cin_pad, wdt);                              // K order: see conv_igemm.hip `stage`
        for (int ci = 0; ci < cin; ++ci)
            for (int t = 0; t < k * k; ++t) {
                const float v = row[(size_t)ci * k * k + t];
                if (split == 2) {
                    // split fp16 (YOLO_FP16X2), the input is an interleaved pair tensor (pair K loop): per 32-channel group and tap one 64-element
                    // K-step row W_hi 32 | W_lo 32 -- k = ((ci / 32) * k * k + t) * 64 + ci % 32 (+ 32 for the low half)
                    const uint16_t h = f2h(v); const uint16_t l = f2h(v - h2f(h));
                    const size_t idx = (size_t)o * L.kpad + ((size_t)(ci / 32) * k * k + t) * 64 + ci % 32;
                    memcpy(&wbuf[idx * 2], &h, 2); memcpy(&wbuf[(idx + 32) * 2], &l, 2);
                    continue;
                }
                if (split) {
                    // ... the input is the network image, three blocks hi | lo | hi of its 8 padded channels (plain K loop over 3 * Cp 'channels'):
                    // the filter row holds W_hi | W_hi | W_lo
                    const int Cp = L.cin_pad / 3;
                    const uint16_t h = f2h(v); const uint16_t l = f2h(v - h2f(h));
                    for (int blk = 0; blk < 3; ++blk) {
                        const int cv = blk * Cp + ci;
                        const size_t idx = (size_t)o * L.kpad + ((size_t)(cv / kc) * k * k + t) * kc + cv % kc;
                        memcpy(&wbuf[idx * 2], blk < 2 ? &h : &l, 2);
                    }
                    continue;
                }
                const size_t idx = (size_t)o * L.kpad + ((size_t)(ci / kc) * k * k + t) * kc + ci % kc;     // t = kh * k + kw
                if (wdt == DT_FP8) wbuf[idx] = f2e4m3(v / osc[o]);
                else put_elt(wbuf, idx, v, wdt);
            }
    }
}

// [deconvolutional]: batch norm folded as pack_conv folds it, then one filter block per output phase (DeconvArgs, kernels.h): phase
// (py, px) holds the taps kh = py + ty * stride, kw = px + tx * stride as rows [cout_pad][kp], k = (ty * taps(px) + tx) * cin_pad + ci
void pack_deconv(const Layer &L, const float *bn_or_bias, const float *w_iohw, int wdt, std::vector<uint8_t> &wbuf, std::vector<float> &bias, int semantics)
{
    const int n = L.filters, k = L.size, cin = L.cin, st = L.stride;
    DeconvArgs g = deconv_geometry(k, st, L.pad, 1, 1, L.cin_pad, n, ACT_LINEAR, wdt);
    bias.assign(g.cout_pad, 0.f);
    std::vector<float> scale(n);
    fold_bn(L.bn, n, bn_or_bias, semantics, scale.data(), bias.data());
    wbuf.assign(deconv_layout(g) * dt_size(wdt), 0);
    for (int kh = 0; kh < k; ++kh) for (int kw = 0; kw < k; ++kw) {
        const int py = kh % st, px = kw % st, phase = py * st + px, tap = (kh / st) * deconv_taps(px, k, st) + kw / st;
        for (int o = 0; o < n; ++o) for (int ci = 0; ci < cin; ++ci) {
            const float v = w_iohw[(((size_t)ci * n + o) * k + kh) * k + kw] * scale[o];
            put_elt(wbuf, (size_t)g.woff[phase] + (size_t)o * g.kp[phase] + (size_t)tap * L.cin_pad + ci, v, wdt);
        }
    }
}

// [convolutional] with groups > 1: batch norm folded as pack_conv folds it, then the bundle layout (GConvArgs, kernels.h): filter o of group
// g = o / m lies in bundle g / t as row o (the bundles' rows are the output channels in order), its channel ci of tap (ky, kx) at column
// (ky * size + kx) * kc + (g % t) * cg + ci; every other entry of the row is zero.  fp32: no bundling, column (ky * size + kx) * cg + ci
void pack_gconv(const Layer &L, const float *bn_or_bias, const float *w_oihw, int wdt, std::vector<uint8_t> &wbuf, std::vector<float> &bias, int semantics)
{
    const int n = L.filters, k = L.size;
    GConvArgs g = gconv_geometry(k, L.stride, L.pad, 1, 1, L.cin, n, L.groups, ACT_LINEAR, wdt);
    bias.assign((size_t)g.nb * g.mb, 0.f);
    std::vector<float> scale(n);
    fold_bn(L.bn, n, bn_or_bias, semantics, scale.data(), bias.data());
    wbuf.assign(gconv_layout(g) * dt_size(wdt), 0);
    for (int o = 0; o < n; ++o) {
        const int gi = wdt == DT_F32 ? 0 : (o / g.m) % g.t;          // (fp32 rows hold the group's own channels only)
        for (int ci = 0; ci < g.cg; ++ci) for (int tap = 0; tap < k * k; ++tap) {
            const float v = w_oihw[((size_t)o * g.cg + ci) * k * k + tap] * scale[o];
            put_elt(wbuf, (size_t)o * g.kp + (size_t)tap * g.kc + gi * g.cg + ci, v, wdt);
        }
    }
}

// alpha_f = mean |w_f| of binarize_weights (DN/convolutional_layer.c:28-41) with the bits the reference's BUILD gives it.  The source reads as a float running
// sum in index order and one division; the reference is compiled with -Ofast (its own Makefile's OPTS, and oracle/Makefile), under which the compiler keeps
// four partial sums -- element j in sum j % 4 --, adds them as (s0 + s2) + (s1 + s3), then the elements past the last whole four in order, and multiplies
// by the float reciprocal of the count.  That order is restated here (every one of the 128 filters of the fixtures matches bit for bit; the plain running
// sum differs from it by up to 9 ulp in most of them: NOTEBOOK "XNOR layers")
static float xnor_alpha(const float *w, int n)
{
    float lane[4] = {0.f, 0.f, 0.f, 0.f};
    const int whole = n / 4 * 4;
    for (int j = 0; j < whole; j += 4) for (int q = 0; q < 4; ++q) lane[q] += fabsf(w[j + q]);
    float sum = (lane[0] + lane[2]) + (lane[1] + lane[3]);
    for (int j = whole; j < n; ++j) sum += fabsf(w[j]);
    return sum * (1.0f / (float)n);
}

// [convolutional] with xnor=1 (DN/convolutional_layer.c:28-41 binarize_weights): alpha_f = mean |w_f| as the reference forms it (xnor_alpha), the filters as
// int8 signs (w > 0 ? 1 : -1) in the fragment order of
// XConvArgs (kernels.h), every padded channel, K position and row 0.  The epilogue's scale is alpha_f times the batch-norm scale pack_conv folds
// into the filters, the shift the one it folds into the bias
void pack_xconv(const Layer &L, const float *bn_or_bias, const float *w_oihw, std::vector<uint8_t> &wbuf, std::vector<float> &scale, std::vector<float> &bias, int semantics)
{
    const int n = L.filters, k = L.size, cin = L.cin, per = cin * k * k;
    XConvArgs g = xconv_geometry(k, L.stride, L.pad, 1, 1, cin, n, ACT_LINEAR);
    scale.assign(g.cout_pad, 0.f); bias.assign(g.cout_pad, 0.f);
    wbuf.assign(xconv_layout(g), 0);
    const int ksteps = g.kpad / 64;
    std::vector<float> sc(n);
    fold_bn(L.bn, n, bn_or_bias, semantics, sc.data(), bias.data());
    for (int o = 0; o < n; ++o) {
        const float *w = w_oihw + (size_t)o * per;
        scale[o] = xnor_alpha(w, per) * sc[o];
        for (int ci = 0; ci < cin; ++ci) for (int tap = 0; tap < k * k; ++tap)
            wbuf[xconv_pack_index(o, xconv_k(g, tap, ci), ksteps)] = w[(size_t)ci * k * k + tap] > 0.f ? 1 : 0xff;
    }
}

// one [connected] sublayer of the weight stream (DN/parser.c load_connected_weights: biases, weights [outputs][inputs], then scales, rolling mean,
// rolling variance when batch-normalised) with its batch norm folded into the rows and the bias (DN/connected_layer.c:161 -> batchnorm_layer.c: the
// rolling statistics, scale, then the biases), by pack_conv's rule.  Returns the stream behind it
static const float *read_connected(const float *p, int inputs, int outputs, int bn, int semantics, std::vector<float> &w, std::vector<float> &b)
{
    const float *bias = p, *wf = p + outputs;
    p += (size_t)outputs * (1 + (size_t)inputs);
    w.assign(wf, wf + (size_t)outputs * inputs); b.assign(bias, bias + outputs);
    if (!bn) return p;
    const float *gamma = p, *mean = p + outputs, *var = p + 2 * (size_t)outputs;
    std::vector<float> sc(outputs);
    fold_bn(outputs, bias, gamma, mean, var, semantics, sc.data(), b.data());
    for (int o = 0; o < outputs; ++o) for (int j = 0; j < inputs; ++j) w[(size_t)o * inputs + j] *= sc[o];
    return p + 3 * (size_t)outputs;
}

// [rnn] / [gru] / [lstm]: the sublayers of the stream -> the stacked matrices of the layer's launches (RecurArgs, kernels.h), in fragment order, and
// their bias pairs.  A sublayer over the layer's input has its columns moved from darknet's CHW flattening to the tensor's [pixel][stride] order
static int pack_recurrent(yolo_ctx *c, Layer &L, const float *&p)
{
    const RecurGeom g = recur_geom(c, L);
    const int U = L.filters, hw = L.fc_h * L.fc_w, xs = hw ? g.x_len / hw : 0;
    int subs[8]; const int ns = recur_sublayers(L, subs);
    std::vector<float> w[8], b[8];
    for (int q = 0; q < ns; ++q) p = read_connected(p, subs[q] ? U : L.cin, U, L.bn, c->semantics, w[q], b[q]);
    // per launch and gate: the sublayer over the x part and the one over the h part of K (-1: none)
    int G[2] = {recur_gates(g.mode[0]), recur_gates(g.mode[1])}, sx[2][4] = {}, sh[2][4] = {};
    if (L.rkind == RECUR_LSTM) for (int t = 0; t < 4; ++t) { sx[0][t] = 4 + t; sh[0][t] = t; }          // rows i f o g: ui uf uo ug over x, wi wf wo wg over h
    if (L.rkind == RECUR_GRU) { sx[0][0] = 3; sh[0][0] = 0; sx[0][1] = 4; sh[0][1] = 1; sx[1][0] = 5; sh[1][0] = 2; }      // rows z r: uz ur | wz wr; then uh | wh over r * h
    if (L.rkind == RECUR_RNN) { sx[0][0] = 0; sh[0][0] = 1; sx[1][0] = 2; sh[1][0] = -1; }          // input | self; then output over the new state
    void *dw[2] = {L.d_w, L.d_w2}; float *db[2] = {L.d_b, L.d_b2};
    const size_t es = dt_size(L.in_dt);
    for (int q = 0; q < g.launches; ++q) {
        const int K = g.Kx[q] + g.Kh[q], KS = K / 32;
        std::vector<uint8_t> wbuf((size_t)g.Mp[q] * K * es, 0); std::vector<float> bias((size_t)2 * g.Mp[q], 0.f);
        auto put = [&](int row, int k, float v) { put_elt(wbuf, recur_pack_index(row, k, KS), v, L.in_dt); };
        const bool x_is_input = !(L.rkind == RECUR_RNN && q == 1);
        for (int u = 0; u < U; ++u) for (int t = 0; t < G[q]; ++t) {
            const int row = u * G[q] + t, a = sx[q][t], hpart = sh[q][t];
            bias[row] = b[a][u];
            if (x_is_input) { for (int ch = 0; ch < L.fc_c; ++ch) for (int px = 0; px < hw; ++px) put(row, px * xs + ch, w[a][(size_t)u * L.cin + (size_t)ch * hw + px]); }
            else for (int j = 0; j < U; ++j) put(row, j, w[a][(size_t)u * U + j]);
            if (hpart < 0) continue;
            bias[g.Mp[q] + row] = b[hpart][u];
            for (int j = 0; j < U; ++j) put(row, g.Kx[q] + j, w[hpart][(size_t)u * U + j]);
        }
        HIPCK(c, hipMemcpy(dw[q], wbuf.data(), wbuf.size(), hipMemcpyHostToDevice));
        HIPCK(c, hipMemcpy(db[q], bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
    }
    return YOLO_OK;
}

// the parameter blobs of a layer with state, in the order an artifact holds them: an [rnn] / [gru] / [lstm]'s stacked matrix and bias pair per launch,
// a [crnn]'s filters and bias per conv.  Returns how many (at most 6)
static int state_layer_blobs(const yolo_ctx *c, const Layer &L, void *ptr[6], uint64_t bytes[6])
{
    int n = 0;
    if (L.type == L_CRNN) { for (const Layer &S : L.sub) { ptr[n] = S.d_w; bytes[n++] = (uint64_t)S.cout_pad * S.kpad * dt_size(S.in_dt); ptr[n] = S.d_b; bytes[n++] = (uint64_t)S.cout_pad * 4; } return n; }
    void *all[4] = {L.d_w, L.d_b, L.d_w2, L.d_b2};
    for (int k = 0; k < 4; ++k) if (const size_t b = recur_blob_bytes(c, L, k)) { ptr[n] = all[k]; bytes[n++] = b; }
    return n;
}

// fp8: scale of the tensor each layer's view holds, and per-input-channel scales of a conv
void resolve_scales(yolo_ctx *c)
{
    const int NL = (int)c->layers.size();
    if ((int)c->user_scale.size() != NL) c->user_scale.assign(NL, 1.f);
    c->eff_scale.assign(NL, 1.f);
    for (int i = 0; i < NL; ++i) {
        const Layer &L = c->layers[i];
        switch (L.type) {
        case L_CONV: c->eff_scale[i] = L.store_dt != DT_FP8 ? 1.f : (L.residual_from >= -1 && i + 1 < NL) ? c->user_scale[i + 1] : c->user_scale[i]; break;
        case L_SHORTCUT: c->eff_scale[i] = L.store_dt != DT_FP8 ? 1.f : c->user_scale[i]; break;
        case L_ROUTE: c->eff_scale[i] = L.in.size() == 1 ? c->eff_scale[L.in[0]] : NAN; break;
        case L_UPSAMPLE: case L_MAXPOOL: case L_REORG: c->eff_scale[i] = c->eff_scale[L.in[0]]; break;
        default: break;
        }
    }
}
// scale of every logical channel of layer idx's output (multi-input routes concatenate their sources)
void channel_scales(const yolo_ctx *c, int idx, std::vector<float> &out)
{
    const Layer &L = c->layers[idx];
    if (L.type == L_ROUTE && L.in.size() > 1) { for (int j : L.in) channel_scales(c, j, out); return; }
    if (L.type == L_REORG) {             // channel order is scrambled but every source channel has the same scale
        std::vector<float> src; channel_scales(c, L.in[0], src);
        for (int k = 0; k < L.C; ++k) out.push_back(src[0]);
        return;
    }
    if (L.type == L_ROUTE || L.type == L_UPSAMPLE || L.type == L_MAXPOOL) { channel_scales(c, L.in[0], out); return; }
    for (int k = 0; k < L.C; ++k) out.push_back(c->eff_scale[idx]);
}

// The fused 1x1 tail (conv_igemm_kernel.h) reads its filters as MFMA A fragments straight from global memory: lane (l15, lq) of a wave
// takes the 16 bytes at k = (kk * 4 + lq) * 8 of row ct2 * 16 + l15.  From the [row][K] image one such wave-load touches sixteen
// 64-byte pieces 2 * K bytes apart, and every workgroup of the layer asks for the same 64 KB at the same moment; a copy in fragment
// order -- [channel tile][K step][lane][8 bf16] -- makes each wave-load one contiguous KiB.  Built from the packed filters already on
// the device, so both ways of loading parameters (weight stream, export artifact) share it.
// rows [0, rows) of a 16-bit [row][K] filter image in fragment order: [row / 16][K / 32][64 lanes][8 elements] (rows a multiple of 16, K of 32)
void fragment_order(const uint16_t *src, int rows, int K, uint16_t *dst)
{
    const int K2S = K / 32;
    for (int ct2 = 0; ct2 < rows / 16; ++ct2)
        for (int kk = 0; kk < K2S; ++kk)
            for (int lane = 0; lane < 64; ++lane)
                memcpy(&dst[(((size_t)ct2 * K2S + kk) * 64 + lane) * 8], &src[(size_t)(ct2 * 16 + (lane & 15)) * K + (kk * 4 + (lane >> 4)) * 8], 16);
}

// The free-running halo forms (conv_igemm_kernel.h FRAGW) read the filters of their main K loop the same way: every 16-bit 3x3 / stride 1 /
// pad 1 conv over whole 64-channel chunks -- what such an id can run (conv_halo13.hip halo_ok; the spatial size is the launch's business) --
// gets a second image of ALL its packed rows in fragment order.  The rows past the filters are the packed image's own zero rows, the K order
// is the packed image's (chunk-major), so fragment (ct, kt, kk) holds exactly what the LDS path reads at wrow(i) + sw0 / sw1 of K-step kt.
bool wants_filter_fragments(const yolo_ctx *c, const Layer &L)
{
    return c->fragw && !c->split() && L.type == L_CONV && (L.in_dt == DT_BF16 || L.in_dt == DT_F16) && !L.head && !L.fc && !L.s2d7 &&
           L.size == 3 && L.stride == 1 && L.pad == 1 && L.cin_pad % 64 == 0 && L.kpad == 9 * L.cin_pad && L.cout_pad % 16 == 0;
}
int filter_fragments(yolo_ctx *c)
{
    std::vector<uint16_t> src, dst;
    for (auto &L : c->layers) {
        if (!wants_filter_fragments(c, L)) continue;
        src.resize((size_t)L.cout_pad * L.kpad); dst.resize(src.size());
        HIPCK(c, hipMemcpy(src.data(), L.d_w, src.size() * 2, hipMemcpyDeviceToHost));
        fragment_order(src.data(), L.cout_pad, L.kpad, dst.data());
        if (!L.d_wfrag) HIPCK(c, hipMalloc(&L.d_wfrag, dst.size() * 2));
        HIPCK(c, hipMemcpy(L.d_wfrag, dst.data(), dst.size() * 2, hipMemcpyHostToDevice));
    }
    return YOLO_OK;
}

int tail_fragments(yolo_ctx *c)
{
    std::vector<uint16_t> src, dst;
    for (auto &T : c->layers) {
        if (T.type != L_CONV || T.fused_into < 0) continue;
        if (T.in_dt != DT_BF16 && T.in_dt != DT_F16) continue;          // (16-bit tails only; also the bf16 islands of a mixed e4m3 plan)
        // K == the producer's channel count, a multiple of 32.  A HEAD tail is read by all eight waves, 32 rows each, whatever its filter count
        // (conv_igemm_kernel.h, head mode: t2g = wave_id): its fragment image is always the padded 256 rows, the rows past the filters zero
        // (18 filters of a 1-class head, 75 of a VOC head: ADVICE r05 -- the short image was read past its end).
        const int C2 = T.head ? T.cout_pad : roundup(T.filters, 16), K = T.kpad;
        if (C2 > T.cout_pad || K % 32 || (T.head && T.cout_pad < 256)) continue;
        src.resize((size_t)T.cout_pad * K); dst.assign((size_t)C2 * K, 0);
        HIPCK(c, hipMemcpy(src.data(), T.d_w, src.size() * 2, hipMemcpyDeviceToHost));
        fragment_order(src.data(), C2, K, dst.data());
        if (!T.d_wf) HIPCK(c, hipMalloc(&T.d_wf, dst.size() * 2));
        HIPCK(c, hipMemcpy(T.d_wf, dst.data(), dst.size() * 2, hipMemcpyHostToDevice));
    }
    return YOLO_OK;
}

}  // namespace yolo_impl

extern "C" {

int yolo_set_act_scales(yolo_ctx *c, const float *scales, int n)
{
    if (!c) return YOLO_ERR_INVALID;
    if (c->dtype != YOLO_FP8) return fail(c, YOLO_ERR_STATE, "activation scales only exist in the fp8 configuration");
    if (!scales || n != (int)c->layers.size()) return fail(c, YOLO_ERR_INVALID, "need one scale per layer (%zu)", c->layers.size());
    for (int i = 0; i < n; ++i) if (!(scales[i] > 0.f) || !std::isfinite(scales[i])) return fail(c, YOLO_ERR_INVALID, "layer %d: scale must be finite and > 0", i);
    c->user_scale.assign(scales, scales + n);
    resolve_scales(c);
    c->weights_loaded = false;           // filters absorb the input scales: they have to be packed again
    drop_graph(c);
    return YOLO_OK;
}

int yolo_set_weights(yolo_ctx *c, const float *flat, size_t n)
{
    if (!c) return YOLO_ERR_INVALID;
    if (!flat) return fail(c, YOLO_ERR_INVALID, "weights == NULL");
    if (n != c->weights_count) return fail(c, YOLO_ERR_IO, "weights stream has %zu floats, topology needs %zu", n, c->weights_count);
    HIPCK(c, hipSetDevice(c->device));
    const float *p = flat;
    std::vector<uint8_t> wbuf; std::vector<float> bias, osc;
    resolve_scales(c);
    for (auto &L : c->layers) {
        if (L.type == L_LOCAL) {
            // file: biases [filter][location], weights [location][filter][c][kh][kw] (DN/parser.c:1315-1320) -> device: bias [location][filter],
            // weights [location][filter][kh][kw][c] in the activations' type
            const int loc = L.H * L.W, F = L.filters, k = L.size, C = L.cin;
            const float *bfile = p; p += (size_t)F * loc;
            const float *wfile = p; p += (size_t)loc * F * C * k * k;
            std::vector<float> b((size_t)loc * F);
            for (int f = 0; f < F; ++f) for (int l = 0; l < loc; ++l) b[(size_t)l * F + f] = bfile[(size_t)f * loc + l];
            const size_t es = dt_size(L.in_dt);
            std::vector<uint8_t> wb((size_t)loc * F * k * k * C * es);
            for (size_t lf = 0; lf < (size_t)loc * F; ++lf)
                for (int ch = 0; ch < C; ++ch)
                    for (int t = 0; t < k * k; ++t) put_elt(wb, (lf * k * k + t) * C + ch, wfile[(lf * C + ch) * k * k + t], L.in_dt);
            HIPCK(c, hipMemcpy(L.d_w, wb.data(), wb.size(), hipMemcpyHostToDevice));
            HIPCK(c, hipMemcpy(L.d_b, b.data(), b.size() * 4, hipMemcpyHostToDevice));
            continue;
        }
        if (is_side_conv(L)) {          // the file: as a conv's, [bias | beta gamma mean var] then the filters (DN/parser.c load_convolutional_weights: l.nweights, cin / groups channels per filter)
            const float *params = p; p += (size_t)L.filters * (L.bn ? 4 : 1);
            const float *w = p; p += (size_t)L.filters * (L.cin / L.groups) * L.size * L.size;
            if (L.type == L_DECONV) pack_deconv(L, params, w, L.in_dt, wbuf, bias, c->semantics);
            else if (L.type == L_GCONV) pack_gconv(L, params, w, L.in_dt, wbuf, bias, c->semantics);
            else pack_xconv(L, params, w, wbuf, osc, bias, c->semantics);
            HIPCK(c, hipMemcpy(L.d_w, wbuf.data(), wbuf.size(), hipMemcpyHostToDevice));
            HIPCK(c, hipMemcpy(L.d_b, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
            if (L.d_sc) HIPCK(c, hipMemcpy(L.d_sc, osc.data(), osc.size() * 4, hipMemcpyHostToDevice));
            continue;
        }
        if (L.type == L_RECUR) { if (int rc = pack_recurrent(c, L, p)) return rc; continue; }
        if (L.type == L_CRNN) {          // input, self, output: three convs in a conv's own file layout
            for (Layer &S : L.sub) {
                const float *params = p; p += (size_t)S.filters * (S.bn ? 4 : 1);
                const float *w = p; p += (size_t)S.filters * S.cin * 9;
                pack_conv(S, params, w, S.in_dt, nullptr, wbuf, bias, osc, c->semantics, 0);
                HIPCK(c, hipMemcpy(S.d_w, wbuf.data(), wbuf.size(), hipMemcpyHostToDevice));
                HIPCK(c, hipMemcpy(S.d_b, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
            }
            continue;
        }
        if (L.type != L_CONV) continue;
        const float *params = p; p += (size_t)L.filters * (L.bn ? 4 : 1);
        const float *w = p; p += (size_t)L.filters * L.cin * L.size * L.size;
        std::vector<float> fcbn;
        if (L.fc && L.bn) {          // a batch-normalised [connected]: biases, weights, scales, rolling mean, rolling variance -> pack_conv's beta gamma mean var | weights
            const size_t F = L.filters, nw = F * L.cin;
            fcbn.assign(params, params + F); fcbn.insert(fcbn.end(), params + F + nw, params + 4 * F + nw); fcbn.insert(fcbn.end(), params + F, params + F + nw);
            params = fcbn.data(); w = fcbn.data() + 4 * F;
        }
        std::vector<float> in_sc;
        if (L.in_dt == DT_FP8) {
            channel_scales(c, L.in[0], in_sc);
            if ((int)in_sc.size() != L.cin) return fail(c, YOLO_ERR_STATE, "internal: scale vector of %zu for %d channels", in_sc.size(), L.cin);
        }
        std::vector<float> wperm;
        const Layer *PL = &L; Layer tmp;
        if (L.fc && L.fc_h * L.fc_w > 1) {
            // darknet / the transposed TF graph flatten the producer CHW (V1/YOLO_V1_Inference.py:196-198); the tensor here is HWC
            const int hw = L.fc_h * L.fc_w, C = L.fc_c;
            wperm.resize((size_t)L.filters * L.cin);
            for (int o = 0; o < L.filters; ++o)
                for (int ch = 0; ch < C; ++ch)
                    for (int q = 0; q < hw; ++q) wperm[(size_t)o * L.cin + (size_t)q * C + ch] = w[(size_t)o * L.cin + (size_t)ch * hw + q];
            w = wperm.data();
        } else if (L.s2d7) {
            // 7x7 / stride 2 / pad 3 over 3 channels == 4x4 / stride 1 / pad 2 over the 2x2 space-to-depth image (32 = 4 positions x 8 padded
            // channels): input row 2*oy + kh - 3 = 2*(oy + a - 2) + dy  <=>  kh = 2a + dy - 1 (taps outside 0..6 get zero weights)
            tmp = L; tmp.size = 4; tmp.cin = 32; PL = &tmp;
            wperm.assign((size_t)L.filters * 32 * 16, 0.f);
            for (int o = 0; o < L.filters; ++o)
                for (int ch = 0; ch < 3; ++ch)
                    for (int a4 = 0; a4 < 4; ++a4) for (int dy = 0; dy < 2; ++dy) { const int kh = 2 * a4 + dy - 1; if (kh < 0 || kh > 6) continue;
                        for (int b4 = 0; b4 < 4; ++b4) for (int dx = 0; dx < 2; ++dx) { const int kw = 2 * b4 + dx - 1; if (kw < 0 || kw > 6) continue;
                            wperm[(((size_t)o * 32 + (dy * 2 + dx) * 8 + ch) * 4 + a4) * 4 + b4] = w[(((size_t)o * 3 + ch) * 7 + kh) * 7 + kw]; } }
            w = wperm.data();
        }
        pack_conv(*PL, params, w, L.in_dt, in_sc.empty() ? nullptr : in_sc.data(), wbuf, bias, osc, c->semantics, !c->pair_of(L.in[0]) ? 0 : L.in[0] < 0 ? 1 : 2);      // (filter rows against a tensor stored as pairs: W_hi | W_hi | W_lo for the image's three blocks, W_hi 32 | W_lo 32 per group for an interleaved layer output)
        HIPCK(c, hipMemcpy(L.d_w, wbuf.data(), wbuf.size(), hipMemcpyHostToDevice));
        HIPCK(c, hipMemcpy(L.d_b, bias.data(), bias.size() * 4, hipMemcpyHostToDevice));
        if (L.d_sc) HIPCK(c, hipMemcpy(L.d_sc, osc.data(), osc.size() * 4, hipMemcpyHostToDevice));
    }
    if (int rc = tail_fragments(c)) return rc;
    if (int rc = filter_fragments(c)) return rc;
    c->weights_loaded = true;
    return YOLO_OK;
}

int yolo_load_darknet_weights(yolo_ctx *c, const char *path, int header_ints)
{
    if (!c) return YOLO_ERR_INVALID;
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) return fail(c, YOLO_ERR_IO, "cannot open weights file '%s'", path ? path : "(null)");
    int32_t ver[3];
    if (fread(ver, 4, 3, f) != 3) { fclose(f); return fail(c, YOLO_ERR_IO, "truncated header in '%s'", path); }
    if (header_ints == 0) header_ints = (ver[0] * 10 + ver[1]) >= 2 ? 5 : 4;      // DN/parser.c:1259-1265
    if (header_ints != 4 && header_ints != 5) { fclose(f); return fail(c, YOLO_ERR_INVALID, "header_ints must be 0, 4 or 5"); }
    fseek(f, 0, SEEK_END); long end = ftell(f); fseek(f, header_ints * 4, SEEK_SET);
    size_t n = (size_t)(end - header_ints * 4) / 4;
    if (n != c->weights_count) { fclose(f); return fail(c, YOLO_ERR_IO, "'%s' holds %zu floats after a %d-int header, topology needs %zu", path, n, header_ints, c->weights_count); }
    std::vector<float> flat(n);
    size_t got = fread(flat.data(), 4, n, f); fclose(f);
    if (got != n) return fail(c, YOLO_ERR_IO, "short read on '%s'", path);
    return yolo_set_weights(c, flat.data(), n);
}

// ---- export artifact: one self-describing file = cfg text + run configuration + the folded, packed,
//      device-ready parameters of every conv (+ fp8 scales, + the tile plan).  Counterpart of the reference's frozen
//      `.pb` (D2T/YOLO_V3_convert_darkenet_to_Tensorflow.py:99-104, D2T/object_detect.py:64-99): `input` in,
//      boxes / scores / classes out, nothing else needed to run. ----
namespace {
struct ArtHeader { char magic[8]; uint32_t version, dtype, semantics, decode, n_layers, num_cfgs, cfg_len, reserved; };
const char kArtMagic[8] = {'Y', 'O', 'L', 'O', 'H', 'I', 'P', '1'};
const uint32_t kArtHasTrees = 1;         // ArtHeader::reserved, bit 0: the softmax trees of the cfg's tree= keys follow the tile plan (0: the layout every artifact had before)
const uint32_t kArtVersion = 3;          // 3: split-fp16 filters packed for the interleaved pair layout (round 6); 2: filters packed chunk-major (conv_kchunk); 1: tap-major
uint64_t fnv1a(uint64_t h, const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } return h; }
struct ArtWriter {
    FILE *f; uint64_t h = 1469598103934665603ull; bool ok = true;
    void put(const void *p, size_t n) { if (ok && n && fwrite(p, 1, n, f) != n) ok = false; h = fnv1a(h, p, n); }
};
struct ArtReader {
    FILE *f; uint64_t h = 1469598103934665603ull; bool ok = true;
    void get(void *p, size_t n) { if (ok && n && fread(p, 1, n, f) != n) ok = false; if (ok) h = fnv1a(h, p, n); }
};
}  // namespace

int yolo_export(yolo_ctx *c, const char *path)
{
    if (!c) return YOLO_ERR_INVALID;
    if (c->vec_n) return fail(c, YOLO_ERR_UNSUPPORTED, "yolo_export: the export artifact of a vector-input network ([net] yolo_input=vector) is not built");
    if (!c->weights_loaded) return fail(c, YOLO_ERR_STATE, "yolo_export before weights were loaded");
    HIPCK(c, hipSetDevice(c->device)); HIPCK(c, hipStreamSynchronize(c->stream));
    FILE *f = path ? fopen(path, "wb") : nullptr;
    if (!f) return fail(c, YOLO_ERR_IO, "cannot create '%s'", path ? path : "(null)");
    ArtWriter w{f};
    const uint32_t NL = (uint32_t)c->layers.size();
    ArtHeader hd; memset(&hd, 0, sizeof hd); memcpy(hd.magic, kArtMagic, 8);
    hd.version = kArtVersion; hd.dtype = c->dtype; hd.semantics = c->semantics; hd.decode = c->decode; hd.n_layers = NL;
    hd.num_cfgs = (uint32_t)conv_num_cfgs(); hd.cfg_len = (uint32_t)c->cfg_text.size();
    hd.reserved = c->trees.empty() ? 0 : kArtHasTrees;
    w.put(&hd, sizeof hd); w.put(c->cfg_text.data(), c->cfg_text.size());
    std::vector<float> sc(c->user_scale); sc.resize(NL, 1.f); w.put(sc.data(), NL * 4);
    std::vector<int32_t> plan(NL); yolo_get_tile_configs(c, plan.data()); w.put(plan.data(), NL * 4);
    // softmax trees (only where the cfg has tree= keys: a network without one writes what it always wrote): path and text of each
    for (auto &t : c->trees) { const uint32_t len[2] = {(uint32_t)t.path.size(), (uint32_t)t.text.size()}; w.put(len, sizeof len); w.put(t.path.data(), t.path.size()); w.put(t.text.data(), t.text.size()); }
    std::vector<uint8_t> buf;
    for (auto &L : c->layers) {
        if (has_state(L)) {          // the parameter blobs of its launches, each behind its byte count (no state: an artifact holds parameters)
            void *ptr[6]; uint64_t bytes[6]; const int nb = state_layer_blobs(c, L, ptr, bytes);
            w.put(bytes, (size_t)nb * 8);
            for (int k = 0; k < nb; ++k) {
                buf.resize(bytes[k]);
                if (hipMemcpy(buf.data(), ptr[k], bytes[k], hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); return fail(c, YOLO_ERR_HIP, "export: device read failed"); }
                w.put(buf.data(), bytes[k]);
            }
            continue;
        }
        if (!has_packed_filters(L)) continue;
        uint64_t sz[3] = {(uint64_t)filter_bytes(L), (uint64_t)L.cout_pad, L.d_sc ? (uint64_t)L.cout_pad : 0};
        if (L.type == L_LOCAL) { sz[0] = (uint64_t)L.H * L.W * L.filters * L.size * L.size * L.cin * dt_size(L.in_dt); sz[1] = (uint64_t)L.H * L.W * L.filters; sz[2] = 0; }
        w.put(sz, sizeof sz);
        const void *src[3] = {L.d_w, L.d_b, L.d_sc}; const size_t bytes[3] = {(size_t)sz[0], (size_t)sz[1] * 4, (size_t)sz[2] * 4};
        for (int k = 0; k < 3; ++k) {
            if (!bytes[k]) continue;
            buf.resize(bytes[k]);
            if (hipMemcpy(buf.data(), src[k], bytes[k], hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); return fail(c, YOLO_ERR_HIP, "export: device read failed"); }
            w.put(buf.data(), bytes[k]);
        }
    }
    const uint64_t sum = w.h;
    if (w.ok && fwrite(&sum, 1, 8, f) != 8) w.ok = false;
    if (fclose(f) != 0) w.ok = false;
    return w.ok ? YOLO_OK : fail(c, YOLO_ERR_IO, "short write on '%s'", path);
}

yolo_ctx *yolo_create_from_file(const char *path, int max_batch, int device, void *stream, int keep_layers, char *err, size_t err_len)
{
    auto bail = [&](yolo_ctx *c, const std::string &m) -> yolo_ctx * { if (err && err_len) snprintf(err, err_len, "%s", m.c_str()); if (c) yolo_destroy(c); return nullptr; };
    FILE *f = path ? fopen(path, "rb") : nullptr;
    if (!f) return bail(nullptr, std::string("cannot open '") + (path ? path : "(null)") + "'");
    ArtReader r{f};
    ArtHeader hd; r.get(&hd, sizeof hd);
    if (!r.ok || memcmp(hd.magic, kArtMagic, 8) != 0 || hd.version != kArtVersion || hd.cfg_len > (1u << 24) || hd.n_layers > 4096) { fclose(f); return bail(nullptr, "not a YOLOHIP1 artifact (or an unsupported version)"); }
    std::string cfg_text(hd.cfg_len, '\0'); r.get(&cfg_text[0], hd.cfg_len);
    std::vector<float> sc(hd.n_layers); r.get(sc.data(), (size_t)hd.n_layers * 4);
    std::vector<int32_t> plan(hd.n_layers); r.get(plan.data(), (size_t)hd.n_layers * 4);
    // the trees the cfg names, in section order: read here, handed to the planner in place of the files (load_tree)
    std::vector<std::pair<std::string, std::string>> trees;
    {
        std::vector<Section> secs; std::string perr;
        if (parse_cfg(cfg_text.c_str(), secs, perr))
            for (size_t i = 1; i < secs.size() && r.ok; ++i) {
                if ((secs[i].type != "region" && secs[i].type != "softmax") || !secs[i].kv.count("tree")) continue;
                // written before trees were served (the [region] head ran as a flat softmax): no tree blobs to read, and not what this cfg means now
                if (!(hd.reserved & kArtHasTrees)) { fclose(f); return bail(nullptr, "the artifact's cfg names a softmax tree but the artifact carries none (exported before trees were served): export it again"); }
                uint32_t len[2] = {0, 0}; r.get(len, sizeof len);
                if (!r.ok || len[0] > (1u << 16) || len[1] > (1u << 26)) { r.ok = false; break; }
                std::string path(len[0], '\0'), text(len[1], '\0'); r.get(&path[0], len[0]); r.get(&text[0], len[1]);
                trees.emplace_back(path, text);
            }
    }
    if (!r.ok) { fclose(f); return bail(nullptr, "truncated artifact"); }
    yolo_config cfg; memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = sizeof cfg; cfg.cfg_text = cfg_text.c_str(); cfg.max_batch = max_batch; cfg.dtype = (int)hd.dtype; cfg.semantics = (int)hd.semantics;
    cfg.decode = (int)hd.decode; cfg.device = device; cfg.keep_layers = keep_layers; cfg.stream = stream;
    g_tree_texts = &trees;
    yolo_ctx *c = yolo_create(&cfg, err, err_len);
    g_tree_texts = nullptr;
    if (!c) { fclose(f); return nullptr; }
    if (c->layers.size() != hd.n_layers) { fclose(f); return bail(c, "artifact layer count does not match its own cfg"); }
    if (c->dtype == YOLO_FP8 && yolo_set_act_scales(c, sc.data(), (int)hd.n_layers) != YOLO_OK) { fclose(f); return bail(c, c->err); }
    std::vector<uint8_t> buf;
    for (auto &L : c->layers) {
        if (has_state(L)) {
            void *ptr[6]; uint64_t bytes[6], got[6]; const int nb = state_layer_blobs(c, L, ptr, bytes);
            r.get(got, (size_t)nb * 8);
            if (!r.ok || memcmp(got, bytes, (size_t)nb * 8) != 0) { fclose(f); return bail(c, "artifact parameters do not fit the topology (truncated file or different packing)"); }
            for (int k = 0; k < nb; ++k) {
                buf.resize(bytes[k]); r.get(buf.data(), bytes[k]);
                if (!r.ok) { fclose(f); return bail(c, "truncated artifact"); }
                if (hipMemcpy(ptr[k], buf.data(), bytes[k], hipMemcpyHostToDevice) != hipSuccess) { fclose(f); return bail(c, "artifact upload failed"); }
            }
            continue;
        }
        if (!has_packed_filters(L)) continue;
        uint64_t sz[3]; r.get(sz, sizeof sz);
        uint64_t want[3] = {(uint64_t)filter_bytes(L), (uint64_t)L.cout_pad, L.d_sc ? (uint64_t)L.cout_pad : 0};
        if (L.type == L_LOCAL) { want[0] = (uint64_t)L.H * L.W * L.filters * L.size * L.size * L.cin * dt_size(L.in_dt); want[1] = (uint64_t)L.H * L.W * L.filters; want[2] = 0; }
        if (!r.ok || sz[0] != want[0] || sz[1] != want[1] || sz[2] != want[2]) { fclose(f); return bail(c, "artifact parameters do not fit the topology (truncated file or different packing)"); }
        void *dst[3] = {L.d_w, L.d_b, L.d_sc}; const size_t bytes[3] = {(size_t)sz[0], (size_t)sz[1] * 4, (size_t)sz[2] * 4};
        for (int k = 0; k < 3; ++k) {
            if (!bytes[k]) continue;
            buf.resize(bytes[k]); r.get(buf.data(), bytes[k]);
            if (!r.ok) { fclose(f); return bail(c, "truncated artifact"); }
            if (hipMemcpy(dst[k], buf.data(), bytes[k], hipMemcpyHostToDevice) != hipSuccess) { fclose(f); return bail(c, "artifact upload failed"); }
        }
    }
    uint64_t sum = 0; const bool got = fread(&sum, 1, 8, f) == 8; fclose(f);
    if (!got || sum != r.h) return bail(c, "artifact checksum mismatch");
    if (tail_fragments(c) != YOLO_OK || filter_fragments(c) != YOLO_OK) return bail(c, c->err);
    c->weights_loaded = true;
    // the tile plan is only meaningful for the tile table it was tuned with and for a plan that fuses nothing it cannot
    if (hd.num_cfgs == (uint32_t)conv_num_cfgs() && !keep_layers) { if (yolo_set_tile_configs(c, plan.data()) != YOLO_OK) { std::vector<int32_t> none(hd.n_layers, -1); yolo_set_tile_configs(c, none.data()); } }
    return c;
}

}  // extern "C"
