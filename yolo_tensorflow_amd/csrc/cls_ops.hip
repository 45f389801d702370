// Classifier tail for gfx950: global average pool, softmax and top-k (darknet's [avgpool] / [softmax] layers and what classify() does with
// their output: DN/avgpool_layer.c:40-55, DN/blas.c:305-321, D2T/darknet.py:117-123).  Memory- and latency-bound: plain HIP, wave64,
// 16-byte loads, fp32 arithmetic throughout, fixed reduction orders (a launch gives the same bits every time).
#include "kernels.h"
#include "wave_ops.h"
#include <math.h>

namespace {

// tensor forms of the pooled tensor (input and output share one form)
enum { F_BF16 = 0, F_F16 = 1, F_F32 = 2, F_PAIR = 3 };

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void ld8_bf16(const uint16_t *p, float *v)
{
    const uint4 u = *(const uint4 *)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __builtin_bit_cast(float, w[i] << 16); v[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u); }
}
__device__ __forceinline__ void ld8_f16(const uint16_t *p, float *v)
{
    const uint4 u = *(const uint4 *)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { const h2_t h = __builtin_bit_cast(h2_t, w[i]); v[2 * i] = (float)h[0]; v[2 * i + 1] = (float)h[1]; }
}
__device__ __forceinline__ uint16_t f16_bits(float f)      // round to nearest even, saturating at +-65504 (as the conv epilogues do)
{
    f = __builtin_amdgcn_fmed3f(f, -65504.f, 65504.f);
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}
__device__ __forceinline__ float f16_value(uint16_t b) { return (float)__builtin_bit_cast(_Float16, b); }

// eight channels [c0, c0 + 8) of one pixel as fp32; `px` points at the pixel's first element
template <int FORM>
__device__ __forceinline__ void load8(const void *px, int c0, float *v)
{
    if (FORM == F_BF16) ld8_bf16((const uint16_t *)px + c0, v);
    else if (FORM == F_F16) ld8_f16((const uint16_t *)px + c0, v);
    else if (FORM == F_F32) {
        const float4 a = *(const float4 *)((const float *)px + c0), b = *(const float4 *)((const float *)px + c0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {            // interleaved split-fp16 pairs: per 32-channel group 32 hi then 32 lo; the value is hi + lo
        const uint16_t *p = (const uint16_t *)px + (c0 >> 5) * 64 + (c0 & 31);
        float h[8], l[8]; ld8_f16(p, h); ld8_f16(p + 32, l);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = h[i] + l[i];
    }
}
template <int FORM>
__device__ __forceinline__ void store1(void *px, int c, float f)
{
    if (FORM == F_BF16) ((uint16_t *)px)[c] = __builtin_bit_cast(uint16_t, (__bf16)f);
    else if (FORM == F_F16) ((uint16_t *)px)[c] = f16_bits(f);
    else if (FORM == F_F32) ((float *)px)[c] = f;
    else {
        uint16_t *p = (uint16_t *)px + (c >> 5) * 64 + (c & 31);
        const uint16_t hi = f16_bits(f);
        p[0] = hi; p[32] = f16_bits(f - f16_value(hi));
    }
}
template <int FORM> __device__ __forceinline__ size_t elt_bytes() { return FORM == F_F32 ? 4 : 2; }

// ---- [avgpool]: NHWC [n][hw][in_stride] -> [n][out_stride], always global.  One workgroup per (image, slab of 64 channels): lane
//      (pg, v) sums the 8 channels of piece v over the pixels pg, pg + 32, ...; the 32 partial sums of a channel are added in LDS in a
//      fixed order, then divided by h * w as the reference does.  Channels [C, Cstore) of the output are written as zeros. ----
constexpr int AP_NT = 256, AP_SLAB = 64, AP_PG = AP_NT / (AP_SLAB / 8);

template <int FORM>
__global__ __launch_bounds__(AP_NT) void k_avgpool(const void *in, int in_stride, void *out, int out_stride, int hw, int C, int Cstore)
{
    __shared__ float part[AP_PG][AP_SLAB + 1];
    const int t = threadIdx.x, v = t & 7, pg = t >> 3, img = blockIdx.y;
    const int c0 = blockIdx.x * AP_SLAB + v * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c0 < ((C + 7) & ~7)) {
        const char *base = (const char *)in + (size_t)img * hw * in_stride * elt_bytes<FORM>();
        for (int p = pg; p < hw; p += AP_PG) {
            float x[8]; load8<FORM>(base + (size_t)p * in_stride * elt_bytes<FORM>(), c0, x);
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += x[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) part[pg][v * 8 + i] = acc[i];
    __syncthreads();
    if (t < AP_SLAB) {
        const int c = blockIdx.x * AP_SLAB + t;
        if (c < Cstore) {
            float s = 0.f;
            for (int g = 0; g < AP_PG; ++g) s += part[g][t];
            s /= (float)hw;
            store1<FORM>((char *)out + (size_t)img * out_stride * elt_bytes<FORM>(), c, c < C ? s : 0.f);
        }
    }
}

// ---- block-wide collectives (any whole number of waves up to 16; every lane gets the result; fixed order) ----
__device__ __forceinline__ float block_max(float m, float *red)
{
    m = wave_max(m);
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < nw; ++w) r = fmaxf(r, red[w]);
    return r;
}
__device__ __forceinline__ float block_sum(float s, float *red)
{
    s = wave_sum(s);
    const int nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    float r = red[0];
    for (int w = 1; w < nw; ++w) r += red[w];
    return r;
}
// The top_k best of v[0 .. len) (value descending, equal values by ascending index) to cls / tkp; slots past len: index -1, value 0.  Thread t owns the
// entries i = t, t + nt, ... and comes in with the best of them in (bp, bi) (bi < 0: none); a round takes the block's best, and only its owner looks for its
// next one.  v (LDS or global memory) is consumed: a taken entry becomes -inf, which -- like a NaN met in a rescan -- is never selected.  Called by every
// thread of the block; shared by the [softmax] launches and k_view_reduce.
__device__ void block_topk(float *v, int len, float bp, int bi, int top_k, int *cls, float *tkp, float *red_p, int *red_i)
{
    const int t = threadIdx.x, nt = blockDim.x;
    for (int r = 0; r < top_k; ++r) {
        float p = bp; int i = bi;
        block_best(p, i, red_p, red_i);
        if (t == 0) { cls[r] = i; tkp[r] = i >= 0 ? p : 0.f; }
        if (i >= 0 && i % nt == t) {
            v[i] = -INFINITY;                // taken
            bp = 0.f; bi = -1;
            for (int j = t; j < len; j += nt) { const float q = v[j]; if (q > -INFINITY && ranks_before(q, j, bp, bi)) { bp = q; bi = j; } }
        }
    }
    __syncthreads();
}
// softmax of the `len` logits in LDS at v (DN/blas.c:305-321: e = exp(x / temp - max / temp), p = e / sum), probabilities to
// probs[0 .. len) and left in v; then, top_k > 0, the top_k best (probability descending, index ascending) to cls / tkp.
// Called by every thread of the block.
__device__ void block_softmax_topk(float *v, int len, float temp, float *probs, int top_k, int *cls, float *tkp, float *red_p, int *red_i)
{
    const int t = threadIdx.x, nt = blockDim.x;
    float m = -INFINITY;
    for (int i = t; i < len; i += nt) m = fmaxf(m, v[i]);
    const float largest = block_max(m, red_p);
    float s = 0.f;
    for (int i = t; i < len; i += nt) { const float e = expf(v[i] / temp - largest / temp); v[i] = e; s += e; }
    const float sum = block_sum(s, red_p);
    float bp = 0.f; int bi = -1;
    for (int i = t; i < len; i += nt) {
        const float p = v[i] / sum;
        v[i] = p; probs[i] = p;
        if (ranks_before(p, i, bp, bi)) { bp = p; bi = i; }
    }
    block_topk(v, len, bp, bi, top_k, cls, tkp, red_p, red_i);
}

constexpr int SM_NT = 256, SM_MAX = CLS_SOFTMAX_MAX;

// ---- [softmax] (+ top-k): one workgroup per (group, image); x [n][x_stride] fp32, groups * len logits per image ----
__global__ __launch_bounds__(SM_NT) void k_softmax_topk(const float *x, int x_stride, int len, float temp, float *probs, int p_stride,
                                                        int top_k, int *cls, float *tkp)
{
    __shared__ float v[SM_MAX];
    __shared__ float red_p[16];
    __shared__ int red_i[16];
    const int g = blockIdx.x, img = blockIdx.y;
    const float *src = x + (size_t)img * x_stride + (size_t)g * len;
    for (int i = threadIdx.x; i < len; i += SM_NT) v[i] = src[i];
    __syncthreads();
    block_softmax_topk(v, len, temp, probs + (size_t)img * p_stride + (size_t)g * len, top_k, cls + (size_t)img * top_k, tkp + (size_t)img * top_k, red_p, red_i);
}

// ---- [avgpool] + [softmax] in one launch (darknet-19's tail: the fp32 logit map is pooled into LDS, the softmax / top-k runs from
//      there).  One workgroup per image.  x [n][hw][x_stride] fp32 with x_stride a multiple of 4; the pooled vector also goes to
//      pooled [n][pooled_stride] (the [avgpool] layer's own tensor). ----
constexpr int FU_NT = 1024;

__global__ __launch_bounds__(FU_NT) void k_avgpool_softmax(const float *x, int x_stride, int hw, int C, float *pooled, int pooled_stride,
                                                           int groups, float temp, float *probs, int p_stride, int top_k, int *cls, float *tkp)
{
    __shared__ float v[SM_MAX];
    __shared__ float part[4 * FU_NT];
    __shared__ float red_p[16];
    __shared__ int red_i[16];
    const int t = threadIdx.x, img = blockIdx.x;
    const int nvec = (C + 3) >> 2, slots = nvec < FU_NT ? nvec : FU_NT, P = FU_NT / slots;
    const int slot = t % slots, pg = t / slots;
    const float *base = x + (size_t)img * hw * x_stride;
    float *po = pooled + (size_t)img * pooled_stride;
    const float fhw = (float)hw;
    if (pg < P)
        for (int q = slot; q < nvec; q += slots) {        // (P > 1: slots == nvec, one piece per thread)
            float4 a = float4{0.f, 0.f, 0.f, 0.f};
            for (int p = pg; p < hw; p += P) { const float4 b = *(const float4 *)(base + (size_t)p * x_stride + 4 * q); a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }
            const float r[4] = {a.x, a.y, a.z, a.w};
            if (P == 1) {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (4 * q + j < C) { const float m = r[j] / fhw; v[4 * q + j] = m; po[4 * q + j] = m; }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) part[(size_t)pg * 4 * nvec + 4 * q + j] = r[j];
            }
        }
    __syncthreads();
    if (P > 1) {
        for (int c = t; c < C; c += FU_NT) {
            float s = 0.f;
            for (int g = 0; g < P; ++g) s += part[(size_t)g * 4 * nvec + c];
            s /= fhw;
            v[c] = s; po[c] = s;
        }
        __syncthreads();
    }
    const int len = C / groups;
    for (int g = 0; g < groups; ++g)
        block_softmax_topk(v + g * len, len, temp, probs + (size_t)img * p_stride + (size_t)g * len, top_k, cls + (size_t)img * top_k, tkp + (size_t)img * top_k, red_p, red_i);
}

// ---- multi-view classification: the views' rows of every image added in view order, scaled, and the top-k of the result, one workgroup per image.
//      rows [n * views][len]; lane t forms the classes t, t + 256, ...: s = 0; s = s + row_v[c] for v = 0 .. views - 1 (axpy_cpu's order, DN/blas.c), then
//      s * scale.  The selection runs over a scratch copy of the scaled row in global memory (any len; a lane re-reads only what it wrote itself). ----
constexpr int VR_NT = 256;

__global__ __launch_bounds__(VR_NT) void k_view_reduce(const float *rows, int views, int len, float scale, float *sums, float *work, int top_k, int *cls, float *tkp)
{
    __shared__ float red_p[16];
    __shared__ int red_i[16];
    const int img = blockIdx.x, t = threadIdx.x;
    const float *src = rows + (size_t)img * views * len;
    float *dst = sums + (size_t)img * len, *w = top_k > 0 ? work + (size_t)img * len : nullptr;
    float bp = 0.f; int bi = -1;
    for (int i = t; i < len; i += VR_NT) {
        float s = 0.f;
        for (int v = 0; v < views; ++v) s = s + src[(size_t)v * len + i];
        s = s * scale;
        dst[i] = s;
        if (top_k > 0) { w[i] = s; if (s > -INFINITY && ranks_before(s, i, bp, bi)) { bp = s; bi = i; } }
    }
    if (top_k > 0) block_topk(w, len, bp, bi, top_k, cls + (size_t)img * top_k, tkp + (size_t)img * top_k, red_p, red_i);
}

}  // namespace

hipError_t launch_view_reduce(const ViewReduceArgs &a, hipStream_t s)
{
    if (!a.rows || !a.sums || a.n < 1 || a.views < 1 || a.views > VIEWS_MAX || a.len < 1 || a.top_k < 0 || a.top_k > CLS_TOPK_MAX || a.top_k > a.len) return hipErrorInvalidValue;
    if (a.top_k > 0 && (!a.work || !a.cls || !a.topk)) return hipErrorInvalidValue;
    k_view_reduce<<<a.n, VR_NT, 0, s>>>(a.rows, a.views, a.len, a.scale, a.sums, a.work, a.top_k, a.cls, a.topk);
    return hipGetLastError();
}

hipError_t launch_avgpool(const TView &in, bool in_pair, const TView &out, hipStream_t s)
{
    if (in.n < 1 || in.h < 1 || in.w < 1 || in.c < 1 || out.c != in.c || out.dt != in.dt || in.dt == DT_FP8) return hipErrorInvalidValue;
    const int hw = in.h * in.w, C = in.c;
    // what the output may hold beyond its C channels: the padding of its own granule (zeros), never a neighbour's window
    const int Cstore = in_pair ? (C + 31) / 32 * 32 : (C + 7) / 8 * 8 <= out.stride ? (C + 7) / 8 * 8 : C;
    if (in_pair ? (in.stride < 2 * Cstore || out.stride < 2 * Cstore) : (in.stride < C || out.stride < C)) return hipErrorInvalidValue;
    if (in.dt != DT_F32 && in.stride % 8) return hipErrorInvalidValue;          // 16-byte loads
    if (in.dt == DT_F32 && in.stride % 4) return hipErrorInvalidValue;
    const dim3 grid((C + AP_SLAB - 1) / AP_SLAB, in.n);
    if (in_pair) { if (in.dt != DT_F16) return hipErrorInvalidValue; k_avgpool<F_PAIR><<<grid, AP_NT, 0, s>>>(in.ptr, in.stride, out.ptr, out.stride, hw, C, Cstore); }
    else if (in.dt == DT_BF16) k_avgpool<F_BF16><<<grid, AP_NT, 0, s>>>(in.ptr, in.stride, out.ptr, out.stride, hw, C, Cstore);
    else if (in.dt == DT_F16) k_avgpool<F_F16><<<grid, AP_NT, 0, s>>>(in.ptr, in.stride, out.ptr, out.stride, hw, C, Cstore);
    else k_avgpool<F_F32><<<grid, AP_NT, 0, s>>>(in.ptr, in.stride, out.ptr, out.stride, hw, C, Cstore);
    return hipGetLastError();
}

static bool softmax_args_ok(const SoftmaxArgs &a)
{
    if (a.n < 1 || a.groups < 1 || a.len < 1 || a.len > CLS_SOFTMAX_MAX || !(a.temperature > 0.f) || !a.x || !a.probs) return false;
    if (a.x_stride < a.groups * a.len || a.p_stride < a.groups * a.len) return false;
    if (a.top_k < 0 || a.top_k > CLS_TOPK_MAX) return false;
    if (a.top_k > 0 && (a.groups != 1 || !a.cls || !a.topk_probs)) return false;
    return true;
}

hipError_t launch_softmax_topk(const SoftmaxArgs &a, hipStream_t s)
{
    if (!softmax_args_ok(a)) return hipErrorInvalidValue;
    k_softmax_topk<<<dim3(a.groups, a.n), SM_NT, 0, s>>>(a.x, a.x_stride, a.len, a.temperature, a.probs, a.p_stride, a.top_k, a.cls, a.topk_probs);
    return hipGetLastError();
}

bool avgpool_softmax_ok(const TView &in, const SoftmaxArgs &a)
{
    return in.dt == DT_F32 && in.stride % 4 == 0 && in.stride >= in.c && in.c == a.groups * a.len && in.c <= CLS_SOFTMAX_MAX && in.h * in.w >= 1;
}

hipError_t launch_avgpool_softmax(const TView &in, float *pooled, int pooled_stride, const SoftmaxArgs &a, hipStream_t s)
{
    SoftmaxArgs b = a; b.x = (const float *)in.ptr; b.x_stride = a.groups * a.len;
    if (!softmax_args_ok(b) || !avgpool_softmax_ok(in, a) || in.n != a.n || !pooled || pooled_stride < in.c) return hipErrorInvalidValue;
    k_avgpool_softmax<<<a.n, FU_NT, 0, s>>>((const float *)in.ptr, in.stride, in.h * in.w, in.c, pooled, pooled_stride, a.groups, a.temperature,
                                            a.probs, a.p_stride, a.top_k, a.cls, a.topk_probs);
    return hipGetLastError();
}
