// Recurrent layers [rnn] / [gru] / [lstm] (DN/rnn_layer.c, gru_layer.c, lstm_layer.c): the stacked gate GEMM of RecurArgs (kernels.h), one
// time step of every stream per launch.
//
// A workgroup of four waves owns one 16-row tile of the stacked weight matrix and 16 (NT = 1) or 32 (NT = 2) streams.  The weights are the
// A operand of v_mfma_f32_16x16x32_{bf16,f16} (fp32: eight v_mfma_f32_16x16x4_f32 per K step, which is a k-ordered fmaf chain), stored in
// fragment order so that a wave's A load is one contiguous KiB (2 KiB in fp32) read exactly once per launch whatever the stream count; the
// activations [x | h] are the B operand, 16 contiguous bytes (32 in fp32) of one stream per lane, straight from global memory.  The waves
// take the K steps round robin and wave 0 sums the four partial accumulators through LDS -- with M = gates x units rows alone a layer of a
// few hundred units would leave most CUs idle, and atomics would make the sum's order, and so the state, differ from run to run.
// The accumulator then has its stream on the lane (lane & 15) and four consecutive rows in its registers ((lane >> 4) * 4 + j): all gates
// of a unit, so the epilogue is the layer's whole step arithmetic, element by element, with no exchange between lanes.
#include "kernels.h"
#include "device_common.h"
#include "activations.h"

namespace {

// eight consecutive K elements of one weight row or one stream
template <int DT> struct frag_t { bf16x8 v; };
template <> struct frag_t<DT_F32> { float v[8]; };

template <int DT> __device__ __forceinline__ frag_t<DT> frag_zero()
{
    frag_t<DT> f;
    if constexpr (DT == DT_F32) { for (int j = 0; j < 8; ++j) f.v[j] = 0.f; }
    else f.v = __builtin_bit_cast(bf16x8, u32x4_t{0u, 0u, 0u, 0u});
    return f;
}
template <int DT> __device__ __forceinline__ frag_t<DT> frag_load(const void *base, size_t elem)      // at element `elem`, a multiple of 8
{
    frag_t<DT> f;
    if constexpr (DT == DT_F32) {
        const float4 lo = *(const float4 *)((const float *)base + elem), hi = *(const float4 *)((const float *)base + elem + 4);
        f.v[0] = lo.x; f.v[1] = lo.y; f.v[2] = lo.z; f.v[3] = lo.w; f.v[4] = hi.x; f.v[5] = hi.y; f.v[6] = hi.z; f.v[7] = hi.w;
    } else f.v = *(const bf16x8 *)((const uint16_t *)base + elem);
    return f;
}
template <int DT> __device__ __forceinline__ f32x4 frag_mma(const frag_t<DT> &w, const frag_t<DT> &b, f32x4 acc)
{
    if constexpr (DT == DT_F32) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.v[j], b.v[j], acc, 0, 0, 0);
        return acc;
    } else return mma16<DT == DT_F16>(w.v, b.v, acc);
}

// one value of a tensor in the storage type (fp16 saturates, as the other fp16 stores of the library)
template <int DT> __device__ __forceinline__ void store_s(void *p, size_t i, float v)
{
    if constexpr (DT == DT_F32) ((float *)p)[i] = v;
    else if constexpr (DT == DT_F16) ((uint16_t *)p)[i] = __builtin_bit_cast(uint16_t, (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f));
    else ((uint16_t *)p)[i] = (uint16_t)(f32x2_to_bf16x2(v, 0.f) & 0xffffu);
}
template <int DT> __device__ __forceinline__ float load_s(const void *p, size_t i)
{
    if constexpr (DT == DT_F32) return ((const float *)p)[i];
    else if constexpr (DT == DT_F16) return (float)__builtin_bit_cast(_Float16, ((const uint16_t *)p)[i]);
    else return __builtin_bit_cast(float, (uint32_t)((const uint16_t *)p)[i] << 16);
}
template <int DT> __device__ __forceinline__ void store_out(const RecurArgs &a, size_t i, float v)
{
    if (a.out_dt == DT_F32) ((float *)a.out)[i] = v; else store_s<DT>(a.out, i, v);
}

// the gates' own activations (LOGISTIC and TANH of DN/activations.h) in float: 1 - 2 / (e^2x + 1) is the reference's (e^2x - 1) / (e^2x + 1)
// without its inf / inf where e^2x overflows a float
__device__ __forceinline__ float gate_sig(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float gate_tanh(float x) { return 1.f - 2.f / (expf(2.f * x) + 1.f); }

template <int DT, int MODE, int NT>
__global__ __launch_bounds__(256) void k_recur(const RecurArgs a)
{
    __shared__ __attribute__((aligned(16))) float red[3][NT][2][64][4];          // the partial accumulators of waves 1..3
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
    const int mt = blockIdx.x, n0 = blockIdx.y * 16 * NT;
    const int KSx = a.Kx >> 5, KSh = a.Kh >> 5, KS = KSx + KSh;
    const size_t wbase = (size_t)mt * KS * 512 + (size_t)lane * 8;
    f32x4 ax[NT], ah[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) { ax[t] = f32x4{0.f, 0.f, 0.f, 0.f}; ah[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kk = wave; kk < KSx; kk += 4) {
        const frag_t<DT> wf = frag_load<DT>(a.w, wbase + (size_t)kk * 512);
        const int k = kk * 32 + lq * 8;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + l15;
            frag_t<DT> b = frag_zero<DT>();
            if (n < a.n && k < a.x_len) b = frag_load<DT>(a.x, (size_t)n * a.x_stride + k);
            ax[t] = frag_mma<DT>(wf, b, ax[t]);
        }
    }
    for (int kk = wave; kk < KSh; kk += 4) {
        const frag_t<DT> wf = frag_load<DT>(a.w, wbase + (size_t)(KSx + kk) * 512);
        const int k = kk * 32 + lq * 8;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int n = n0 + t * 16 + l15;
            frag_t<DT> b = frag_zero<DT>();
            if (n < a.n && k < a.h_len) b = frag_load<DT>(a.h, (size_t)n * a.h_stride + k);
            ah[t] = frag_mma<DT>(wf, b, ah[t]);
        }
    }
    if (wave) {
#pragma unroll
        for (int t = 0; t < NT; ++t) { *(f32x4 *)red[wave - 1][t][0][lane] = ax[t]; *(f32x4 *)red[wave - 1][t][1][lane] = ah[t]; }
    }
    __syncthreads();
    if (wave) return;
#pragma unroll
    for (int w = 0; w < 3; ++w)
#pragma unroll
        for (int t = 0; t < NT; ++t) { ax[t] += *(const f32x4 *)red[w][t][0][lane]; ah[t] += *(const f32x4 *)red[w][t][1][lane]; }

    const int r0 = mt * 16 + lq * 4;          // this lane's four rows
    const float4 bx = *(const float4 *)(a.bx + r0), bh = *(const float4 *)(a.bh + r0);
    const int ow = min(a.out_stride, (a.units + 7) & ~7);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int n = n0 + t * 16 + l15;
        if (n >= a.n) continue;
        const float px[4] = {ax[t][0] + bx.x, ax[t][1] + bx.y, ax[t][2] + bx.z, ax[t][3] + bx.w};
        const float ph[4] = {ah[t][0] + bh.x, ah[t][1] + bh.y, ah[t][2] + bh.z, ah[t][3] + bh.w};
        const size_t srow = (size_t)n * a.s_stride, orow = (size_t)n * a.out_stride;
        if constexpr (MODE == RK_RNN_STATE) {          // DN/rnn_layer.c:110-118
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = r0 + i;
                if (u >= a.units) continue;
                float v = a.shortcut ? load_s<DT>(a.h, (size_t)n * a.h_stride + u) : 0.f;
                v = (v + act_apply(px[i], a.act)) + act_apply(ph[i], a.act);
                store_s<DT>(a.h_new, srow + u, v);
            }
        } else if constexpr (MODE == RK_DENSE) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = r0 + i;
                if (u < a.units) store_out<DT>(a, orow + u, act_apply(px[i], a.act));
                else if (u < ow) store_out<DT>(a, orow + u, 0.f);
            }
        } else if constexpr (MODE == RK_GRU_GATES) {          // DN/gru_layer.c:164-174
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int u = (r0 >> 1) + j;
                if (u >= a.units) continue;
                const float z = gate_sig(px[2 * j] + ph[2 * j]), r = gate_sig(px[2 * j + 1] + ph[2 * j + 1]);
                a.z[srow + u] = z;
                store_s<DT>(a.rh, srow + u, r * a.h32[srow + u]);
            }
        } else if constexpr (MODE == RK_GRU_BLEND) {          // DN/gru_layer.c:179-190; weighted_sum_cpu: z * state + (1 - z) * candidate
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int u = r0 + i;
                if (u < a.units) {
                    const float s = px[i] + ph[i], cand = a.tanh_ ? gate_tanh(s) : gate_sig(s), z = a.z[srow + u];
                    const float hn = z * a.h32[srow + u] + (1.f - z) * cand;
                    a.h32[srow + u] = hn; store_s<DT>(a.hs, srow + u, hn); store_out<DT>(a, orow + u, hn);
                } else if (u < ow) store_out<DT>(a, orow + u, 0.f);
            }
        } else {          // RK_LSTM, rows i f o g (DN/lstm_layer.c:209-224)
            const int u = r0 >> 2;
            if (u < a.units) {
                const float gi = gate_sig(px[0] + ph[0]), gf = gate_sig(px[1] + ph[1]), go = gate_sig(px[2] + ph[2]), gg = gate_tanh(px[3] + ph[3]);
                const float c = gf * a.c[srow + u] + gi * gg;
                const float hn = go * gate_tanh(c);
                a.c[srow + u] = c; store_s<DT>(a.h_new, srow + u, hn); store_out<DT>(a, orow + u, hn);
            } else if (u < ow) store_out<DT>(a, orow + u, 0.f);
        }
    }
}

template <int DT, int MODE> hipError_t launch_mode(const RecurArgs &a, hipStream_t s)
{
    const unsigned mtiles = (unsigned)(recur_rows(a.mode, a.units) / 16);
    if (a.n <= 16) hipLaunchKernelGGL((k_recur<DT, MODE, 1>), dim3(mtiles, 1), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_recur<DT, MODE, 2>), dim3(mtiles, (unsigned)((a.n + 31) / 32)), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <int DT> hipError_t launch_dt(const RecurArgs &a, hipStream_t s)
{
    switch (a.mode) {
    case RK_RNN_STATE: return launch_mode<DT, RK_RNN_STATE>(a, s);
    case RK_DENSE: return launch_mode<DT, RK_DENSE>(a, s);
    case RK_GRU_GATES: return launch_mode<DT, RK_GRU_GATES>(a, s);
    case RK_GRU_BLEND: return launch_mode<DT, RK_GRU_BLEND>(a, s);
    default: return launch_mode<DT, RK_LSTM>(a, s);
    }
}

bool part_ok(const void *p, int stride, int len, int K) { return len == 0 ? K == 0 : p && !((uintptr_t)p & 15) && stride % 8 == 0 && len % 8 == 0 && len <= stride && K % 32 == 0 && len <= K && K - len < 32; }

}  // namespace

hipError_t launch_recur(const RecurArgs &a, hipStream_t s)
{
    if (a.mode < RK_RNN_STATE || a.mode > RK_LSTM || a.units < 1 || a.n < 1 || !a.w || !a.bx || !a.bh || ((uintptr_t)a.w & 15) || ((uintptr_t)a.bx & 15) || ((uintptr_t)a.bh & 15)) return hipErrorInvalidValue;
    if (!part_ok(a.x, a.x_stride, a.x_len, a.Kx) || !part_ok(a.h, a.h_stride, a.h_len, a.Kh) || a.Kx == 0) return hipErrorInvalidValue;
    if (a.s_stride < a.units || a.s_stride % 8) return hipErrorInvalidValue;
    const bool has_out = a.mode != RK_RNN_STATE && a.mode != RK_GRU_GATES;
    if (has_out && (!a.out || a.out_stride < a.units || (a.out_dt != DT_F32 && a.out_dt != a.dt))) return hipErrorInvalidValue;
    switch (a.mode) {
    case RK_RNN_STATE: if (!a.h_new || !a.h || a.h_stride != a.s_stride) return hipErrorInvalidValue; break;
    case RK_DENSE: if (a.Kh) return hipErrorInvalidValue; break;
    case RK_GRU_GATES: if (!a.z || !a.rh || !a.h32 || !a.h) return hipErrorInvalidValue; break;
    case RK_GRU_BLEND: if (!a.z || !a.h32 || !a.hs || !a.h) return hipErrorInvalidValue; break;
    default: if (!a.c || !a.h_new || !a.h) return hipErrorInvalidValue; break;
    }
    if (a.dt == DT_F32) return launch_dt<DT_F32>(a, s);
    if (a.dt == DT_F16) return launch_dt<DT_F16>(a, s);
    if (a.dt == DT_BF16) return launch_dt<DT_BF16>(a, s);
    return hipErrorInvalidValue;
}
