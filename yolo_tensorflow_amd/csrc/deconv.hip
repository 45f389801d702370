// Transposed convolution ([deconvolutional], DN/deconvolutional_layer.c) on NHWC tensors as a gather: see DeconvArgs (kernels.h) for the
// phase decomposition and the filter layout.
//
// 16-bit operands (k_deconv16): one wave computes 16 output pixels of one phase x DECONV_CO_TILE channels with
// v_mfma_f32_16x16x32_{bf16,f16}.  The FILTERS are the A operand (rows = output channels) and the gathered input pixels the B operand
// (columns = pixels), so the accumulator has its pixel on the lane (lane & 15) and four consecutive channels in its registers
// ((lane >> 4) * 4 + j): the epilogue stores them as one 8-byte (16-bit) or 16-byte (fp32) piece.  Both fragments are 16 contiguous
// bytes in memory -- 8 channels of one input pixel and tap, 8 K-elements of one filter row -- and are loaded straight from global
// memory: no LDS, no barrier.  A K-step of 32 never straddles a tap inside a lane because Cin_pad is a multiple of 8.
// fp32 operands (k_deconv_f32): plain FMAs, one thread per (output pixel, channel).
#include "kernels.h"
#include "device_common.h"
#include "side_epilogue.h"

namespace {

// the output rows (or columns) of phase p along one axis: o = o0, o0 + s, ... < extent
__device__ __forceinline__ int phase_first(int p, int pad, int s) { return ((p - pad) % s + s) % s; }
__device__ __forceinline__ int phase_count(int o0, int extent, int s) { return o0 < extent ? (extent - o0 + s - 1) / s : 0; }

template <bool H16>
__global__ __launch_bounds__(256) void k_deconv16(const DeconvArgs a)
{
    const int s = a.stride, phase = blockIdx.z, py = phase / s, px = phase - py * s;
    const int oy0 = phase_first(py, a.pad, s), ox0 = phase_first(px, a.pad, s);
    const int ny = phase_count(oy0, a.Ho, s), nx = phase_count(ox0, a.Wo, s);
    const long M = (long)a.N * ny * nx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
    const long m0 = ((long)blockIdx.x * 4 + wave) * 16;
    if (m0 >= M) return;          // (wave-uniform)
    const int ntx = deconv_taps(px, a.size, s), ntap = deconv_taps(py, a.size, s) * ntx;
    // this lane's pixel: column l15 of the B operand and of the accumulator
    const long m = m0 + l15; const bool mv = m < M;
    int n = 0, oy = 0, ox = 0;
    if (mv) { const long t = m / nx; ox = ox0 + (int)(m - t * nx) * s; n = (int)(t / ny); oy = oy0 + (int)(t - (long)n * ny) * s; }
    const int qy = (oy + a.pad) / s, qx = (ox + a.pad) / s;          // input row of tap ty: qy - ty
    const int c0 = blockIdx.y * DECONV_CO_TILE, KP = a.kp[phase];
    const uint16_t *in = (const uint16_t *)a.in, *wt = (const uint16_t *)a.wt + a.woff[phase];
    f32x4 acc[DECONV_CO_TILE / 16];
#pragma unroll
    for (int t = 0; t < DECONV_CO_TILE / 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < KP; k0 += 32) {
        const int k = k0 + lq * 8, tap = k / a.Cin_pad, c = k - tap * a.Cin_pad;
        bf16x8 b = __builtin_bit_cast(bf16x8, u32x4_t{0u, 0u, 0u, 0u});
        if (mv && tap < ntap) {
            const int ty = tap / ntx, iy = qy - ty, ix = qx - (tap - ty * ntx);
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) b = *(const bf16x8 *)(in + (((long)n * a.H + iy) * a.W + ix) * a.in_stride + c);
        }
#pragma unroll
        for (int t = 0; t < DECONV_CO_TILE / 16; ++t) {
            const bf16x8 w = *(const bf16x8 *)(wt + (long)(c0 + t * 16 + l15) * KP + k);
            acc[t] = mma16<H16>(w, b, acc[t]);
        }
    }
    if (!mv) return;
    const float slope = act_slope(a.act);
    const int odt = a.out_dt == DT_F32 ? DT_F32 : H16 ? DT_F16 : DT_BF16;
    const long opix = ((long)n * a.Ho + oy) * a.Wo + ox;
#pragma unroll
    for (int t = 0; t < DECONV_CO_TILE / 16; ++t) {
        const int co = c0 + t * 16 + lq * 4;
        if (co >= a.Cstore) continue;          // (co and Cstore are multiples of 4: the four channels are in or out together)
        const float4 bv = *(const float4 *)(a.bias + co);
        const float v[4] = {acc[t][0] + bv.x, acc[t][1] + bv.y, acc[t][2] + bv.z, acc[t][3] + bv.w};
        side_store4(a.out, opix * a.out_stride + co, odt, slope, v);
    }
}

__global__ __launch_bounds__(256) void k_deconv_f32(const DeconvArgs a)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)a.N * a.Ho * a.Wo * a.Cstore;
    if (idx >= total) return;
    const int co = (int)(idx % a.Cstore); const long opix = idx / a.Cstore;
    const int ox = (int)(opix % a.Wo); const long t = opix / a.Wo; const int oy = (int)(t % a.Ho), n = (int)(t / a.Ho);
    const int s = a.stride, py = (oy + a.pad) % s, px = (ox + a.pad) % s, qy = (oy + a.pad) / s, qx = (ox + a.pad) / s, phase = py * s + px;
    const int nty = deconv_taps(py, a.size, s), ntx = deconv_taps(px, a.size, s);
    const float *in = (const float *)a.in, *w = (const float *)a.wt + a.woff[phase] + (long)co * a.kp[phase];
    float acc = 0.f;
    for (int ty = 0; ty < nty; ++ty) {
        const int iy = qy - ty; if (iy < 0 || iy >= a.H) continue;
        for (int tx = 0; tx < ntx; ++tx) {
            const int ix = qx - tx; if (ix < 0 || ix >= a.W) continue;
            const float *x = in + (((long)n * a.H + iy) * a.W + ix) * a.in_stride, *wk = w + (ty * ntx + tx) * a.Cin_pad;
            for (int c = 0; c < a.Cin_pad; ++c) acc = fmaf(wk[c], x[c], acc);
        }
    }
    float v = acc + a.bias[co];
    v = fmaxf(v, v * act_slope(a.act));
    ((float *)a.out)[opix * a.out_stride + co] = v;
}

}  // namespace

hipError_t launch_deconv(const DeconvArgs &a, hipStream_t s)
{
    if (!side_conv_args_ok(a, a.cout_pad) || !deconv_served(a.size, a.stride, a.pad, a.H, a.W) || a.Cin_pad < 8 || a.Cin_pad % 8 || a.in_stride < a.Cin_pad || a.cout_pad % DECONV_CO_TILE ||
        a.Ho != (a.H - 1) * a.stride + a.size - 2 * a.pad || a.Wo != (a.W - 1) * a.stride + a.size - 2 * a.pad) return hipErrorInvalidValue;
    if (a.in_dt == DT_F32) {
        if (a.out_dt != DT_F32) return hipErrorInvalidValue;
        const long total = (long)a.N * a.Ho * a.Wo * a.Cstore;
        hipLaunchKernelGGL(k_deconv_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if ((a.in_dt != DT_BF16 && a.in_dt != DT_F16) || (a.out_dt != a.in_dt && a.out_dt != DT_F32)) return hipErrorInvalidValue;
    // the largest phase decides the grid: phase p of an axis holds ceil((extent - first) / stride) <= ceil(extent / stride) outputs
    const long mmax = (long)a.N * ((a.Ho + a.stride - 1) / a.stride) * ((a.Wo + a.stride - 1) / a.stride);
    const dim3 grid((unsigned)((mmax + 63) / 64), (unsigned)(a.cout_pad / DECONV_CO_TILE), (unsigned)(a.stride * a.stride));
    if (a.in_dt == DT_F16) hipLaunchKernelGGL(k_deconv16<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_deconv16<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
