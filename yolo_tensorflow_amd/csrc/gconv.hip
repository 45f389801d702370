// Grouped convolution ([convolutional] with groups > 1, DN/convolutional_layer.c:458-471) on NHWC tensors: see GConvArgs (kernels.h) for
// the bundle rule and the filter layout.
//
// 16-bit operands (k_gconv16): one wave computes GCONV_PT tiles of 16 output pixels x up to GCONV_CO_TILE output channels of ONE bundle with
// v_mfma_f32_16x16x32_{bf16,f16}.  As in deconv.hip the FILTERS are the A operand (rows = output channels) and the gathered input pixels
// the B operand (columns = pixels): the accumulator has its pixel on the lane (lane & 15) and four consecutive channels in its registers
// ((lane >> 4) * 4 + j), stored as one 8-byte (16-bit) or 16-byte (fp32) piece.  Both fragments are 16 contiguous bytes in memory -- 8
// channels of one input pixel and tap inside the bundle's window, 8 K-elements of one filter row -- and are loaded straight from global
// memory: no LDS, no barrier.  A K-step of 32 never straddles a tap inside a lane because a bundle's kc channels are whole granules.
// The four waves of a workgroup take neighbouring (bundle, piece) units of the SAME pixels, so that the cache lines one wave's gather
// brings in hold the next waves' channels.
//
// Two things follow from the bundles being block-diagonal matrices with stored zeros:
//   * a zero filter entry multiplies a real activation of a neighbouring group, so a non-finite activation in one group reaches the other
//     groups of its bundle as NaN (0 * Inf).  Such a network is lost already; a dense conv spreads it further;
//   * the padding channels of the input window (C .. roundup(C, 8)) must be finite.  They are zeros by the library's store convention.
//
// fp32 operands (k_gconv_f32): plain FMAs, one thread per (output pixel, channel), over the group's own cg channels only.
#include "kernels.h"
#include "device_common.h"
#include "side_epilogue.h"

namespace {

template <bool H16>
__global__ __launch_bounds__(256) void k_gconv16(const GConvArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
    const int pieces = (a.mb + GCONV_CO_TILE - 1) / GCONV_CO_TILE, unit = blockIdx.y * 4 + wave;
    if (unit >= a.nb * pieces) return;          // (wave-uniform)
    const int b = unit / pieces, c0 = (unit - b * pieces) * GCONV_CO_TILE;
    const int nt = min(GCONV_CO_TILE, a.mb - c0) / 16;          // 16-row tiles of this piece: 1 .. GCONV_CO_TILE / 16
    const long M = (long)a.N * a.Ho * a.Wo, m0 = (long)blockIdx.x * (16 * GCONV_PT);
    // this lane's pixels: column l15 of the B operands and of the accumulators
    bool mv[GCONV_PT]; int iy0[GCONV_PT], ix0[GCONV_PT]; long img[GCONV_PT];
#pragma unroll
    for (int p = 0; p < GCONV_PT; ++p) {
        const long m = m0 + p * 16 + l15; mv[p] = m < M; iy0[p] = ix0[p] = 0; img[p] = 0;
        if (mv[p]) { const long r = m / a.Wo; const int n = (int)(r / a.Ho); ix0[p] = (int)(m - r * a.Wo) * a.stride - a.pad; iy0[p] = (int)(r - (long)n * a.Ho) * a.stride - a.pad; img[p] = (long)n * a.H * a.W; }
    }
    const int cb = b * a.kc, Cr = (a.C + 7) & ~7, KP = a.kp;          // the bundle's window begins at channel cb; channels at or past Cr are not read
    const uint16_t *in = (const uint16_t *)a.in + cb, *wt = (const uint16_t *)a.wt + (long)(b * a.mb + c0) * KP;
    f32x4 acc[GCONV_PT][GCONV_CO_TILE / 16];
#pragma unroll
    for (int p = 0; p < GCONV_PT; ++p)
#pragma unroll
        for (int t = 0; t < GCONV_CO_TILE / 16; ++t) acc[p][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // this lane's K position k0 + lq * 8 as (tap row, tap column, channel in the bundle), advanced by 32 per step without a division
    int c = lq * 8, ty = 0, tx = 0;
    while (c >= a.kc) { c -= a.kc; if (++tx == a.size) { tx = 0; ++ty; } }
    for (int k0 = 0; k0 < KP; k0 += 32) {
        bf16x8 bf[GCONV_PT];
#pragma unroll
        for (int p = 0; p < GCONV_PT; ++p) {
            bf[p] = __builtin_bit_cast(bf16x8, u32x4_t{0u, 0u, 0u, 0u});
            const int iy = iy0[p] + ty, ix = ix0[p] + tx;
            if (mv[p] && ty < a.size && cb + c < Cr && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                bf[p] = *(const bf16x8 *)(in + (img[p] + (long)iy * a.W + ix) * a.in_stride + c);
        }
#pragma unroll
        for (int t = 0; t < GCONV_CO_TILE / 16; ++t) {
            if (t >= nt) continue;          // (wave-uniform)
            const bf16x8 w = *(const bf16x8 *)(wt + (long)(t * 16 + l15) * KP + k0 + lq * 8);
#pragma unroll
            for (int p = 0; p < GCONV_PT; ++p) acc[p][t] = mma16<H16>(w, bf[p], acc[p][t]);
        }
        c += 32;
        while (c >= a.kc) { c -= a.kc; if (++tx == a.size) { tx = 0; ++ty; } }
    }
    const float slope = act_slope(a.act);
    const int odt = a.out_dt == DT_F32 ? DT_F32 : H16 ? DT_F16 : DT_BF16;
#pragma unroll
    for (int p = 0; p < GCONV_PT; ++p) {
        if (!mv[p]) continue;
        const long opix = m0 + p * 16 + l15;
#pragma unroll
        for (int t = 0; t < GCONV_CO_TILE / 16; ++t) {
            const int co = b * a.mb + c0 + t * 16 + lq * 4;
            if (t >= nt || co >= a.Cstore) continue;          // (co and Cstore are multiples of 4: the four channels are in or out together)
            const float4 bv = *(const float4 *)(a.bias + co);
            const float v[4] = {acc[p][t][0] + bv.x, acc[p][t][1] + bv.y, acc[p][t][2] + bv.z, acc[p][t][3] + bv.w};
            side_store4(a.out, opix * a.out_stride + co, odt, slope, v);
        }
    }
}

__global__ __launch_bounds__(256) void k_gconv_f32(const GConvArgs a)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)a.N * a.Ho * a.Wo * a.Cstore;
    if (idx >= total) return;
    const int co = (int)(idx % a.Cstore); const long opix = idx / a.Cstore;
    float *o = (float *)a.out + opix * a.out_stride + co;
    if (co >= a.Cout) { *o = 0.f; return; }          // the zeros past the filters, up to the output's granule
    const int ox = (int)(opix % a.Wo); const long r = opix / a.Wo; const int oy = (int)(r % a.Ho), n = (int)(r / a.Ho);
    const int g = co / a.m;          // row co of the filters: its group's own channels, [tap][cg]
    const float *in = (const float *)a.in + g * a.cg, *w = (const float *)a.wt + (long)co * a.kp;
    float acc = 0.f;
    for (int ty = 0; ty < a.size; ++ty) {
        const int iy = oy * a.stride - a.pad + ty; if (iy < 0 || iy >= a.H) continue;
        for (int tx = 0; tx < a.size; ++tx) {
            const int ix = ox * a.stride - a.pad + tx; if (ix < 0 || ix >= a.W) continue;
            const float *x = in + (((long)n * a.H + iy) * a.W + ix) * a.in_stride, *wk = w + (ty * a.size + tx) * a.kc;
            for (int ci = 0; ci < a.cg; ++ci) acc = fmaf(wk[ci], x[ci], acc);
        }
    }
    float v = acc + a.bias[co];
    v = fmaxf(v, v * act_slope(a.act));
    *o = v;
}

}  // namespace

hipError_t launch_gconv(const GConvArgs &a, hipStream_t s)
{
    GConvArgs g = a;
    if (a.groups < 1 || a.C < 1 || a.Cout < 1 || a.C % a.groups || a.Cout % a.groups) return hipErrorInvalidValue;
    gconv_layout(g);
    if (!gconv_served(a.size, a.stride, a.pad, a.H, a.W) || g.t != a.t || g.kp != a.kp || g.nb != a.nb || g.kc != a.kc || g.mb != a.mb || !side_conv_args_ok(a, a.nb * a.mb) || a.in_stride < (a.C + 7) / 8 * 8 ||
        a.Ho != (a.H + 2 * a.pad - a.size) / a.stride + 1 || a.Wo != (a.W + 2 * a.pad - a.size) / a.stride + 1) return hipErrorInvalidValue;
    if (a.in_dt == DT_F32) {
        if (a.out_dt != DT_F32) return hipErrorInvalidValue;
        const long total = (long)a.N * a.Ho * a.Wo * a.Cstore;
        hipLaunchKernelGGL(k_gconv_f32, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a);
        return hipGetLastError();
    }
    if ((a.in_dt != DT_BF16 && a.in_dt != DT_F16) || (a.out_dt != a.in_dt && a.out_dt != DT_F32)) return hipErrorInvalidValue;
    const long M = (long)a.N * a.Ho * a.Wo;
    const int units = a.nb * ((a.mb + GCONV_CO_TILE - 1) / GCONV_CO_TILE);
    if ((units + 3) / 4 > 65535 || (M + 16 * GCONV_PT - 1) / (16 * GCONV_PT) > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((M + 16 * GCONV_PT - 1) / (16 * GCONV_PT)), (unsigned)((units + 3) / 4));
    if (a.in_dt == DT_F16) hipLaunchKernelGGL(k_gconv16<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_gconv16<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
