// Fused convolution for gfx950: im2col-free implicit GEMM on bf16 MFMA, NHWC activations.
//
//   out[n,oy,ox,co] = act( sum_{kh,kw,ci} in[n, oy*s+kh-p, ox*s+kw-p, ci] * W[co][kh][kw][ci] + bias[co] ) (+ residual)
//
// Replaces, in one launch, the reference's per-layer chain fill -> im2col -> sgemm -> normalize ->
// scale_bias -> add_bias -> activate (-> shortcut)  (DN/convolutional_layer.c:445-485,
// DN/convolutional_kernels.cu:73-135, DN/blas_kernels.cu:12-75,194-201,711-745) and TF's
// Conv2D + FusedBatchNorm + LeakyRelu (+ Add) behind slim.conv2d (V3/yolo_v3.py:47-60).
//
// GEMM view: D[channel][pixel] = sum_k Wt[channel][k] * X[pixel][k], k = (kh*K+kw)*Cin_pad + ci.
//   * MFMA A operand = filter rows, B operand = activation rows  -> each lane ends up holding 4
//     consecutive output channels of ONE pixel (D row = 4*(lane>>4)+reg, col = lane&15), i.e. an 8-byte
//     (bf16) or 16-byte (fp32) contiguous NHWC store.
//   * K is walked in 64-wide steps; both operand tiles are staged in LDS as [rows][64] bf16 (128-B rows),
//     16-B chunk index XOR-swizzled with (row & 7) so the ds_read_b128 fragment reads are conflict free.
//     LDS-DMA destinations are lane-linear, so the swizzle is applied to the SOURCE offset and to the read.
//   * Activation rows are gathered straight from the NHWC tensor (no im2col buffer) with
//     `buffer_load_dwordx4 ... offen lds`: per lane a CONSTANT 32-bit byte offset (its pixel, its 16-B chunk),
//     per K-step one SCALAR offset (tap and channel base) -- the address arithmetic of a K-step is a handful of
//     SALU instructions, not ~20 VALU per load (which had made the loop VALU-bound).  Padding taps and rows
//     past the last pixel use an out-of-range offset: the buffer range check makes the DMA write zeros
//     (verified on MI355X by tools/probe/lds_dma_oob.hip).
//   * NS-stage LDS ring: the loads of K-step t+NS-1 are issued before the MFMAs of step t; a counted
//     s_waitcnt vmcnt + one raw s_barrier per K-step keep them in flight across the barrier.
#include "kernels.h"
#include <cstdio>
#include <mutex>
#include <set>
#include <utility>

hipError_t conv_opt_in_lds(const void *kernel, size_t lds_bytes)
{
    static std::mutex mu;
    static std::set<std::pair<int, const void *>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev); if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> g(mu);
    if (done.count({dev, kernel})) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e == hipSuccess) done.insert({dev, kernel});
    return e;
}

#include "conv_igemm_kernel.h"


template <int EB>
static hipError_t launch_conv_diag_t(const ConvArgs &a, hipStream_t s)
{
    // diagnostic instantiation of ONE configuration (p176c128_s2, uniform tap)
    constexpr int WP = 1, WC = 4, TP = 11, TC = 2, NS = 2, BK = 64;
    constexpr int BP = WP * TP * 16, BC = WC * TC * 16, NW = WP * WC;
    const long M = (long)a.N * a.Ho * a.Wo;
    const long tiles = ((M + BP - 1) / BP) * ((a.Cout + BC - 1) / BC);
    constexpr size_t lds = conv_lds_bytes<WP, WC, TP, TC, NS, BK>();
    { hipError_t e = conv_opt_in_lds((const void *)conv_igemm<WP, WC, TP, TC, NS, BK, true, 0, true, EB>, lds); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL((conv_igemm<WP, WC, TP, TC, NS, BK, true, 0, true, EB>), dim3((unsigned)((tiles + 7) / 8 * 8)), dim3(64 * NW), lds, s, conv_tile_magic(a, WC * TC * 16, 0));
    return hipGetLastError();
}
hipError_t launch_conv_diag(const ConvArgs &a, hipStream_t s) { return a.in_dt == DT_FP8 ? launch_conv_diag_t<1>(a, s) : launch_conv_diag_t<2>(a, s); }

// ---------------------------------------------------------------------------------------------
// First layer (3x3, stride 1, 3 real input channels padded to 8): HBM-bound (it writes N*H*W*Cout bf16), K is only
// 9 taps x 8 channels = 72 (padded to 96).  No LDS: a lane's MFMA B fragment for K-group (kk, lq) is exactly the
// 16-byte channel vector of ONE input pixel (tap kk*4+lq), so it is a single global_load_dwordx4; the filters
// (Cout x 96 bf16) live in registers for the whole wave.  One wave computes 16 pixels x Cout per step.
template <int TC, bool H16 = false>
__global__ __launch_bounds__(256) void conv_c8_3x3_direct(const ConvArgs a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (H16) fp16_saturating_mode();
    const int lane = threadIdx.x & 63, l15 = lane & 15, lq = lane >> 4;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const long nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    const int M = a.N * a.Ho * a.Wo;
    const int tiles = (M + 15) / 16;
    const bf16_t *__restrict__ in = (const bf16_t *)a.in;
    const bf16_t *__restrict__ wt = (const bf16_t *)a.wt;

    // filters: A fragment (i, kk) = W[channel i*16 + l15][k = (kk*4 + lq)*8 .. +7]; Kpad >= 96 holds zeros past k = 72
    bf16x8 fw[TC][3];
#pragma unroll
    for (int i = 0; i < TC; ++i)
#pragma unroll
        for (int kk = 0; kk < 3; ++kk)
            fw[i][kk] = *(const bf16x8 *)(wt + (size_t)(i * 16 + l15) * a.Kpad + (kk * 4 + lq) * 8);
    float4 bv[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) bv[i] = *(const float4 *)(a.bias + i * 16 + lq * 4);

    const int HoWo = a.Ho * a.Wo;
    constexpr int U = 4;                        // 16-pixel tiles in flight per wave (memory-level parallelism)
    const long groups = (tiles + U - 1) / U;
    for (long g = wave; g < groups; g += nwaves) {
        bf16x8 fx[U][3];
        int mrow[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int m = (int)(g * U + u) * 16 + l15;
            const bool mv = m < M;
            mrow[u] = mv ? m : -1;
            const int mm = mv ? m : M - 1;
            const int n = fast_div(mm, a.howo_mul, a.howo_shift), rem = mm - n * HoWo;
            const int oy = fast_div(rem, a.wo_mul, a.wo_shift), ox = rem - oy * a.Wo;
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                const int tap = kk * 4 + lq;
                const int kh = (tap * 11) >> 5, kw = tap - kh * 3;
                const int iy = oy + kh - 1, ix = ox + kw - 1;
                const bool ok = mv && tap < 9 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
                const bf16_t *p = ok ? in + ((size_t)(n * a.H + iy) * a.W + ix) * a.in_stride : (const bf16_t *)a.zeros;
                fx[u][kk] = *(const bf16x8 *)p;
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            f32x4 acc[TC];
#pragma unroll
            for (int i = 0; i < TC; ++i) {
                acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 3; ++kk) acc[i] = mma16<H16>(fw[i][kk], fx[u][kk], acc[i]);
            }
            if (mrow[u] >= 0) {
#pragma unroll
                for (int i = 0; i < TC; ++i) {
                    float v[4] = {acc[i][0] + bv[i].x, acc[i][1] + bv[i].y, acc[i][2] + bv[i].z, acc[i][3] + bv[i].w};
                    if (a.act != ACT_LINEAR) {
                        const float slope = act_slope(a.act);
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] = fmaxf(v[q], slope * v[q]);     // leaky: == v > 0 ? v : 0.1 v
                    }
                    uint2 pk;
                    pk.x = pack16x2<H16>(v[0], v[1]);
                    pk.y = pack16x2<H16>(v[2], v[3]);
                    if (!H16 && a.out_dt == DT_FP8) {
                        // same value chain as the tiled kernel: bf16 rounding, then e4m3 of value / scale_out
                        const float s8 = a.out_inv_scale;
                        const uint32_t w8 = f32x2_to_fp8<true>(bf16_bits_to_f32(pk.y & 0xffff) * s8, bf16_bits_to_f32(pk.y >> 16) * s8,
                                                               f32x2_to_fp8<false>(bf16_bits_to_f32(pk.x & 0xffff) * s8, bf16_bits_to_f32(pk.x >> 16) * s8, 0));
                        *(uint32_t *)((char *)a.out + (size_t)mrow[u] * a.out_stride + i * 16 + lq * 4) = w8;
                    } else
                        *(uint2 *)((bf16_t *)a.out + (size_t)mrow[u] * a.out_stride + i * 16 + lq * 4) = pk;
                }
            }
        }
    }
#endif
}

bool conv_c8_direct_ok(const ConvArgs &a)
{
    return (a.in_dt == DT_BF16 || (a.in_dt == DT_F16 && a.out_dt == DT_F16)) && a.ksize == 3 && a.stride == 1 && a.pad == 1 && a.Cin_pad == 8 && a.out_dt != DT_F32 && !a.res && a.Kpad >= 96 &&
           (a.Cout == 16 || a.Cout == 32 || a.Cout == 64);
}

hipError_t launch_conv_c8_direct(const ConvArgs &a, hipStream_t s)
{
    const long M = (long)a.N * a.Ho * a.Wo;
    long waves = (M + 63) / 64;
    long blocks = (waves + 3) / 4; if (blocks > 256 * 8) blocks = 256 * 8;
    dim3 grid((unsigned)blocks), block(256);
    if (a.in_dt == DT_F16) {
        if (a.Cout == 16) hipLaunchKernelGGL((conv_c8_3x3_direct<1, true>), grid, block, 0, s, a);
        else if (a.Cout == 32) hipLaunchKernelGGL((conv_c8_3x3_direct<2, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((conv_c8_3x3_direct<4, true>), grid, block, 0, s, a);
    }
    else if (a.Cout == 16) hipLaunchKernelGGL((conv_c8_3x3_direct<1>), grid, block, 0, s, a);
    else if (a.Cout == 32) hipLaunchKernelGGL((conv_c8_3x3_direct<2>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((conv_c8_3x3_direct<4>), grid, block, 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Tile configurations: the table and the families' id lists are conv_cfgs.h
int conv_num_cfgs() { return kNumCfgs; }
bool conv_cfg_is_halo(int cfg) { return cfg >= 0 && cfg < kNumCfgs && kCfgs[cfg].halo; }
bool conv_cfg_tail_ok(int cfg, int cout, bool fp8, bool head)
{
    if (cfg < 0 || cfg >= kNumCfgs) return false;
    const ConvCfg &c = kCfgs[cfg];
    const int bc = c.wc * c.tc * 16;
    if (head) return !fp8 && c.head_tail && cout == 256;      // a head as the tail: the free-running 176 x 256 / 10 x 19 x 256 halo forms have a HEADT instantiation
    return conv_tail_shape(c.wp, c.wc, bc, c.nl, fp8 ? 1 : 2) && bc == cout;
}
const char *conv_cfg_name(int cfg)
{
    struct Names {
        char s[kNumCfgs][32];
        Names()
        {
            for (const ConvCfg &c : kCfgs) {
                const int bp = c.wp * c.tp * 16, bc = c.wc * c.tc * 16;
                if (c.halo && !CfgsHalo16::has(c.id)) snprintf(s[c.id], sizeof s[c.id], "f%dc%d_w%d_pair", bp, bc, c.wp * c.wc);      // the pair K loop's own forms
                else if (c.halo && (c.bh != HALO_B || c.bw != HALO_B)) snprintf(s[c.id], sizeof s[c.id], "f%dx%dc%d_s%d", c.bh, c.bw, bc, c.ns);
                else snprintf(s[c.id], sizeof s[c.id], "%s%dc%d_s%d_k%d%s%d", c.halo ? (c.free ? "f" : "h") : "p", bp, bc, c.ns, c.bk, c.nl ? "_L" : "_w", c.nl ? c.nl : c.wp * c.wc);
            }
        }
    };
    static const Names names;
    if (cfg < 0 || cfg >= kNumCfgs) return cfg == CONV_CFG_DIRECT ? "direct_c8" : "?";
    return names.s[cfg];
}

template <int WP, int WC, int TP, int TC, int NS, int BK, int NL, bool UNI, int EB, bool H16 = false, bool SPLIT = false>
static hipError_t launch_u(const ConvArgs &a, hipStream_t s)
{
    constexpr int BP = WP * TP * 16, BC = WC * TC * 16;
    const long M = (long)a.N * a.Ho * a.Wo;
    const long tiles = ((M + BP - 1) / BP) * ((a.Cout + BC - 1) / BC);
    constexpr size_t lds = conv_lds_bytes<WP, WC, TP, TC, NS, BK, NL>();
    dim3 grid((unsigned)((tiles + 7) / 8 * 8)), block(64 * (WP * WC + NL));   // multiple of 8: see the XCD mapping
    if (lds > 65536) {
        hipError_t e = conv_opt_in_lds((const void *)conv_igemm<WP, WC, TP, TC, NS, BK, UNI, NL, false, EB, false, false, H16, SPLIT>, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((conv_igemm<WP, WC, TP, TC, NS, BK, UNI, NL, false, EB, false, false, H16, SPLIT>), grid, block, lds, s, conv_tile_magic(a, BC, 0));
    return hipGetLastError();
}

template <int WP, int WC, int TP, int TC, int NS, int BK, int NL, int EB, bool H16 = false, bool SPLIT = false>
static hipError_t launch_t(const ConvArgs &a, hipStream_t s)
{
    // 32-bit buffer offsets: the activation window must stay below 2 GiB
    if (((double)a.N * a.H * a.W * a.in_stride + ((a.pad > 1 ? a.pad : 1) + 1.0) * (a.W + 1) * a.in_stride) * EB >= 2147483648.0) return hipErrorInvalidValue;
    constexpr int BKE = BK * 2 / EB;
    if (a.Kpad % BKE) return hipErrorInvalidValue;
    return (a.Cin_pad % BKE) == 0 ? launch_u<WP, WC, TP, TC, NS, BK, NL, true, EB, H16, SPLIT>(a, s) : launch_u<WP, WC, TP, TC, NS, BK, NL, false, EB, H16, SPLIT>(a, s);
}

// tile configuration ID with EB-byte operands
template <int ID, int EB, bool H16 = false, bool SPLIT = false>
static hipError_t launch_id(const ConvArgs &a, hipStream_t s)
{
    constexpr ConvCfg c = kCfgs[ID];
    return launch_t<c.wp, c.wc, c.tp, c.tc, c.ns, c.bk, c.nl, EB, H16, SPLIT>(a, s);
}

hipError_t launch_conv_bf16(const ConvArgs &a, int cfg, hipStream_t s)
{
    // (16-bit storage: bf16, or fp16 -- the same tile table, the same kernels with the other MFMA and conversions)
    if (a.in_dt != DT_BF16 && a.in_dt != DT_F16) return hipErrorInvalidValue;
    if (a.in_dt == DT_F16 && a.out_dt != DT_F16 && a.out_dt != DT_F32) return hipErrorInvalidValue;
    if (conv_is_wide(a)) return launch_conv_wide(a, cfg, s);          // more than 25 taps: the row / column mask instantiations or nothing (conv_wide.hip)
    if (cfg == CONV_CFG_DIRECT && a.split) return launch_conv_c8_direct_pair(a, s);      // the first layer of a split-fp16 network: direct kernel (conv_pair.hip)
    if (a.pairk) return launch_conv_pair(a, cfg, s);          // the input is an interleaved pair tensor: the pair K loop (conv_pair.hip, conv_halo13.hip)
    if (a.split) {
        // split fp16 storage (YOLO_FP16X2), PLAIN input (or the network input's three blocks): fp16 operands, the ordinary K loop, 16-bit
        // outputs written as interleaved pairs (fp32 head outputs as ever); a subset of the tile table is instantiated
        if (a.in_dt != DT_F16 || (a.out_dt != DT_F16 && a.out_dt != DT_F32) || a.w2 || (a.res && a.out_dt == DT_F32)) return hipErrorInvalidValue;
        if (CfgsHaloSplit::has(cfg)) return launch_conv_halo13(a, cfg, s);
        return cfg_dispatch(CfgsSplit{}, cfg, [&](auto id) { return launch_id<decltype(id)::value, 2, true, true>(a, s); });
    }
    if (cfg == CONV_CFG_DIRECT) return conv_c8_direct_ok(a) ? launch_conv_c8_direct(a, s) : hipErrorInvalidValue;
    if (conv_cfg_is_halo(cfg)) return launch_conv_halo13(a, cfg, s);
    if (a.in_dt == DT_F16) return cfg_dispatch(Cfgs16{}, cfg, [&](auto id) { return launch_id<decltype(id)::value, 2, true>(a, s); });
    return cfg_dispatch(Cfgs16{}, cfg, [&](auto id) { return launch_id<decltype(id)::value, 2>(a, s); });
}

// fp8 operands: the same tile ids, the kernel on the e4m3 MFMA
hipError_t launch_conv_fp8(const ConvArgs &a, int cfg, hipStream_t s)
{
    if (a.in_dt != DT_FP8 || conv_is_wide(a)) return hipErrorInvalidValue;
    if (CfgsHaloFp8::has(cfg)) return launch_conv_halo13(a, cfg, s);
    return cfg_dispatch(CfgsFp8{}, cfg, [&](auto id) { return launch_id<decltype(id)::value, 1>(a, s); });
}
