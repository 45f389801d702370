// Dense convs of more than 25 taps (6x6 .. 11x11) on 16-bit storage: the tiled implicit-GEMM kernel of conv_igemm.hip with its WIDE switch
// on (conv_igemm_kernel.h) -- tap validity as a row mask and a column mask per output pixel instead of one bit per tap.  Everything else is
// the tiled form as it stands: LDS-DMA gather from NHWC, chunk-outermost K order for whole 128-byte channel chunks, per-lane taps for
// Cin_pad 8 / 16 / 32, the ordinary epilogue (bias, slope activation, folded shortcut, fp32 head store, window of a wider buffer).  A file of
// its own so that these instantiations compile beside, and never with, the ones the headline path runs.
#include "kernels.h"
#include "conv_igemm_kernel.h"

template <int WP, int WC, int TP, int TC, int NS, int BK, int NL, bool UNI, bool H16>
static hipError_t launch_wide_u(const ConvArgs &a, hipStream_t s)
{
    constexpr int BP = WP * TP * 16, BC = WC * TC * 16;
    const long M = (long)a.N * a.Ho * a.Wo;
    const long tiles = ((M + BP - 1) / BP) * ((a.Cout + BC - 1) / BC);
    constexpr size_t lds = conv_lds_bytes<WP, WC, TP, TC, NS, BK, NL>();
    dim3 grid((unsigned)((tiles + 7) / 8 * 8)), block(64 * (WP * WC + NL));   // multiple of 8: see the XCD mapping
    const void *k = (const void *)conv_igemm<WP, WC, TP, TC, NS, BK, UNI, NL, false, 2, false, false, H16, false, HALO_B, HALO_B, false, false, true>;
    if (lds > 65536) {
        hipError_t e = conv_opt_in_lds(k, lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((conv_igemm<WP, WC, TP, TC, NS, BK, UNI, NL, false, 2, false, false, H16, false, HALO_B, HALO_B, false, false, true>), grid, block, lds, s, conv_tile_magic(a, BC, 0));
    return hipGetLastError();
}

template <int ID, bool H16>
static hipError_t launch_wide_id(const ConvArgs &a, hipStream_t s)
{
    constexpr ConvCfg c = kCfgs[ID];
    constexpr int BKE = c.bk;          // K elements per step (2-byte operands)
    return (a.Cin_pad % BKE) == 0 ? launch_wide_u<c.wp, c.wc, c.tp, c.tc, c.ns, c.bk, c.nl, true, H16>(a, s) : launch_wide_u<c.wp, c.wc, c.tp, c.tc, c.ns, c.bk, c.nl, false, H16>(a, s);
}

hipError_t launch_conv_wide(const ConvArgs &a, int cfg, hipStream_t s)
{
    if (!conv_is_wide(a) || a.ksize > CONV_MAX_SIZE || (a.in_dt != DT_BF16 && a.in_dt != DT_F16) || a.split || a.pairk || a.w2) return hipErrorInvalidValue;
    if (a.in_dt == DT_F16 && a.out_dt != DT_F16 && a.out_dt != DT_F32) return hipErrorInvalidValue;
    // 32-bit buffer offsets: the activation window, the `lead` pixels in front of it included, must stay below 2 GiB
    if (((double)a.N * a.H * a.W * a.in_stride + ((a.pad > 1 ? a.pad : 1) + 1.0) * (a.W + 1) * a.in_stride) * 2 >= 2147483648.0) return hipErrorInvalidValue;
    if (a.Kpad % 64) return hipErrorInvalidValue;
    if (a.in_dt == DT_F16) return cfg_dispatch(CfgsWide16{}, cfg, [&](auto id) { return launch_wide_id<decltype(id)::value, true>(a, s); });
    return cfg_dispatch(CfgsWide16{}, cfg, [&](auto id) { return launch_wide_id<decltype(id)::value, false>(a, s); });
}
