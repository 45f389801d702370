// Halo-staged instantiations of the implicit-GEMM conv kernel (conv_igemm_kernel.h, HALO = true): 3x3 / stride 1 / pad 1 layers
// whose spatial size is a multiple of 13 -- every residual-block 3x3 conv of a 416x416 darknet-53 (104, 52, 26, 13) --, or (round 5) tiles
// into 10 x 19 blocks / 5 x 19 strips: the 76 / 38 / 19 grids of the 608x608 network.  Which ids are halo forms, and their blocks: conv_cfgs.h.
// Replaces the same reference chain as conv_igemm.hip (DN/convolutional_layer.c:445-485; slim.conv2d V3/yolo_v3.py:47-60).
#include "conv_igemm_kernel.h"

static bool halo_ok(const ConvArgs &a, int bh, int bw);
bool conv_halo13_ok(const ConvArgs &a) { return halo_ok(a, HALO_B, HALO_B); }
bool conv_halo_cfg_ok(const ConvArgs &a, int cfg)
{
    // instantiated for the conv's storage family (the rectangular blocks: bf16 / fp16 storage; pair K loop: the free-running forms writing
    // pairs, 57 / 58 for it alone), and the layer tiles into the configuration's blocks
    return conv_cfg_is_halo(cfg) && conv_cfg_instantiated(a, cfg) && halo_ok(a, kCfgs[cfg].bh, kCfgs[cfg].bw);
}
static bool halo_ok(const ConvArgs &a, int bh, int bw)
{
    const int row = a.in_dt == DT_FP8 ? 128 : 64;                  // channels of one 128-byte chunk
    if (a.in_dt != DT_BF16 && a.in_dt != DT_FP8 && a.in_dt != DT_F16) return false;
    if (a.ksize != 3 || a.stride != 1 || a.pad != 1 || a.Ho != a.H || a.Wo != a.W) return false;
    // whole 13 x 13 blocks (416 x 416 networks), or ragged ones on the bottom / right edge where they waste little (608 x 608: 38 = 3 * 13 - 1,
    // 76 = 6 * 13 - 2, 152 = 12 * 13 - 4: 5 % of the columns; 19 x 19 would compute 26 x 26: refused)
    // (round 5: 10 x 19 and 5 x 19 blocks -- 76 = 8 x 10 - 4 rows, 4 x 19 columns; 38 = 4 x 10 - 2; 19 = 4 x 5 - 1: at most 5 % of the rows)
    const long cover = (long)((a.H + bh - 1) / bh) * ((a.W + bw - 1) / bw) * bh * bw;
    if (cover * 100 > (long)a.H * a.W * 115) return false;
    if (a.Cin_pad % row || a.kchunk != row || a.Kpad != 9 * a.Cin_pad) return false;
    if (a.out_dt == DT_F32) return false;
    // 32-bit buffer offsets below the out-of-range sentinel
    return (double)a.N * a.H * a.W * a.in_stride * dt_size(a.in_dt) < 2147483648.0;
}

template <int WC, int TC, int NL, int EB, bool FREE = false, int NS = 2, bool H16 = false, bool SPLIT = false, int BH = HALO_B, int BW = HALO_B, bool HEADT = false, bool PAIRK = false, bool FRAGW = false>
static hipError_t launch_h(const ConvArgs &a, hipStream_t s)
{
    if (a.tail_f32 && !HEADT) return hipErrorInvalidValue;        // a head as the tail runs on the HEADT instantiations (head_tail in the table)
    constexpr int WP = 1, TP = (BH * BW + 15) / 16, BK = 64, BC = WC * TC * 16;
    const long blocks = (long)a.N * ((a.H + BH - 1) / BH) * ((a.W + BW - 1) / BW);
    const long tiles = blocks * ((a.Cout + BC - 1) / BC);
    constexpr size_t lds = conv_lds_bytes<WP, WC, TP, TC, NS, BK, NL, true, BH, BW, FRAGW>();
    static_assert(lds <= 160 * 1024, "halo form: LDS");
    hipError_t e = conv_opt_in_lds((const void *)conv_igemm<WP, WC, TP, TC, NS, BK, true, NL, false, EB, true, FREE, H16, SPLIT, BH, BW, HEADT, PAIRK, false, FRAGW>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((conv_igemm<WP, WC, TP, TC, NS, BK, true, NL, false, EB, true, FREE, H16, SPLIT, BH, BW, HEADT, PAIRK, false, FRAGW>), dim3((unsigned)((tiles + 7) / 8 * 8)), dim3(64 * (WP * WC + NL)), lds, s, conv_tile_magic(a, BC, BH, BW));
    return hipGetLastError();
}

// stamped diagnostic builds of the free-running 176x256 form (tools only): per-wave cycle sums of the issue / wait / MFMA phases.
// variant 1 (wide): four waves of 176 x 64 (one per SIMD) instead of eight of 176 x 32 -- what a K-step costs a wave that shares its SIMD with
// nobody and reads 40 % fewer LDS bytes per FLOP
template <int WC, int TC>
static hipError_t launch_diag(const ConvArgs &a, hipStream_t s)
{
    constexpr int BC = WC * TC * 16;
    const long tiles = (long)a.N * ((a.H + HALO_B - 1) / HALO_B) * ((a.W + HALO_B - 1) / HALO_B) * ((a.Cout + BC - 1) / BC);
    constexpr size_t lds = conv_lds_bytes<1, WC, 11, TC, 2, 64, 0, true>();
    hipError_t e = conv_opt_in_lds((const void *)conv_igemm<1, WC, 11, TC, 2, 64, true, 0, true, 2, true, true>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((conv_igemm<1, WC, 11, TC, 2, 64, true, 0, true, 2, true, true>), dim3((unsigned)((tiles + 7) / 8 * 8)), dim3(64 * WC), lds, s, conv_tile_magic(a, BC, HALO_B));
    return hipGetLastError();
}
hipError_t launch_conv_halo13_diag(const ConvArgs &a, hipStream_t s, int variant)
{
    if (!conv_halo13_ok(a) || a.in_dt != DT_BF16) return hipErrorInvalidValue;
    return variant == 1 ? launch_diag<4, 4>(a, s) : launch_diag<8, 2>(a, s);
}

// halo configuration ID (conv_cfgs.h): the tile shape comes from the table, operand size / storage form / tail kind / K loop from the conv
template <int ID, int EB, bool H16 = false, bool SPLIT = false, bool HEADT = false, bool PAIRK = false>
static hipError_t launch_hid(const ConvArgs &a, hipStream_t s)
{
    constexpr ConvCfg c = kCfgs[ID];
    static_assert(c.halo && c.wp == 1 && c.bk == 64 && c.tp == (c.bh * c.bw + 15) / 16, "halo form: one wave row over the block's sub-tiles");
    // the free-running 16-bit forms take their filters as fragments from the fragment-order image when the arguments carry one (FRAGW;
    // the planner and the operator leave a.wf null under YOLO_NO_FRAGW=1: the filter stages in LDS, the same id)
    if constexpr (c.free && EB == 2 && !SPLIT && !PAIRK)
        if (a.wf) return launch_h<c.wc, c.tc, c.nl, EB, c.free, c.ns, H16, SPLIT, c.bh, c.bw, HEADT, PAIRK, true>(a, s);
    return launch_h<c.wc, c.tc, c.nl, EB, c.free, c.ns, H16, SPLIT, c.bh, c.bw, HEADT, PAIRK>(a, s);
}
// 16-bit storage: a detection head as the fused tail has its own instantiation where the table says so
template <int ID, bool H16>
static hipError_t launch_hid16(const ConvArgs &a, hipStream_t s)
{
    if constexpr (kCfgs[ID].head_tail) if (a.tail_f32) return launch_hid<ID, 2, H16, false, true>(a, s);
    return launch_hid<ID, 2, H16>(a, s);
}

hipError_t launch_conv_halo13(const ConvArgs &a, int cfg, hipStream_t s)
{
    if (!conv_halo_cfg_ok(a, cfg)) return hipErrorInvalidValue;
    if (a.split) {        // split fp16 storage (YOLO_FP16X2): the free-running forms with the two-pass epilogue
        if (a.in_dt != DT_F16 || a.out_dt != DT_F16 || a.w2) return hipErrorInvalidValue;
        if (a.pairk)          // pairs in, pairs out: the pair K loop (three products per K-step row pair)
            return cfg_dispatch(CfgsHaloPairK{}, cfg, [&](auto id) { return launch_hid<decltype(id)::value, 2, true, true, false, true>(a, s); });
        return cfg_dispatch(CfgsHaloSplit{}, cfg, [&](auto id) { return launch_hid<decltype(id)::value, 2, true, true>(a, s); });          // plain fp16 in, pairs out (mixed plans)
    }
    if (a.in_dt == DT_FP8) return cfg_dispatch(CfgsHaloFp8{}, cfg, [&](auto id) { return launch_hid<decltype(id)::value, 1>(a, s); });
    if (a.in_dt == DT_F16) {
        if (a.out_dt != DT_F16) return hipErrorInvalidValue;
        return cfg_dispatch(CfgsHalo16{}, cfg, [&](auto id) { return launch_hid16<decltype(id)::value, true>(a, s); });
    }
    return cfg_dispatch(CfgsHalo16{}, cfg, [&](auto id) { return launch_hid16<decltype(id)::value, false>(a, s); });
}
