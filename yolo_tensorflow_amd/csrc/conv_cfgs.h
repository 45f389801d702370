// The tile table of the implicit-GEMM conv kernels (conv_igemm_kernel.h): ONE row per tile configuration id, and per storage family the
// list of ids it instantiates.  Host-side only (no kernels).  Every launcher dispatches `launch<kCfgs[ID]...>` over its family's list and
// every "may this conv run this id" question is a list or column look-up, so an id names the same tile shape wherever it is accepted.
// The ids are what the tuned plans (yolo_tensorflow_amd/tuned/*.json) and the export artifacts store: a row's id is its index, rows are
// only ever appended.
#pragma once
#include "kernels.h"
#include <type_traits>

struct ConvCfg {
    // waves along pixels, waves along channels, 16-px tiles per wave, 16-ch tiles per wave, LDS stages, K-step, loader waves (0: every
    // wave loads; > 0: role-split, nl loaders beside the wp * wc consumers)
    int id, wp, wc, tp, tc, ns, bk, nl;
    bool halo;          // halo-staged 3x3 / stride 1 form (conv_halo13.hip): one bh x bw pixel block x (wc * tc * 16) channels per workgroup
    bool free;          // ... with free-running waves
    int bh, bw;
    bool head_tail;     // ... that also has the instantiation whose fused 1x1 tail is a detection head (HEADT)
};
#define X(id, wp, wc, tp, tc, ns, bk, nl) {id, wp, wc, tp, tc, ns, bk, nl, false, false, 0, 0, false},
#define HX(id, wp, wc, tp, tc, ns, bk, nl, free, bh, bw, head_tail) {id, wp, wc, tp, tc, ns, bk, nl, true, free, bh, bw, head_tail},
constexpr ConvCfg kCfgs[] = {
    // Pixel-tile heights that are not powers of two exist so the autotuner can make the tile count a near multiple of 256 CUs x resident
    // workgroups (wave quantisation), e.g. 176 px for M = 32 * 26 * 26.
    X(0, 2, 2, 4, 4, 2, 64, 0)  X(1, 2, 2, 4, 4, 3, 64, 0)  X(2, 2, 2, 2, 4, 2, 64, 0)  X(3, 2, 2, 2, 4, 3, 64, 0)
    X(4, 4, 1, 4, 2, 2, 64, 0)  X(5, 4, 1, 4, 2, 3, 64, 0)  X(6, 2, 2, 4, 2, 2, 64, 0)  X(7, 2, 2, 4, 2, 3, 64, 0)
    X(8, 4, 1, 4, 4, 2, 64, 0)  X(9, 4, 1, 4, 4, 3, 64, 0)  X(10, 4, 2, 4, 4, 2, 64, 0) X(11, 4, 2, 4, 4, 3, 64, 0)
    X(12, 2, 4, 4, 4, 2, 64, 0) X(13, 2, 4, 4, 4, 3, 64, 0) X(14, 2, 2, 2, 2, 2, 64, 0) X(15, 2, 2, 2, 2, 4, 64, 0)
    X(16, 1, 4, 11, 2, 2, 64, 0) X(17, 1, 4, 11, 4, 2, 64, 0) X(18, 1, 4, 11, 1, 2, 64, 0) X(19, 1, 4, 10, 2, 2, 64, 0)
    X(20, 1, 4, 12, 2, 2, 64, 0) X(21, 1, 4, 9, 2, 2, 64, 0) X(22, 1, 4, 13, 2, 2, 64, 0) X(23, 1, 4, 6, 2, 2, 64, 0)
    X(24, 1, 4, 7, 2, 2, 64, 0)
    // BK = 32 halves the staging LDS (three or four workgroups per CU) and makes Cin = 32 layers uniform-tap; measured it only pays on
    // the early, short-K layers -- on the deep 3x3 layers the extra barriers cost more than the occupancy buys (0.066 vs 0.053 ms) -- so
    // only a few BK = 32 shapes are kept.
    X(25, 1, 4, 11, 2, 2, 32, 0) X(26, 2, 2, 4, 2, 2, 32, 0)  X(27, 4, 1, 4, 2, 2, 32, 0)  X(28, 4, 1, 4, 4, 2, 32, 0)
    X(29, 2, 2, 2, 2, 2, 32, 0)  X(30, 2, 2, 2, 4, 2, 32, 0)
    X(31, 1, 8, 11, 2, 2, 64, 4) X(32, 1, 8, 11, 2, 2, 64, 0)
    X(33, 1, 4, 11, 2, 3, 64, 0) X(34, 1, 4, 6, 2, 3, 64, 0)
    X(35, 2, 4, 3, 4, 2, 64, 0)
    // halo-staged 3x3 forms on 13 x 13 blocks; 40-: free-running waves
    HX(36, 1, 8, 11, 2, 2, 64, 0, false, 13, 13, false) HX(37, 1, 8, 11, 2, 2, 64, 4, false, 13, 13, false)
    HX(38, 1, 4, 11, 2, 2, 64, 4, false, 13, 13, false) HX(39, 1, 4, 11, 2, 2, 64, 0, false, 13, 13, false)
    HX(40, 1, 8, 11, 2, 2, 64, 0, true, 13, 13, true)   HX(41, 1, 8, 11, 1, 2, 64, 0, true, 13, 13, false)
    HX(42, 1, 4, 11, 2, 2, 64, 0, true, 13, 13, false)  HX(43, 1, 8, 11, 1, 3, 64, 0, true, 13, 13, false)
    // (Tried and dropped, round 4: the free-running halo form with ONE wave per SIMD -- four waves of 176 x 64, 40 % fewer LDS bytes per
    // FLOP than eight of 176 x 32, whose stamped K loop needs 1 708 cycles per K-step against 1 862.  In the network it LOSES: 26x26 layers
    // 0.412 ms against 0.387 for the eleven of them, 52x52 0.495 against 0.460, 13x13 0.307 against 0.289 -- set-up and epilogue are serial
    // in a wave, and with nobody else on the SIMD nothing runs under them.)
    // round 4: whole-Cout tiles for the stand-alone 1x1 layers (every activation row enters ONE CU) and small-batch shapes.  (No tile
    // wider than 256 channels: filters and bias are padded to multiples of 256 rows, cout_pad.)
    X(44, 1, 8, 6, 2, 2, 64, 0) X(45, 1, 8, 6, 2, 3, 64, 0) X(46, 2, 4, 3, 4, 2, 64, 0) X(47, 2, 4, 2, 4, 2, 64, 0)
    X(48, 2, 4, 3, 2, 2, 64, 0) X(49, 2, 4, 4, 2, 3, 64, 0) X(50, 1, 8, 4, 2, 3, 64, 0) X(51, 2, 4, 2, 2, 3, 64, 0)
    X(52, 2, 4, 3, 2, 3, 64, 0) X(53, 2, 4, 3, 2, 4, 64, 0)
    // round 5: free-running halo forms on rectangular blocks: 10 x 19 (12 sub-tiles) x 256 / 128 channels, 5 x 19 (6 sub-tiles) x 128 --
    // the 608 x 608 network's 76 / 38 / 19 grids tile into them exactly, 256 workgroups each at 8 images per GPU
    HX(54, 1, 8, 12, 2, 2, 64, 0, true, 10, 19, true) HX(55, 1, 8, 12, 1, 3, 64, 0, true, 10, 19, false) HX(56, 1, 8, 6, 1, 3, 64, 0, true, 5, 19, false)
    // round 6: free-running 13 x 13-block halo forms with ONE wave per SIMD, for the pair K loop (split fp16 only): four waves of 176 x 64
    // (57) / 176 x 32 (58) read every pixel fragment four times per K-step instead of eight -- 42 % fewer LDS bytes per MFMA in a loop whose
    // LDS reads (1 952 cycles per K-step) sit just under its MFMAs (2 112)
    HX(57, 1, 4, 11, 4, 2, 64, 0, true, 13, 13, false) HX(58, 1, 4, 11, 2, 2, 64, 0, true, 13, 13, false)
};
#undef X
#undef HX
constexpr int kNumCfgs = (int)(sizeof(kCfgs) / sizeof(kCfgs[0]));
constexpr bool conv_cfgs_indexed() { for (int i = 0; i < kNumCfgs; ++i) if (kCfgs[i].id != i) return false; return true; }
static_assert(conv_cfgs_indexed(), "a tile configuration's id is its index in kCfgs");

// ---- what each storage family instantiates: lists of ids, tiled and halo-staged forms apart --------------------------------------------
template <int... I> struct CfgList { static constexpr bool has(int cfg) { return ((cfg == I) || ...); } };
// f(std::integral_constant<int, ID>) for the list's entry ID == cfg; hipErrorInvalidValue if the list does not hold cfg
template <int... I, class F> hipError_t cfg_dispatch(CfgList<I...>, int cfg, F &&f)
{
    hipError_t e = hipErrorInvalidValue;
    (void)((cfg == I && ((e = f(std::integral_constant<int, I>{})), true)) || ...);
    return e;
}
// 16-bit storage (bf16, or fp16: the same kernels with the other MFMA and conversions): every tiled shape; 57 / 58 exist for the pair K loop only
using Cfgs16 = CfgList<0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35,
                       44, 45, 46, 47, 48, 49, 50, 51, 52, 53>;
using CfgsHalo16 = CfgList<36, 37, 38, 39, 40, 41, 42, 43, 54, 55, 56>;
// fp8 operands: the two-stage 128-B-row symmetric shapes that the bf16 tuning kept, and round 4's 8-wave / 3-stage shapes
using CfgsFp8 = CfgList<0, 2, 4, 6, 8, 12, 14, 16, 17, 19, 20, 23, 31, 32, 33, 34, 45, 48, 49, 51>;
using CfgsHaloFp8 = CfgList<36, 37, 38, 39, 40, 41, 42, 43>;
// split fp16 storage (YOLO_FP16X2), plain input: the two-pass epilogue (25..28: 64-byte rows, 3 x 32 = 96 input 'channels' are uniform-tap)
using CfgsSplit = CfgList<0, 2, 3, 4, 6, 7, 8, 14, 15, 16, 23, 25, 26, 27, 28, 33, 34, 45, 49, 52>;
using CfgsHaloSplit = CfgList<40, 41, 43>;
// the pair K loop (the input is an interleaved pair tensor) writing pairs or an fp32 head ...
using CfgsPairK = CfgList<0, 2, 3, 4, 6, 7, 8, 14, 15, 16, 23, 33, 34, 45, 49, 52>;
using CfgsHaloPairK = CfgList<40, 41, 43, 57, 58>;
// ... and writing PLAIN fp16 (the boundaries of a mixed plan); no halo form
using CfgsPairKPlain = CfgList<0, 2, 4, 6, 8, 14, 16, 33>;
// 16-bit storage, convs of more than 25 taps (conv_is_wide): the instantiations with row / column tap masks (WIDE, conv_wide.hip) -- every id
// conv_default_cfg returns, and the 176-pixel shape
using CfgsWide16 = CfgList<0, 2, 4, 6, 8, 14, 16>;

template <int... I> constexpr bool cfgs_are(CfgList<I...>, bool halo) { return ((I >= 0 && I < kNumCfgs && kCfgs[I].halo == halo) && ...); }
static_assert(cfgs_are(Cfgs16{}, false) && cfgs_are(CfgsFp8{}, false) && cfgs_are(CfgsSplit{}, false) && cfgs_are(CfgsPairK{}, false) && cfgs_are(CfgsPairKPlain{}, false) && cfgs_are(CfgsWide16{}, false), "tiled lists hold tiled ids");
static_assert(cfgs_are(CfgsHalo16{}, true) && cfgs_are(CfgsHaloFp8{}, true) && cfgs_are(CfgsHaloSplit{}, true) && cfgs_are(CfgsHaloPairK{}, true), "halo lists hold halo ids");

// is `cfg` instantiated for the storage family of conv `a`
inline bool conv_cfg_instantiated(const ConvArgs &a, int cfg)
{
    // more than 25 taps: only the instantiations with row / column masks read the right taps, and only plain 16-bit storage has them
    if (conv_is_wide(a)) return (a.in_dt == DT_BF16 || a.in_dt == DT_F16) && !a.split && !a.pairk && CfgsWide16::has(cfg);
    if (a.in_dt == DT_FP8) return CfgsFp8::has(cfg) || CfgsHaloFp8::has(cfg);
    if (a.pairk) return a.split ? CfgsPairK::has(cfg) || CfgsHaloPairK::has(cfg) : CfgsPairKPlain::has(cfg);
    if (a.split) return CfgsSplit::has(cfg) || CfgsHaloSplit::has(cfg);
    return Cfgs16::has(cfg) || CfgsHalo16::has(cfg);
}

// Tile shapes whose epilogue can run the fused 1x1 tail (eb: bytes per operand element, 2 or 1 = e4m3): 8-wave shapes only -- in the 4-wave
// 176x128 shapes the extra live registers push the kernel past 256 VGPRs and cost the second resident workgroup per CU, measured slower
// overall even where the pair itself got faster; 16-bit: not in the role-split shapes -- the tail's addresses, hoisted above the K loop,
// push their 168-VGPR budget into spills
constexpr bool conv_tail_shape(int wp, int wc, int bc, int nl, int eb) { return wp == 1 && wc == 8 && (eb == 2 ? nl == 0 && (bc == 256 || bc == 128) : bc == 256); }
