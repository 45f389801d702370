// Internal launcher interface between the host side (planner yolo_plan.cpp, launch sequence yolo_run.cpp, tile selection yolo_tune.cpp, operators
// yolo_ops.cpp) and the gfx950 kernels.
#pragma once
// Cache policy of the conv kernels' OUTPUT stores (aux operand of buffer_store on gfx950: 0 plain write-back, 2 nt, 16 sc1, 17 sc0 sc1).
// Round 5: sc1 -- write-through to memory as the epilogue runs, instead of leaving up to 32 MB of dirty lines for the end-of-kernel L2
// write-back, which is serial with the next launch.  Same-box A/B, YOLOv3-416 batch 32 bf16 (tools/probe/ab/ab_multi.sh, four interleaved
// rounds): conv stack 2.495 -> 2.367 ms per forward, 12.44 -> 13.08 k img/s; sc0 sc1 the same, sc1 nt worse, nt alone no change.  Only for
// COALESCED stores (whole 128-byte lines per lane group): the fp32 head path, 16 bytes per lane into 64 different rows, stays plain.
#ifndef OUT_STORE_AUX
#define OUT_STORE_AUX 16
#endif
// probe knobs (tools/probe/ab), 0 = default policy in the shipped library: cache policy of the halo-staged form's activation tile loads
// (each byte is read once per workgroup) and of the epilogue's shortcut loads (read once)
#ifndef HALO_LOAD_AUX
#define HALO_LOAD_AUX 0
#endif
#ifndef RES_LOAD_AUX
#define RES_LOAD_AUX 0
#endif
#include <hip/hip_runtime.h>
#include <stdint.h>
// the same policy for a 16-byte store of a kernel that holds no descriptor for its output: a buffer store based at the tensor (`base`
// wave-uniform, byte offset below 2 GiB).  (NOT inline asm: a `global_store ... sc1` written as asm is a vector-memory operation the
// compiler's vmcnt bookkeeping does not see -- its counted waits for the loads around it then wait for one operation too few.  Round 5: the
// fp32 head path written that way returned garbage at batch 32 and passed every small test.)
typedef unsigned out_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void out_store16_at(const void *base, unsigned byte_off, unsigned x, unsigned y, unsigned z, unsigned w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, 0x80000000u, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(out_u32x4{x, y, z, w}, r, byte_off, 0, OUT_STORE_AUX);
#endif
}

typedef uint16_t bf16_t;   // raw bfloat16 bits in HBM
struct fp8_t { uint8_t b; };   // raw OCP e4m3 (e4m3fn) bits in HBM
struct f16_t { uint16_t b; };  // raw IEEE binary16 bits in HBM
enum { DT_BF16 = 0, DT_F32 = 1, DT_FP8 = 2, DT_F16 = 3 };
inline size_t dt_size(int dt) { return dt == DT_F32 ? 4 : dt == DT_FP8 ? 1 : 2; }
#define FP8_MAX 448.0f

// A view of an NHWC activation tensor living inside a (possibly wider) buffer: pixel p, channel c is
// at ptr[p * stride + c].  Concats are never materialised: producers write into a channel window of
// the wider buffer (DESIGN.md "route/concat").
struct TView {
    void *ptr = nullptr;
    int n = 0, h = 0, w = 0, c = 0;
    int stride = 0;          // elements per pixel of the underlying buffer
    int dt = DT_BF16;        // element type (DT_*)
};

// Activations: the set DN/activations.c get_activation accepts (the codes are YOLO_ACT_* of include/yolo_hip.h).  The SLOPE FAMILY --
// linear 1, leaky 0.1, relu 0, relie 0.01 -- is max(v, v * act_slope(act)) in every conv epilogue (device_common.h); the others never enter a
// conv kernel: the planner gives such a layer a linear epilogue and a post-activation (Layer::post_act), applied by k_activate (ew_ops.hip)
enum { ACT_LINEAR = 0, ACT_LEAKY = 1, ACT_RELU = 2, ACT_RELIE = 3, ACT_LOGISTIC = 4, ACT_LOGGY = 5, ACT_ELU = 6, ACT_RAMP = 7, ACT_TANH = 8,
       ACT_PLSE = 9, ACT_STAIR = 10, ACT_HARDTAN = 11, ACT_LHTAN = 12, ACT_COUNT = 13 };
inline bool act_is_slope(int act) { return act == ACT_LINEAR || act == ACT_LEAKY || act == ACT_RELU || act == ACT_RELIE; }
int act_from_name(const char *name);          // the code of a darknet activation name, -1 for a name get_activation does not know (yolo_ops.cpp; the planner and yolo_activation_code share it)

struct ConvArgs {
    const void *in; int in_stride;       // elements per input pixel; Cin_pad channels are readable
    const void *wt;                      // packed filters [Cout_pad][Kpad], K index = (kh*k+kw)*Cin_pad + c
    const float *bias;                   // [Cout_pad] fp32 (BN folded)
    void *out; int out_stride; int out_dt;
    const void *res; int res_stride;     // residual (same type as out) or nullptr
    // fp8 (e4m3) operands, DESIGN.md "fp8 scheme": value = code * scale.  in_dt selects the MFMA; `oscale` is the
    // per-output-channel dequantisation factor of the accumulator (filter scale; input scales are folded into the
    // filters), `out_inv_scale` = 1 / scale of the output tensor, `res_scale` = scale of the residual tensor.
    int in_dt;
    int split;                           // 1: split fp16 OUTPUT (YOLO_FP16X2): every 16-bit output value is stored as the pair hi | lo, interleaved per 32-channel group
                                         //    (64 bytes of hi, then 64 bytes of lo); out_stride >= 2 * roundup(Cout, 32) elements; the shortcut source (res) has the same form
    int pairk;                           // 1: the INPUT is such an interleaved pair tensor (Cin_pad = 2 * roundup(Cin, 32) elements per tap) and the filters are packed
                                         //    W_hi 32 | W_lo 32 per group: the conv runs the pair K loop (three MFMA products per K-step row pair, conv_igemm_kernel.h PAIRK)
    const float *oscale;                 // [Cout_pad] or nullptr (== 1)
    float out_inv_scale, res_scale;
    float mid_scale, mid_inv_scale;      // fused shortcut: this conv's own output scale (quantised before the add)
    // fused 1x1 tail (bf16, tile configurations with conv_cfg_tail_ok): out2[pixel][C2] = act2(W2 . out[pixel][:] + b2),
    // computed from the finished output tile while it is still in LDS (the 1x1 conv that follows a 3x3 in every darknet
    // residual block).  w2 == nullptr: none.  C2 = Cout / 2, W2 packed [C2 pad][K2pad], k = channel of `out`.
    const void *w2; const float *b2; void *out2; int out2_stride, K2pad, act2;
    const void *w2f;                     // bf16 tail: W2 in MFMA-fragment order [C2 / 16][K2 / 32][64 lanes][8] (yolo_api.cpp tail_fragments)
    const float *oscale2; float out2_inv_scale;      // fp8 tail: per-channel dequantisation scale of W2, 1 / scale of out2
    const void *wf;                      // 16-bit 3x3 / stride 1 conv: `wt` in MFMA-fragment order [Cout_pad / 16][Kpad / 32][64 lanes][8] (yolo_pack.cpp filter_fragments), or nullptr.
                                         // With it the free-running halo forms read their filters as fragments from global memory (conv_igemm_kernel.h FRAGW), without it through LDS
    int N, H, W, Cin_pad;
    int Ho, Wo, Cout;
    int ksize, stride, pad;
    int Kpad;                            // multiple of 64 (bf16) / 128 (fp8) elements
    int kchunk;                          // channels per K-order chunk: k = (chunk * k*k + tap) * kchunk + c (conv_kchunk())
    int act;
    const void *zeros;                   // >= 64 B of zeros in device memory (padding source)
    // n / d for n < 2^31 as mulhi(n, mul) >> shift (shift == 255: d == 1); filled by conv_finalize()
    uint32_t howo_mul, howo_shift, wo_mul, wo_shift;
    // fp32 head convs feeding a [yolo] layer: objectness logits (channel an * obj_attrs + 4 of every pixel) are ALSO written to
    // obj_out[pixel * obj_na + an]; nullptr: off.  obj_mul / obj_shift: division by obj_attrs (conv_magic)
    float *obj_out; int obj_attrs, obj_na; uint32_t obj_mul, obj_shift;
    unsigned long long *dbg;             // diagnostic builds only: per-wave phase cycle sums
    int dbg_light;                       // diagnostic builds only: 1 = stamp once around the K loop and nothing inside it (the in-kernel clock measurement)
    int C2out;                                // ... its real filter count (255)
    int tail_f32;                             // the fused tail is a detection HEAD: C2 = up to 256 filters, fp32 output [pixel][out2_stride] + bias, linear, objectness plane (obj_*)
    // division constants of the tile decode, filled by the launcher for its tile shape (conv_tile_magic): channel tiles per pixel
    // tile; halo form: 13x13 blocks per image and per block row
    uint32_t tc_mul, tc_shift, bpi_mul, bpi_shift, bpr_mul, bpr_shift;
};
// K-order chunk of a conv whose filters are stored with `wdt` elements: one 128-byte LDS row of channels when the padded
// channel count is a multiple of that, else all channels (i.e. plain tap-major order); fp32 filters keep tap-major order
inline int conv_kchunk(int cin_pad, int wdt) { const int row = wdt == DT_FP8 ? 128 : 64; return (wdt != DT_F32 && cin_pad % row == 0) ? row : cin_pad; }
// host helper: derives the division constants from Ho, Wo (call after filling the geometry)
inline void conv_magic(uint32_t d, uint32_t &mul, uint32_t &shift)
{
    if (d <= 1) { mul = 0; shift = 255; return; }
    uint32_t l = 0; while ((1u << l) < d) ++l;          // ceil(log2 d)
    const unsigned k = 31 + l;
    mul = (uint32_t)(((unsigned long long)1 << k) / d + 1);
    shift = k - 32;
}
inline void conv_finalize(ConvArgs &a)
{
    conv_magic((uint32_t)(a.Ho * a.Wo), a.howo_mul, a.howo_shift);
    conv_magic((uint32_t)a.Wo, a.wo_mul, a.wo_shift);
}
// launcher side of the tile decode: BC = output channels per workgroup, bh x bw = block (rows x columns) of the halo form (0: tiled form)
inline ConvArgs conv_tile_magic(const ConvArgs &a0, int BC, int bh, int bw = 0)
{
    ConvArgs a = a0;
    if (bw == 0) bw = bh;
    conv_magic((uint32_t)((a.Cout + BC - 1) / BC), a.tc_mul, a.tc_shift);
    if (bh > 0) { const int br = (a.H + bh - 1) / bh, bc = (a.W + bw - 1) / bw; conv_magic((uint32_t)(br * bc), a.bpi_mul, a.bpi_shift); conv_magic((uint32_t)bc, a.bpr_mul, a.bpr_shift); }      // (ragged edge blocks included)
    return a;
}

// Dense [convolutional] sizes served (bf16, fp16, fp32).  Up to 25 taps (5x5) the tiled 16-bit kernel carries one validity bit per tap; a
// conv of more taps is WIDE: it runs the instantiations that carry a row mask and a column mask instead (conv_wide.hip)
#define CONV_MAX_SIZE 11
inline bool conv_is_wide(const ConvArgs &a) { return a.ksize * a.ksize > 25; }
inline bool conv_served(int size, int stride, int pad, int h, int w)
{
    return size >= 1 && size <= CONV_MAX_SIZE && stride >= 1 && pad >= 0 && h + 2 * pad >= size && w + 2 * pad >= size;
}
hipError_t launch_conv_wide(const ConvArgs &a, int cfg, hipStream_t s);          // 16-bit storage, conv_is_wide(a), cfg in CfgsWide16
// opt a kernel in to more than 64 KiB of dynamic LDS, once per (device, kernel) -- the attribute is per device
hipError_t conv_opt_in_lds(const void *kernel, size_t lds_bytes);
// bf16 MFMA implicit-GEMM conv.  cfg in [0, conv_num_cfgs()) (the tile table: conv_cfgs.h); returns hipError.
#define CONV_CFG_DIRECT 1000          // first-layer direct kernel (Cin padded 3 -> 8), outside the tile table
bool conv_c8_direct_ok(const ConvArgs &a);
int conv_num_cfgs();
const char *conv_cfg_name(int cfg);
// Tile selection (yolo_tune.cpp), the ONE rule behind the forward, the autotuner, the plan loader and the single-operator entry points:
int conv_default_cfg(const ConvArgs &a);                 // rough preference used when no autotune ran (an id every storage family instantiates, or DIRECT)
bool conv_cfg_runs(const ConvArgs &a, int cfg);          // would the launcher of a's storage family accept (a, cfg)?
int conv_resolve_cfg(const ConvArgs &a, int planned);    // the id a layer planned with `planned` (-1: none) launches
hipError_t launch_conv_bf16(const ConvArgs &a, int cfg, hipStream_t s);
// halo-staged 3x3 / stride 1 form (conv_halo13.hip): bf16 or fp8 operands, spatial size a multiple of 13, whole 128-byte channel chunks
bool conv_halo13_ok(const ConvArgs &a);                  // the 13 x 13-block halo forms
bool conv_halo_cfg_ok(const ConvArgs &a, int cfg);       // halo configuration `cfg`: instantiated for a's storage family, and its block shape fits the layer
bool conv_cfg_is_halo(int cfg);
hipError_t launch_conv_halo13(const ConvArgs &a, int cfg, hipStream_t s);
hipError_t launch_conv_halo13_diag(const ConvArgs &a, hipStream_t s, int variant = 0);   // 0: eight waves of 176 x 32 (the shipped shape), 1: four waves of 176 x 64      // stamped free-running 176x256 build (tools only)
bool conv_cfg_tail_ok(int cfg, int cout, bool fp8, bool head = false);      // can tile configuration `cfg` run the fused 1x1 tail for a conv with `cout` channels
// a conv that READS interleaved pairs (pair K loop), writing pairs / plain fp16 or an fp32 head
hipError_t launch_conv_pair(const ConvArgs &a, int cfg, hipStream_t s);
// first layer of a split-fp16 network (image in three blocks hi | lo | hi -> interleaved pairs): the direct kernel, no LDS (conv_pair.hip)
// fused conv0 + conv1 of a split-fp16 network (conv_stem_pair.hip): image in three blocks -> conv1's interleaved pairs, conv0 never materialised
struct StemPairArgs {
    const void *in;                 // [N, H, W, 24] f16: hi | lo | hi blocks of the 8 padded channels
    const uint8_t *in_u8; float in_scale, in_mul, in_add;      // or (in_u8 != nullptr) the uint8 [N,H,W,3] image itself, converted in the kernel as k_preprocess + k_split_from_f32 would: x * in_scale [* in_mul + in_add], split
    const void *w0; const float *b0; int Kpad0, C0, act0;      // conv0: rows [tap][hi 8 | hi 8 | lo 8] (k = tap * 24 + ...), C0 = 16 or 32 filters
    const void *w1; const float *b1; int Kpad1, act1;          // conv1: rows [tap][W_hi 32 | W_lo 32] (k = tap * 64 + ...), 64 filters
    void *out; int out_stride;      // [N, Ho, Wo, >= 128] f16 interleaved pairs (two 32-channel groups)
    int N, H, W, Ho, Wo;
};
bool conv_stem_pair_ok(const StemPairArgs &a);
hipError_t launch_conv_stem_pair(const StemPairArgs &a, hipStream_t s);
bool conv_c8_direct_pair_ok(const ConvArgs &a);
hipError_t launch_conv_c8_direct_pair(const ConvArgs &a, hipStream_t s);      // the tiled pair-K-loop instantiations (conv_pair.hip); the halo ones: launch_conv_halo13
// fp8 (e4m3 x e4m3 -> fp32, v_mfma_f32_16x16x128_f8f6f4) variant of the same kernel; only the 128-B-row tile configs
hipError_t launch_conv_fp8(const ConvArgs &a, int cfg, hipStream_t s);
hipError_t launch_conv_diag(const ConvArgs &a, hipStream_t s);   // stamped diagnostic build of p176c128_s2 (tools only)
// fused stem: conv 3x3/s1 (3 -> 32) + conv 3x3/s2 (32 -> 64), bf16 (conv_stem.hip)
struct StemArgs {
    const void *in; int in_stride;            // [N,H,W,8] bf16 image (3 real channels)
    const uint8_t *in_u8; float in_scale, in_mul, in_add;      // or (in_u8 != nullptr) the uint8 [N,H,W,3] image itself, converted in the kernel as k_preprocess would: x * in_scale [* in_mul + in_add]
    const void *w0; const float *b0; int Kpad0, C0, act0;    // layer 0: [C0 pad][Kpad0], k = tap*8 + ci
    const void *w1; const float *b1; int Kpad1, C1, act1;    // layer 1: [C1 pad][Kpad1], k = tap*C0 + ci
    void *out; int out_stride;                // [N,Ho,Wo,C1] bf16
    int dt;                                   // DT_BF16 or DT_F16: the 16-bit storage type of every tensor and filter of the launch
    // optional tail: a 1x1/s1 conv C1 -> C2 = 32 on the freshly produced layer-1 tile (darknet-53 layer 2); w2 == nullptr: none
    const void *w2; const float *b2; int Kpad2, C2, act2;    // [C2 pad][Kpad2], k = ci
    void *out2; int out2_stride;              // [N,Ho,Wo,C2] bf16
    int N, H, W, Ho, Wo;
    const void *zeros;
};
bool conv_stem_ok(const StemArgs &a);
hipError_t launch_conv_stem(const StemArgs &a, hipStream_t s);
// halo-staged 3x3/s1 conv, Cin = 32 -> Cout = 64, bf16, optional shortcut (conv_stem.hip)
struct HaloArgs {
    const void *in; int in_stride;            // [N,H,W,>=32] bf16
    const void *w; const float *b; int Kpad, Cin, Cout, act;   // [Cout pad][Kpad], k = tap*32 + ci
    const void *res; int res_stride;          // shortcut source [N,H,W,>=64] bf16 or nullptr
    void *out; int out_stride;
    int N, H, W;
    int dt;                                   // DT_BF16 or DT_F16
};
bool conv_halo_ok(const HaloArgs &a);
hipError_t launch_conv_halo(const HaloArgs &a, hipStream_t s);
// 3x3 / stride 2 / pad 1, 64 -> 128 channels, 16-bit storage, no shortcut (conv_s2.hip): same arguments (H, W: the INPUT size; k = tap*64 + ci)
bool conv_s2_ok(const HaloArgs &a);
hipError_t launch_conv_s2(const HaloArgs &a, hipStream_t s);
// conv 3x3/s1 32 -> 64 + shortcut and the 3x3/s2 64 -> 128 conv that reads it, in one launch (conv_c3s2.hip): the tensor between them is never stored
struct C3S2Args {
    const void *in; int in_stride;            // [N,H,W,>=32]: input of the 3x3/s1 conv
    const void *w3; const float *b3; int Kpad3, act3;         // 3x3/s1: [64 pad][Kpad3], k = tap*32 + ci
    const void *res; int res_stride;          // shortcut source [N,H,W,>=64]
    const void *w5; const float *b5; int Kpad5, act5;         // 3x3/s2: [128 pad][Kpad5], k = tap*64 + ci
    void *out; int out_stride;                // [N,(H-1)/2+1,(W-1)/2+1,>=128]
    int N, H, W;                              // size of the tensor between the two convs
    int dt;                                   // DT_BF16 or DT_F16
};
bool conv_c3s2_ok(const C3S2Args &a);
hipError_t launch_conv_c3s2(const C3S2Args &a, hipStream_t s);
// fused residual block x + act2(conv3x3(act1(conv1x1(x)))), 128 -> 64 -> 128 channels, 16-bit storage (conv_block.hip)
struct BlockArgs {
    const void *x; int x_stride;              // [N,H,W,>=128]: input of the 1x1 and source of the shortcut
    const void *w1; const float *b1; int Kpad1, act1;         // 1x1: [64 pad][Kpad1], k = ci
    const void *w2; const float *b2; int Kpad2, act2;         // 3x3: [128 pad][Kpad2], k = tap*64 + ci
    void *out; int out_stride;                // [N,H,W,>=128]
    int N, H, W, C, Cmid;
    int dt;                                   // DT_BF16 or DT_F16
};
bool conv_resblock_ok(const BlockArgs &a);
hipError_t launch_conv_resblock(const BlockArgs &a, hipStream_t s);
// exact-fp32 MFMA conv (config 2); same argument meaning, in/wt/res are float
hipError_t launch_conv_f32(const ConvArgs &a, hipStream_t s);

// ---- the side convs: [deconvolutional], [convolutional] with groups > 1, [convolutional] with xnor=1 -----------------------------------
// Three conv kinds with a filter layout and a K loop of their own (deconv.hip, gconv.hip, xconv.hip) and everything else in common: these
// fields, the accumulator mapping and the store of their MFMA kernels (side_epilogue.h), the launch sequence's case (yolo_run.cpp), the
// single-operator body (yolo_ops.cpp).  Each kind's struct adds its layout fields and says which channels of `in` it reads.
struct SideConvArgs {
    const void *in; int in_stride;       // elements per input pixel
    const void *wt;                      // the packed filters, in the kind's own layout
    const float *bias;                   // fp32 (BN folded), one entry per filter row of the layout
    void *out; int out_stride; int out_dt, in_dt;      // out_dt: the operand type, or DT_F32 (a "head": logits, a map network's output)
    int N, H, W, Ho, Wo, Cout;
    int Cstore;                          // channels written per pixel: Cout rounded up to the output's granule (zeros past Cout), a multiple of 4
    int size, stride, pad, act;          // act: slope family only
};
// what every launcher asks of those fields; `rows`: the filter rows of the kind's layout (the bias has as many entries).  16-byte fragment loads
// and 8- / 16-byte stores: pixels and channel windows begin on whole granules
inline bool side_conv_args_ok(const SideConvArgs &a, int rows)
{
    if (a.N < 1 || a.in_stride % 8 || a.out_stride % 4 || !act_is_slope(a.act)) return false;
    if (a.Cstore % 4 || a.Cstore < a.Cout || a.Cstore > rows || a.Cstore > a.out_stride) return false;
    return !(((uintptr_t)a.in & 15) || ((uintptr_t)a.wt & 15) || ((uintptr_t)a.bias & 15) || ((uintptr_t)a.out & (a.out_dt == DT_F32 ? 15 : 7)));
}

// ---- transposed convolution (deconv.hip; DN/deconvolutional_layer.c) ------------------------------------------------------------
// out[f, iy * s - p + kh, ix * s - p + kw] += sum_ci w[ci, f, kh, kw] * in[ci, iy, ix], computed as a GATHER: the output splits into s x s
// PHASES ((oy + p) mod s, (ox + p) mod s); phase (py, px) is an implicit GEMM over the taps kh = py + ty * s < size, kw = px + tx * s < size,
// reading iy = (oy + p) / s - ty, ix = (ox + p) / s - tx (rows and columns outside the input contribute nothing).  Per phase the filters
// are packed [cout_pad][kp], k = (ty * taps(px) + tx) * Cin_pad + ci, kp = that K rounded up to 32; a phase without taps (stride > size)
// has kp = 0 and its pixels are act(bias).  No atomics, no col buffer, no zero-fill pass.
#define DECONV_MAX_SIZE 7
#define DECONV_MAX_STRIDE 4
#define DECONV_CO_TILE 32            // output channels per workgroup: cout_pad is a multiple of it
struct DeconvArgs : SideConvArgs {      // in: Cin_pad channels are readable; wt: the phases' filter blocks back to back, in the operand type (in_dt); bias: [cout_pad]
    int Cin_pad, cout_pad;
    int woff[DECONV_MAX_STRIDE * DECONV_MAX_STRIDE], kp[DECONV_MAX_STRIDE * DECONV_MAX_STRIDE];      // per phase py * stride + px: element offset of its block in wt, its padded K
};
__host__ __device__ inline int deconv_taps(int p, int size, int stride) { return p < size ? (size - p + stride - 1) / stride : 0; }
// fills woff / kp for (size, stride, Cin_pad, cout_pad); returns the elements of all blocks together
inline size_t deconv_layout(DeconvArgs &a)
{
    size_t off = 0;
    for (int py = 0; py < a.stride; ++py) for (int px = 0; px < a.stride; ++px) {
        const int k = deconv_taps(py, a.size, a.stride) * deconv_taps(px, a.size, a.stride) * a.Cin_pad;
        a.kp[py * a.stride + px] = (k + 31) / 32 * 32; a.woff[py * a.stride + px] = (int)off;
        off += (size_t)a.cout_pad * a.kp[py * a.stride + px];
    }
    return off;
}
inline bool deconv_served(int size, int stride, int pad, int h, int w)
{
    return size >= 1 && size <= DECONV_MAX_SIZE && stride >= 1 && stride <= DECONV_MAX_STRIDE && pad >= 0 && pad < size &&
           (h - 1) * stride + size - 2 * pad >= 1 && (w - 1) * stride + size - 2 * pad >= 1;
}
// 16-bit operands: v_mfma_f32_16x16x32_{bf16,f16}, fp32 accumulators; fp32 operands: plain FMAs
hipError_t launch_deconv(const DeconvArgs &a, hipStream_t s);

// ---- grouped convolution (gconv.hip; [convolutional] with groups > 1, DN/convolutional_layer.c:458-471) ---------------------------
// Group g reads the input channels g * cg .. (cg = C / groups) and writes the output channels g * m .. (m = Cout / groups); the file
// holds the filters [Cout][cg][size][size].  The packer merges t = max(8 / gcd(cg, 8), 16 / gcd(m, 16)) <= 16 consecutive groups into
// a BUNDLE: its kc = t * cg input channels are whole 8-channel granules, contiguous in NHWC, its mb = t * m output channels whole 16-row
// MFMA tiles.  Per bundle the filters are a block-diagonal matrix [mb][kp], k = tap * kc + (channel in the bundle), tap = ky * size + kx,
// kp = size^2 * kc rounded up to 32; everything off the diagonal, and the rows and columns of the groups a trailing bundle lacks, is zero.
// The bundles lie back to back: nb * mb rows in all (>= Cout; the bias has as many entries).  fp32 operands (in_dt == DT_F32) are not
// bundled: the same nb * mb rows, row o = its group's own filters [tap][cg] (kc = cg, kp = size^2 * cg).
#define GCONV_MAX_SIZE 7
#define GCONV_MAX_STRIDE 4
#define GCONV_CO_TILE 32             // output channels of a bundle per wave: a bundle of more is cut into pieces of this size
#define GCONV_PT 2                   // 16-pixel tiles per wave: one filter fragment feeds this many MFMAs
struct GConvArgs : SideConvArgs {       // in: the channels up to C rounded up to 8 are readable and finite; wt: the bundles' filter blocks back to back, in the operand type (in_dt); bias: [nb * mb]
    int C;
    int groups, cg, m, t, nb, kc, mb, kp;      // the bundle layout (gconv_layout)
};
// fills cg .. kp from (C, Cout, groups, size, in_dt); returns the elements of all blocks together
inline size_t gconv_layout(GConvArgs &a)
{
    a.cg = a.C / a.groups; a.m = a.Cout / a.groups;
    int tc, tm;          // the smallest power of two tc with tc * cg a multiple of 8, tm with tm * m a multiple of 16
    for (tc = 1; (tc * a.cg) % 8; tc *= 2) {}
    for (tm = 1; (tm * a.m) % 16; tm *= 2) {}
    a.t = tc > tm ? tc : tm;
    a.nb = (a.groups + a.t - 1) / a.t; a.kc = a.t * a.cg; a.mb = a.t * a.m;
    a.kp = (a.size * a.size * a.kc + 31) / 32 * 32;
    if (a.in_dt == DT_F32) { a.kc = a.cg; a.kp = a.size * a.size * a.cg; }          // fp32: no bundling, row o holds [tap][cg] of its own group
    return (size_t)a.nb * a.mb * a.kp;
}
inline bool gconv_served(int size, int stride, int pad, int h, int w)
{
    return size >= 1 && size <= GCONV_MAX_SIZE && stride >= 1 && stride <= GCONV_MAX_STRIDE && pad >= 0 && pad < size &&
           h + 2 * pad >= size && w + 2 * pad >= size;
}
// 16-bit operands: v_mfma_f32_16x16x32_{bf16,f16} over the bundles, fp32 accumulators; fp32 operands: plain FMAs over the group's own channels
hipError_t launch_gconv(const GConvArgs &a, hipStream_t s);

// ---- XNOR convolution (xconv.hip; [convolutional] with xnor=1, DN/convolutional_layer.c:28-49, 451-485) ---------------------------
// out = act(scale_f * sum(sign(x) * sign(w_f)) + bias_f): the input becomes +1 where the stored value is > 0 and -1 elsewhere (+0, -0 and NaN give
// -1), a tap outside the image 0; filter f becomes +-1 with alpha_f = mean|w_f| in its scale.  The sum is an integer: v_mfma_i32_16x16x64_i8.
// A workgroup computes a te x te block of output pixels (te = XCONV_TILE, or 4 where the larger block's window does not fit) of one image and
// stages that block's input window into LDS once, as int8.  The window holds the rows and columns the block's taps read: with rs = min(stride,
// size), window row r is input row iy0 + (r / rs) * stride + r % rs (for stride < size every row from the first to the last; for a larger
// stride the rows between two pixels' taps are left out), ww = (te - 1) * rs + size rows and as many columns; tap (ty, tx) of block pixel
// (y, x) is window position (y * rs + ty, x * rs + tx).  The channels are padded to 16 and cut into CHUNKS of cc channels so that a window of
// one chunk fits XCONV_LDS_BYTES (every chunk but the last has cc channels, all are whole 16-channel granules).
// K order: chunk by chunk, inside a chunk k = (tap * granules + granule) * 16 + channel, tap = ky * size + kx, each chunk's K rounded up to
// 64: one lane's 16-byte MFMA fragment is one granule -- 16 consecutive channels of one tap.  The filters are int8 +1 / -1 (0 in every padded
// channel, K position and row) in fragment order, [16-row tile][K step][lane][16]: xconv_pack_index.
#define XCONV_TILE 8                 // edge of the block of output pixels of one workgroup: 64 pixels, four 16-pixel MFMA columns
#define XCONV_CO_TILE 64             // filters of one workgroup pass: the four waves take 32 pixels x 32 filters each
#define XCONV_LDS_BYTES (128 * 1024)
struct XConvArgs : SideConvArgs {       // in: the producer's tensor as stored (in_dt: bf16, fp16 or fp32, whatever out_dt is), the channels up to C rounded up to 8 are readable;
                                        // wt: int8 [cout_pad / 16][kpad / 64][64][16]; bias: [cout_pad], the folded shift, zeros past Cout
    const float *scale;                  // [cout_pad]: alpha_f (* the folded batch-norm scale), zeros past Cout
    int C;
    int te, rs, ww, cc, nchunks, kpad, cout_pad;      // xconv_layout
};
// fills te .. cout_pad from (C, Cout, size, stride); returns the bytes of the filters
inline size_t xconv_layout(XConvArgs &a)
{
    a.rs = a.stride < a.size ? a.stride : a.size;
    a.te = XCONV_TILE; a.ww = (a.te - 1) * a.rs + a.size;
    if ((size_t)a.ww * a.ww * 32 > XCONV_LDS_BYTES) { a.te = 4; a.ww = 3 * a.rs + a.size; }          // (at most 44 x 44 positions: size 11, stride >= 11)
    const int cp = (a.C + 15) / 16 * 16, room = (int)(XCONV_LDS_BYTES / ((size_t)a.ww * a.ww) - 16) / 16 * 16;      // a window position holds cc + 16 bytes (xconv.hip: the pitch)
    a.cc = cp < room ? cp : room;
    a.nchunks = (cp + a.cc - 1) / a.cc;
    const int taps = a.size * a.size, last = cp - (a.nchunks - 1) * a.cc;
    a.kpad = (a.nchunks - 1) * ((taps * a.cc + 63) / 64 * 64) + (taps * last + 63) / 64 * 64;
    a.cout_pad = (a.Cout + XCONV_CO_TILE - 1) / XCONV_CO_TILE * XCONV_CO_TILE;
    return (size_t)a.cout_pad * a.kpad;
}
// where channel ci of tap `tap` lies in a filter row's K (the layout must be filled)
inline int xconv_k(const XConvArgs &a, int tap, int ci)
{
    const int j = ci / a.cc, cp = (a.C + 15) / 16 * 16, ccj = j + 1 < a.nchunks ? a.cc : cp - j * a.cc;
    return j * ((a.size * a.size * a.cc + 63) / 64 * 64) + tap * ccj + (ci - j * a.cc);
}
inline size_t xconv_pack_index(int row, int k, int ksteps) { return ((((size_t)(row >> 4) * ksteps + (k >> 6)) * 64 + (((k >> 4) & 3) << 4 | (row & 15))) << 4) | (size_t)(k & 15); }
inline bool xconv_served(int size, int stride, int pad, int h, int w) { return conv_served(size, stride, pad, h, w); }
hipError_t launch_xconv(const XConvArgs &a, hipStream_t s);

// ---- recurrent layers [rnn] / [gru] / [lstm] (rnn_ops.hip): the stacked gate GEMM with the gate arithmetic in its epilogue ----------
// One launch computes acc[row][stream] = W[row][:] . [x | h][stream][:] for every row of a layer's stacked weight matrix and every stream
// (batch index) of the call, then the step arithmetic of `mode` on the accumulators.  The WEIGHTS are the MFMA A operand, the G gates of
// one unit interleaved along M (row = unit * G + gate), so the four consecutive rows a lane's accumulator holds ((lane >> 4) * 4 + j,
// column lane & 15) are all gates of one unit (G = 4), of two units (G = 2) or four units (G = 1): the epilogue needs no exchange.  The
// activations [x | h] are the B operand, concatenated along K: Kx = roundup(x_len, 32) columns of x, then Kh = roundup(h_len, 32) of h; a
// column at or past x_len / h_len reads as zero.  The products over x and over h are kept in two accumulators (an [rnn] activates each
// before the sum; the gates add them, as the reference adds the two sublayers' outputs); bx / bh [Mp] are their biases (batch norm folded).
// w is stored in fragment order, [M tile][K step][lane][8]: element j of lane l in K step kk of M tile mt is W[mt * 16 + (l & 15)][kk * 32 +
// (l >> 4) * 8 + j] (recur_pack_index) -- a wave's load of one A fragment is one contiguous piece, 16-bit or fp32 alike (the fp32 kernel
// contracts k = (l >> 4) * 8 + j in its j-th v_mfma_f32_16x16x4_f32).  Four waves of a workgroup split the K steps and reduce through LDS.
// Modes (u: unit, n: stream; sig the logistic function; state tensors [max_batch][s_stride], the columns past `units` stay zero):
//   RK_RNN_STATE  G 1  h_new[n][u] = (shortcut ? h[n][u] : 0) + act(x-part + bx) + act(h-part + bh)                 (storage type)
//   RK_DENSE      G 1  out[n][u] = act(x-part + bx): the [rnn]'s output sublayer over h_new; no h part
//   RK_GRU_GATES  G 2  rows z, r: z[n][u] = sig(.) (fp32), rh[n][u] = sig(.) * h32[n][u]                          (storage type)
//   RK_GRU_BLEND  G 1  t = (tanh_ ? tanh : sig)(x-part + rh-part); h' = z * h32 + (1 - z) * t -> h32 (fp32), hs (storage type), out
//   RK_LSTM       G 4  rows i, f, o, g: c = sig(f) * c + sig(i) * tanh(g) in place (fp32); h' = sig(o) * tanh(c) -> h_new (storage type), out
// No launch writes a tensor that another workgroup of the same launch reads as an operand: h_new becomes h by a copy after the layer's
// last launch (yolo_run.cpp); RK_GRU_BLEND reads x and rh only, so it writes hs -- the h operand of RK_GRU_GATES -- itself.
enum { RK_RNN_STATE = 0, RK_DENSE = 1, RK_GRU_GATES = 2, RK_GRU_BLEND = 3, RK_LSTM = 4 };
inline int recur_gates(int mode) { return mode == RK_LSTM ? 4 : mode == RK_GRU_GATES ? 2 : 1; }
inline int recur_rows(int mode, int units) { const int g = recur_gates(mode); return (g * ((units + 7) / 8 * 8) + 15) / 16 * 16; }      // Mp: whole 16-row tiles over whole 8-unit granules of the output
inline size_t recur_pack_index(int row, int k, int ksteps) { return ((((size_t)(row >> 4) * ksteps + (k >> 5)) * 64 + (((k >> 3) & 3) << 4 | (row & 15))) << 3) | (size_t)(k & 7); }
struct RecurArgs {
    int mode, dt;                          // RK_*; operand (storage) type DT_BF16 / DT_F16 / DT_F32: of w, x, h, rh, h_new, hs
    const void *w; const float *bx, *bh;   // [Mp * (Kx + Kh)] in fragment order; [Mp] each
    const void *x; int x_stride, x_len;    // [n][x_stride], x_len <= x_stride valid elements per stream (both multiples of 8)
    const void *h; int h_stride, h_len;    // the same for the second part of K (null / 0: none)
    int Kx, Kh, units, n;
    int act, shortcut, tanh_;
    float *c, *h32, *z;                    // fp32 [max_batch][s_stride]: LSTM cell; GRU state; GRU update gate
    void *rh, *h_new, *hs; int s_stride;
    void *out; int out_stride, out_dt;     // [n][out_stride]; the columns units .. min(out_stride, roundup(units, 8)) are written as zeros
};
hipError_t launch_recur(const RecurArgs &a, hipStream_t s);

// ---- the small layers of a dense-prediction network and the map outputs (map_ops.hip) ----------
// [l2norm] (DN/blas.c:126-144): per pixel, over the channels, x / sqrtf(sum x^2); an all-zero pixel is 0 / 0 = NaN, as in the reference
hipError_t launch_l2norm(const TView &in, const TView &out, hipStream_t s);
// [normalization] / [lrn] (DN/normalization_layer.c:66-95), out of place: out[k] = x[k] * (kappa + alpha * (W(k) - g))^(-beta) over a pixel's channels, W(k) the
// sum of x[j]^2 over k - (size - 1) / 2 <= j <= k + size / 2 inside the tensor, g = x[size / 2]^2 (0 where size / 2 == C): the reference's running sum never
// adds that channel (map_ops.hip derives it).  1 <= size <= LRN_MAX_SIZE (a window reaches one 8-channel granule to either side) and size / 2 <= C
enum { LRN_MAX_SIZE = 17 };
hipError_t launch_lrn(const TView &in, const TView &out, int size, float alpha, float beta, float kappa, hipStream_t s);
// [crop] at inference (DN/crop_layer.c:67-102): the centred out.h x out.w window of `in`, times 2 minus 1 where `adjust`; out.c channels (in.c >= out.c)
hipError_t launch_crop(const TView &in, const TView &out, int adjust, hipStream_t s);
// darknet's [upsample] (DN/blas.c:334-349): nearest, out[y][x] = scale * in[y / stride][x / stride]
hipError_t launch_upsample_nearest(const TView &in, const TView &out, int stride, float scale, hipStream_t s);
hipError_t launch_scale(const TView &x, float scale, hipStream_t s);          // x *= scale in place on the real channels
hipError_t launch_copy_channels(const TView &in, const TView &out, hipStream_t s, int zero_to = 0);      // out = in, element by element: any channel count, any strides, any channel offset; channels in.c .. zero_to of out: zeros
// per map pixel the arg-max over the c <= 255 channels of an fp32 map (the lowest index wins a tie), 255 where the maximum is < thresh
hipError_t launch_label_map(const float *map, int stride, size_t npix, int c, float thresh, uint8_t *labels, hipStream_t s);
// The map pixel a native pixel takes, along one axis: native coordinate x of an image `w` wide, fitted to new_w columns at offset dx of
// a net_w-wide input, with a map_w-wide map: floor(((2x + 1) new_w + 2 w dx) map_w / (2 w net_w)), clamped to map_w - 1 (64-bit integers)
__host__ __device__ inline int map_coord(int x, int w, int new_w, int dx, int net_w, int map_w)
{
    const long long num = ((2LL * x + 1) * new_w + 2LL * w * dx) * map_w, den = 2LL * w * net_w;
    const long long m = num / den;
    return m > map_w - 1 ? map_w - 1 : (int)m;
}
struct ImgDesc;
// labels of a ragged batch at every image's OWN size: image i's h x w labels at labels + label_off[i], each native pixel taking its map
// pixel through the fit (map_coord; FIT_LETTERBOX: darknet's letterbox_image integers, the other fits: the stretch)
hipError_t launch_segment_labels(const float *map, int stride, int map_h, int map_w, int c, float thresh, const ImgDesc *descs, const unsigned long long *label_off,
                                 int n, int fit, int net_h, int net_w, uint8_t *labels, hipStream_t s);
hipError_t launch_nhwc_to_chw(const float *in, float *out, int n, int hw, int c, hipStream_t s);      // dense fp32 [n][hw][c] -> [n][c][hw]

// ---- memory-bound operators (ew_ops.hip) ------------------------------------------------------
// The kernels that write the network input take the image's channel count `nch` ([net] channels; 1..PLANES_MAX with yolo_input=planes): 3 runs the RGB
// form (one lane per pixel, 3 real + 5 zero channels), any other count one lane per pixel x 8-channel granule, the padding of the last granule zero
enum { PLANES_MAX = 1024 };
hipError_t launch_preprocess(const void *img, int fmt /*0 u8 HWC, 1 f32 HWC, 2 f32 planar*/, int n, int hw, float scale,
                             void *out, int out_dt, int out_stride, hipStream_t s, float post_mul = 1.0f, float post_add = 0.0f, int nch = 3);
hipError_t launch_resize_u8(const uint8_t *img, int h, int w, int out_h, int out_w, void *out, int out_dt,
                            int out_stride, int out_c, hipStream_t s, float post_scale = 1.0f, float post_add = 0.0f, int nch = 3);
// cv2.resize (INTER_LINEAR, float32) of a uint8 [h,w,3] image to fp32 [oh,ow,3], optional BGR -> RGB, then / divisor (V2/utils.py:13-27)
hipError_t launch_resize_cv2_u8(const uint8_t *img, int h, int w, int oh, int ow, int swap_rb, float divisor, float *out, hipStream_t s);
// ragged batch of native-size uint8 RGB images (yolo_forward_images_u8): one packed HWC buffer, one descriptor per image (the layout of
// yolo_image_desc, include/yolo_hip.h), all fitted into the network input [n][net_h][net_w][out_stride] in ONE launch.  fit: FIT_* below.
struct ImgDesc { unsigned long long offset; int h, w; };
enum { FIT_STRETCH = 0, FIT_LETTERBOX = 1, FIT_CV2 = 2, FIT_CV2_BGR = 3, FIT_CENTER_CROP = 4 };
// source pixels are read through a buffer descriptor of `bytes` bytes (< 2^32, checked by the caller with every descriptor)
hipError_t launch_fit_images(const uint8_t *pixels, size_t bytes, const ImgDesc *d_descs, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                             int out_stride, float post_mul, float post_add, hipStream_t s, int nch = 3);
// One window of a larger image (yolo_detect_tiled_u8): h x w pixels whose first one lies at byte `offset` of the packed buffer, in an image
// whose rows are `pitch` bytes apart; `image`: the descriptor it was cut from, (x0, y0): its first pixel in that image.  32 bytes.
struct WinDesc { unsigned long long offset; int h, w, pitch, image, x0, y0; };
static_assert(sizeof(WinDesc) == 32, "the window table's row");
// the same launch over n windows: the fit clamps at the window's border and never reads the image around it, so a window is fitted
// bit for bit as its crop would be as an image of its own.  FIT_STRETCH and FIT_LETTERBOX
hipError_t launch_fit_windows(const uint8_t *pixels, size_t bytes, const WinDesc *d_wins, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                              int out_stride, float post_mul, float post_add, hipStream_t s);
// One view of an image (yolo_classify_views_u8): the h x w image at byte `offset` of the packed buffer, shown mirrored when flip != 0.  FIT_TEN_CROP (a fit of
// this launch only, not of the public enum): darknet's ten validation crops -- the image resized to (net_w + shift) x (net_h + shift), the window moved by
// (dx, dy), coordinates clamped (px_ten_crop, ew_ops.hip).  32 bytes.
struct ViewDesc { unsigned long long offset; int h, w, dy, dx, flip, shift; };
static_assert(sizeof(ViewDesc) == 32, "the view table's row");
enum { FIT_TEN_CROP = 5 };
// the same launch over n views, one per batch slot; fit: FIT_STRETCH .. FIT_CENTER_CROP (shift, dy, dx unread) or FIT_TEN_CROP
hipError_t launch_fit_views(const uint8_t *pixels, size_t bytes, const ViewDesc *d_views, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                            int out_stride, float post_mul, float post_add, hipStream_t s, int nch = 3);
// darknet's letterbox_image geometry (DN/image.c:960-966): the aspect-preserving size of a w x h image inside netw x neth
__host__ __device__ inline void letterbox_dims(int netw, int neth, int w, int h, int *new_w, int *new_h)
{
    if (((float)netw / w) < ((float)neth / h)) { *new_w = netw; *new_h = (h * netw) / w; } else { *new_h = neth; *new_w = (w * neth) / h; }
}
// darknet's resize_min geometry (DN/image.c:997-1011): the size of a w x h image whose SHORTER side becomes `min` (integer divisions).  The
// classifier's validation fit (FIT_CENTER_CROP, DN/examples/classifier.c:635-636) crops netw x neth from the centre of that.  The caller refuses
// an image whose longer side times `min` does not fit an int (resize_min_ok): the reference's own product overflows there
__host__ __device__ inline void resize_min_dims(int min, int w, int h, int *new_w, int *new_h)
{
    if (w < h) { *new_h = (h * min) / w; *new_w = min; } else { *new_w = (w * min) / h; *new_h = min; }
}
inline bool resize_min_ok(int min, int w, int h) { return min >= 1 && w >= 1 && h >= 1 && (long long)(w > h ? w : h) * min <= 0x7fffffffLL; }
// the value one source byte contributes before any interpolation: STRETCH value / 255.0f (TF's convert_image_dtype), LETTERBOX and CENTER_CROP
// darknet's loader `(float)data / 255.` -- a DOUBLE division rounded to float (DN/image.c load_image_stb) --, CV2 the byte itself (/ 225 comes last)
__host__ __device__ inline float fit_unit_value(int fit, unsigned v)
{
    if (fit == FIT_STRETCH) return (float)v / 255.0f;
    if (fit == FIT_LETTERBOX || fit == FIT_CENTER_CROP) return (float)((double)v / 255.);
    return (float)v;
}
// ---- decoded video frames (yolo_*_frames_*): a frame is h x w pixels stored as NV12, I420 or pitched RGB / BGR rows, every plane at its own
// byte offset of the packed buffer and its own row pitch (the layout of yolo_frame_desc, include/yolo_hip.h; offsets and pitches < 2^32, checked by the
// caller).  The fits read a frame as the h x w x 3 byte image the colour rule below yields; no such image is stored.  64 bytes.
struct FrameDesc { unsigned long long offset[3], pitch[3]; int h, w, format, matrix; };
static_assert(sizeof(FrameDesc) == 64, "the frame table's row: a power of two");
enum { PIX_NV12 = 0, PIX_I420 = 1, PIX_RGB24 = 2, PIX_BGR24 = 3, PIX_COUNT = 4 };
enum { MATRIX_BT601 = 0, MATRIX_BT709 = 1, MATRIX_BT601_FULL = 2, MATRIX_COUNT = 3 };
// The colour rule, in int32 (every intermediate lies in -282 943 616 .. +573 487 137): the integers are round(k * 2^20) of the classic decimal constants
//   BT.601 limited 1.164, 1.596, 0.391, 0.813, 2.018;  BT.709 limited 1.164, 1.793, 0.213, 0.533, 2.112;  BT.601 full (JFIF) 1, 1.402, 0.344136, 0.714136, 1.772.
// The BT.601 limited row is believed to be what OpenCV's COLOR_YUV2RGB_NV12 evaluates; cv2 is absent here: parity unpinned.
struct ColorMatrix { int yoff, cy, cvr, cug, cvg, cub; };
__host__ __device__ inline ColorMatrix color_matrix(int m)
{
    if (m == MATRIX_BT709) return ColorMatrix{16, 1220542, 1880097, 223347, 558891, 2214593};
    if (m == MATRIX_BT601_FULL) return ColorMatrix{0, 1048576, 1470104, 360853, 748826, 1858077};
    return ColorMatrix{16, 1220542, 1673527, 409993, 852492, 2116026};
}
__host__ __device__ inline int clamp8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// R, G, B bytes of one (Y, U, V) sample; `>>` on a negative sum is the arithmetic shift
__host__ __device__ inline void yuv_to_rgb(const ColorMatrix &m, int Y, int U, int V, int *rgb)
{
    const int y = (Y - m.yoff > 0 ? Y - m.yoff : 0) * m.cy, u = U - 128, v = V - 128;
    rgb[0] = clamp8((y + m.cvr * v + (1 << 19)) >> 20);
    rgb[1] = clamp8((y - m.cug * u - m.cvg * v + (1 << 19)) >> 20);
    rgb[2] = clamp8((y + m.cub * u + (1 << 19)) >> 20);
}
// ---- JPEG files (yolo_*_jpegs, yolo_decode_jpegs): the reference reads a JPEG through its vendored stb_image (DN/image.c load_image_stb), whose
// IDCT, chroma upsampling and colour step are integer arithmetic.  The three are restated here, once, for the host twin (yolo_jpeg_to_rgb_host), the IDCT kernel
// (k_jpeg_idct, jpeg_ops.hip) and the frame reader (AtFrame, ew_ops.hip): the bar is bit equality with the compiled reference.  A decoded file is a frame whose
// planes are the component planes the IDCT writes: Y, then Cb and Cr at full size (444), half width (422), half width and height (420) or half height (440); GREY
// has Y alone.
// The formats carry their colour rule with them: the matrix of such a frame must be 0 and selects nothing.
enum { PIX_JPEG_GREY = 16, PIX_JPEG_444 = 17, PIX_JPEG_422 = 18, PIX_JPEG_420 = 19, PIX_JPEG_440 = 20 };
__host__ __device__ inline bool pix_is_jpeg(int format) { return format >= PIX_JPEG_GREY && format <= PIX_JPEG_440; }
// rows and bytes per row the chroma planes of an h x w JPEG frame must have (the component's own size, T.81 A.1.1: ceil(h * v / v_max) x ceil(w * h / h_max))
__host__ __device__ inline int jpeg_chroma_rows(int format, int h) { return format == PIX_JPEG_420 || format == PIX_JPEG_440 ? (h + 1) >> 1 : h; }
__host__ __device__ inline int jpeg_chroma_cols(int format, int w) { return format == PIX_JPEG_444 || format == PIX_JPEG_440 ? w : (w + 1) >> 1; }
// One 8-point pass of the reference's IDCT (stb_image.h:2163-2202 STBI__IDCT_1D, "derived from jidctint"; the constants are its stbi__f2f(k) = (int)(k * 4096 + 0.5)).
// With x0..x3 the even part plus the pass's rounding `bias` and t0..t3 the odd part: out[k] = (x[k] + t[3 - k]) >> shift, out[7 - k] = (x[k] - t[3 - k]) >> shift.
// Evaluated in unsigned so that coefficients no encoder writes wrap as on the reference's machine instead of overflowing an int.
__host__ __device__ inline void jpeg_idct_1d(const int *s, int bias, int shift, int *out)
{
    typedef unsigned U;
    U p2 = (U)s[2], p3 = (U)s[6];
    U p1 = (p2 + p3) * (U)2217;
    U t2 = p1 + p3 * (U)-7567, t3 = p1 + p2 * (U)3135;
    p2 = (U)s[0]; p3 = (U)s[4];
    U t0 = (p2 + p3) * 4096u, t1 = (p2 - p3) * 4096u;
    const U x0 = t0 + t3 + (U)bias, x3 = t0 - t3 + (U)bias, x1 = t1 + t2 + (U)bias, x2 = t1 - t2 + (U)bias;
    t0 = (U)s[7]; t1 = (U)s[5]; t2 = (U)s[3]; t3 = (U)s[1];
    p3 = t0 + t2;
    U p4 = t1 + t3;
    p1 = t0 + t3; p2 = t1 + t2;
    const U p5 = (p3 + p4) * (U)4816;
    t0 *= (U)1223; t1 *= (U)8410; t2 *= (U)12586; t3 *= (U)6149;
    p1 = p5 + p1 * (U)-3685; p2 = p5 + p2 * (U)-10497; p3 *= (U)-8034; p4 *= (U)-1597;
    t3 += p1 + p4; t2 += p2 + p3; t1 += p2 + p4; t0 += p1 + p3;
    out[0] = (int)(x0 + t3) >> shift; out[7] = (int)(x0 - t3) >> shift;
    out[1] = (int)(x1 + t2) >> shift; out[6] = (int)(x1 - t2) >> shift;
    out[2] = (int)(x2 + t1) >> shift; out[5] = (int)(x2 - t1) >> shift;
    out[3] = (int)(x3 + t0) >> shift; out[4] = (int)(x3 - t0) >> shift;
}
// the column pass keeps two extra bits (+512, >> 10); the row pass removes 17 bits, rounds, and adds the level shift 128 before it (stb_image.h:2225-2259).  The
// reference's all-zero-AC shortcut of the column pass (d[0] * 4) is what the general form yields for such a column: no special case is needed
enum { JPEG_IDCT_COL_BIAS = 512, JPEG_IDCT_COL_SHIFT = 10, JPEG_IDCT_ROW_BIAS = 65536 + (128 << 17), JPEG_IDCT_ROW_SHIFT = 17 };
// one dequantised block (natural order) -> 8 rows of 8 samples at `stride`
__host__ __device__ inline void jpeg_idct_block(const int16_t *d, uint8_t *out, size_t stride)
{
    int v[64], s[8], o[8];
    for (int c = 0; c < 8; ++c) {
        for (int r = 0; r < 8; ++r) s[r] = d[8 * r + c];
        jpeg_idct_1d(s, JPEG_IDCT_COL_BIAS, JPEG_IDCT_COL_SHIFT, o);
        for (int r = 0; r < 8; ++r) v[8 * r + c] = o[r];
    }
    for (int r = 0; r < 8; ++r) {
        jpeg_idct_1d(v + 8 * r, JPEG_IDCT_ROW_BIAS, JPEG_IDCT_ROW_SHIFT, o);
        for (int c = 0; c < 8; ++c) out[r * stride + c] = (uint8_t)clamp8(o[c]);
    }
}
// The chroma sample of pixel (y, x) of an h x w frame, from a component plane read through at(row, col) (stb_image.h:3183-3235 stbi__resample_row_h_2 and
// stbi__resample_row_hv_2, and the row bookkeeping of load_jpeg_image :3611-3645, as closed forms).  With wl = ceil(w / 2) samples in a plane row:
//   422  wl == 1: s[0].  x == 0: s[0];  x == 2 wl - 1: s[wl - 1];  x == 2 wl - 2: (3 s[wl - 2] + s[wl - 1] + 2) >> 2 -- the reference's last pair weighs the
//        NEIGHBOUR by 3 --;  else, i = x >> 1: (3 s[i] + s[x odd ? i + 1 : i - 1] + 2) >> 2
//   420  the near row is y >> 1, the far row (y >> 1) + 1 for odd y, - 1 for even y, clamped to 0 .. ceil(h / 2) - 1 (the component's rows, not the padded plane's);
//        t[i] = 3 near[i] + far[i].  wl == 1, x == 0 or x == 2 wl - 1: (t[x >> 1] + 2) >> 2;  else, i = x >> 1: (3 t[i] + t[x odd ? i + 1 : i - 1] + 8) >> 4
//   440  (stbi__resample_row_v_2, :3173-3181) the same near and far rows at full width: (3 near[x] + far[x] + 2) >> 2
template <typename At>
__host__ __device__ inline int jpeg_chroma(int format, int h, int w, int y, int x, const At &at)
{
    if (format == PIX_JPEG_444) return at(y, x);
    const int wl = (w + 1) >> 1, i = x >> 1, o = (x & 1) ? i + 1 : i - 1;
    if (format == PIX_JPEG_422) {
        if (wl == 1 || x == 0) return at(y, 0);
        if (i == wl - 1) return (x & 1) ? at(y, i) : (3 * at(y, i - 1) + at(y, i) + 2) >> 2;
        return (3 * at(y, i) + at(y, o) + 2) >> 2;
    }
    const int rows = (h + 1) >> 1, near = y >> 1, f = (y & 1) ? near + 1 : near - 1, far = f < 0 ? 0 : f > rows - 1 ? rows - 1 : f;
    if (format == PIX_JPEG_440) return (3 * at(near, x) + at(far, x) + 2) >> 2;
    const int t = 3 * at(near, i) + at(far, i);
    if (wl == 1 || x == 0 || x == 2 * wl - 1) return (t + 2) >> 2;
    return (3 * t + 3 * at(near, o) + at(far, o) + 8) >> 4;
}
// R, G, B of one (Y, Cb, Cr) sample (stb_image.h:3367-3391 stbi__YCbCr_to_RGB_row): 12-bit constants (int)(k * 4096 + 0.5) of 1.402, 0.71414, 0.34414, 1.772 shifted
// left by 8, and the Cb term of green with its low 16 bits masked off (how the reference's SIMD and scalar paths are kept equal)
__host__ __device__ inline void jpeg_ycc_to_rgb(int Y, int Cb, int Cr, int *rgb)
{
    const int yf = (Y << 20) + (1 << 19), cr = Cr - 128, cb = Cb - 128;
    rgb[0] = clamp8((yf + cr * 1470208) >> 20);
    rgb[1] = clamp8((yf + cr * -748800 + (int)((unsigned)(cb * -360960) & 0xffff0000u)) >> 20);
    rgb[2] = clamp8((yf + cb * 1858048) >> 20);
}
// R, G, B of pixel (y, x) of a JPEG frame whose bytes are read through byte(offset); GREY repeats Y (stb_image.h:3683-3685)
template <typename Byte>
__host__ __device__ inline void jpeg_frame_rgb(const FrameDesc &f, int y, int x, const Byte &byte, int *rgb)
{
    const int Y = byte((unsigned)f.offset[0] + (unsigned)y * (unsigned)f.pitch[0] + (unsigned)x);
    if (f.format == PIX_JPEG_GREY) { rgb[0] = rgb[1] = rgb[2] = Y; return; }
    int c[2];
    for (int p = 1; p <= 2; ++p) {
        const unsigned base = (unsigned)f.offset[p], pitch = (unsigned)f.pitch[p];
        c[p - 1] = jpeg_chroma(f.format, f.h, f.w, y, x, [&](int r, int col) { return byte(base + (unsigned)r * pitch + (unsigned)col); });
    }
    jpeg_ycc_to_rgb(Y, c[0], c[1], rgb);
}
// byte offsets of the samples of pixel (y, x) of a frame: chroma is taken from (y >> 1, x >> 1) of the FRAME (nearest, no interpolation).  NV12 / I420: o[0] Y, o[1] U,
// o[2] V; RGB24 / BGR24: o[c] the byte of output channel c (BGR swaps 0 and 2)
__host__ __device__ inline void frame_sample_offsets(const FrameDesc &f, int y, int x, unsigned *o)
{
    if (f.format >= PIX_RGB24) {
        const unsigned p = (unsigned)f.offset[0] + (unsigned)y * (unsigned)f.pitch[0] + (unsigned)x * 3u, sw = f.format == PIX_BGR24 ? 2u : 0u;
        o[0] = p + sw; o[1] = p + 1u; o[2] = p + 2u - sw;
        return;
    }
    o[0] = (unsigned)f.offset[0] + (unsigned)y * (unsigned)f.pitch[0] + (unsigned)x;
    const unsigned cy = (unsigned)y >> 1, cx = (unsigned)x >> 1;
    if (f.format == PIX_NV12) { o[1] = (unsigned)f.offset[1] + cy * (unsigned)f.pitch[1] + 2u * cx; o[2] = o[1] + 1u; }
    else { o[1] = (unsigned)f.offset[1] + cy * (unsigned)f.pitch[1] + cx; o[2] = (unsigned)f.offset[2] + cy * (unsigned)f.pitch[2] + cx; }
}
// whole frames, one per batch slot, fitted as launch_fit_images fits RGB images; fit: FIT_STRETCH, FIT_LETTERBOX, FIT_CV2 or FIT_CENTER_CROP.  One batch may mix formats
hipError_t launch_fit_frames(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, int n, int fit, int net_h, int net_w, void *out, int out_dt,
                             int out_stride, float post_mul, float post_add, hipStream_t s);
// windows of frames (yolo_detect_tiled_frames_u8): window i is rows y0 .., columns x0 .. of frame d_wins[i].image (its offset and pitch are not read); chroma is
// indexed by the pixel's position in the FRAME, so a window may start on an odd row or column.  FIT_STRETCH and FIT_LETTERBOX
hipError_t launch_fit_frame_windows(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, const WinDesc *d_wins, int n, int fit, int net_h, int net_w,
                                    void *out, int out_dt, int out_stride, float post_mul, float post_add, hipStream_t s);
// views of frames (yolo_classify_views_frames_u8): slot i is one view of frame d_views[i].offset -- the field holds the FRAME INDEX here, not a byte offset; h, w: the
// frame's -- with launch_fit_views' meaning: fit FIT_STRETCH, FIT_LETTERBOX, FIT_CV2 or FIT_CENTER_CROP, mirrored where flip != 0, or FIT_TEN_CROP.  A mirror or a
// crop moves coordinates of the fitted / resized image only: chroma stays indexed by the pixel's position in the frame
hipError_t launch_fit_frame_views(const uint8_t *pixels, size_t bytes, const FrameDesc *d_frames, const ViewDesc *d_views, int n, int fit, int net_h, int net_w,
                                  void *out, int out_dt, int out_stride, float post_mul, float post_add, hipStream_t s);
// one frame -> the [h][w][3] uint8 image of the colour rule (yolo_op_frame_to_rgb)
hipError_t launch_frame_to_rgb(const uint8_t *pixels, size_t bytes, const FrameDesc &frame, uint8_t *out, hipStream_t s);
// JPEG files: one component plane of one file of a batch -- blocks block0 .. of the batch's coefficient array are its 8 x 8 blocks in raster order, bw across; the
// plane begins at byte `offset` of the surface (a multiple of 8) with rows `pitch` bytes apart (a multiple of 8, >= 8 bw).  The table is sorted by block0
struct JpegPlane { unsigned block0, bw, offset, pitch; };
// the IDCT of a whole batch in one launch (jpeg_ops.hip): coef [blocks][64] int16, dequantised, natural order (16-byte aligned) -> every plane of the table
hipError_t launch_jpeg_idct(const int16_t *coef, const JpegPlane *d_planes, int nplanes, size_t blocks, uint8_t *out, size_t out_bytes, hipStream_t s);
hipError_t launch_upsample2x(const TView &in, const TView &out, int bilinear, hipStream_t s);
hipError_t launch_maxpool(const TView &in, const TView &out, int size, int stride, int pad, hipStream_t s);
hipError_t launch_reorg(const TView &in, const TView &out, int stride, int darknet, hipStream_t s);
// out = (a * sa + b * sb) * so   (the scales are the fp8 tensor scales; 1 for bf16 / fp32)
hipError_t launch_add(const TView &a, const TView &b, const TView &out, hipStream_t s, float sa = 1.f, float sb = 1.f, float so = 1.f);
hipError_t launch_copy(const TView &in, const TView &out, hipStream_t s);
// x = act(x) in place on the view's real channels (k_activate; any of ACT_*, fp32 / bf16 / fp16 or, `pair`, interleaved split-fp16 pairs): the
// post-activation of a layer whose activation is outside the slope family
hipError_t launch_activate(const TView &x, bool pair, int act, hipStream_t s);
// darknet's general [shortcut] (DN/blas.c:68-92 shortcut_cpu + activate_array) in one launch (k_shortcut): out = act(a + gather(b)), a / out
// [n, h2, w2, c2] the layer's input and output, b [n, h1, w1, c1] the `from` tensor.  shortcut_geom restates shortcut_cpu's integers: stride
// = w1 / w2 and sample = w2 / w1 (integer divisions, each raised to 1), the minima, and ok = the reference's two assertions
struct ShortcutGeom { int stride, sample, minw, minh, minc; bool ok; };
ShortcutGeom shortcut_geom(int w1, int h1, int c1, int w2, int h2, int c2);
hipError_t launch_shortcut(const TView &a, const TView &b, const TView &out, bool pair, int act, hipStream_t s);
// [local] (locally connected, DN/local_layer.c): w [locations][filters][k][k][C] in the tensors' type, bias [locations][filters] fp32
hipError_t launch_local(const TView &in, const TView &out, const void *w, const float *bias, int k, int stride, int pad, int act, hipStream_t s);
hipError_t launch_to_f32(const TView &in, float *out, hipStream_t s, float scale = 1.f);   // dense NHWC fp32 copy (* scale)
hipError_t launch_from_f32(const float *in, const TView &out, hipStream_t s, float scale = 1.f);   // (in * scale) -> view
// split fp16 storage (YOLO_FP16X2; ew_ops.hip).  Two layouts of a pair tensor of Cp padded channels:
//   PAIR_ILV  [pixel][stride >= 2 * Cp], Cp a multiple of 32: per 32-channel group 32 hi then 32 lo (every layer output; round 6)
//   PAIR_B3   [pixel][3 * Cp], Cp a multiple of 8: blocks hi | lo | hi (the network INPUT only: 8 padded channels, rounds 4-5's form)
enum { PAIR_ILV = 0, PAIR_B3 = 1 };
hipError_t launch_split_from_f32(const float *in, int in_stride, void *out, int out_stride, int Cp, size_t npix, hipStream_t s, int layout = PAIR_ILV);   // fp32 [pixel][in_stride >= Cp] -> pairs
hipError_t launch_split_to_f32(const void *in, int in_stride, int Cp, float *out, int out_stride, size_t npix, hipStream_t s, int layout = PAIR_ILV);      // pairs -> fp32 (hi + lo)
hipError_t launch_upsample2x_pair(const TView &in, const TView &out, int bilinear, hipStream_t s);      // 2x upsample of an interleaved pair tensor (join, fp32 lerp, split) in one launch
hipError_t launch_add_split(const void *a, int a_stride, const void *b, int b_stride, void *out, int out_stride, int Cp, size_t npix, hipStream_t s);      // shortcut on interleaved pair tensors

// ---- classifier tail (cls_ops.hip) ---------------------------------------------------------------
// darknet's [avgpool] (always global, DN/avgpool_layer.c:40-55): in [n, h, w, c] -> out [n, 1, 1, c] in the same tensor form (bf16 /
// fp16 / fp32, or interleaved split-fp16 pairs with in_pair); fp32 sums, then / (h * w).  Both views may be channel windows.
hipError_t launch_avgpool(const TView &in, bool in_pair, const TView &out, hipStream_t s);
#define CLS_SOFTMAX_MAX 8192          // logits of one softmax group (staged in LDS once)
#define CLS_TOPK_MAX 32
// darknet's [softmax] (DN/blas.c:305-321) over x [n][x_stride] fp32, `groups` runs of `len` logits per image -> probs [n][p_stride];
// top_k > 0 (groups == 1): the same launch also writes the top_k best of every image to cls / topk_probs [n][top_k], probability
// descending, equal probabilities by ascending class (the order of a stable sort by -prob); slots past `len`: class -1, probability 0
struct SoftmaxArgs {
    const float *x; int x_stride;
    int n, groups, len; float temperature;
    float *probs; int p_stride;
    int top_k; int *cls; float *topk_probs;
};
hipError_t launch_softmax_topk(const SoftmaxArgs &a, hipStream_t s);
// [avgpool] of an fp32 tensor followed by [softmax] in ONE launch (a.x / a.x_stride are not read: the logits are the pooled `in`);
// the pooled vector is also written to pooled [n][pooled_stride]
bool avgpool_softmax_ok(const TView &in, const SoftmaxArgs &a);
hipError_t launch_avgpool_softmax(const TView &in, float *pooled, int pooled_stride, const SoftmaxArgs &a, hipStream_t s);
// Multi-view classification (yolo_classify_views_u8): rows [n * views][len] fp32, slot = image * views + view -> sums [n][len] with
// sums[i][c] = ((((0 + p_0) + p_1) + ...) + p_{views-1}) * scale -- axpy_cpu's order, then one multiply --, and, top_k > 0, the top_k best of every scaled row to
// cls / topk [n][top_k] in the order of launch_softmax_topk (the same device code), from the same launch.  work [n][len]: the selection's scratch (top_k > 0).
// Any len >= 1; 1 <= views <= VIEWS_MAX.  Values of -inf are never selected.
enum { VIEWS_MAX = 32 };
struct ViewReduceArgs { const float *rows; int n, views, len; float scale; float *sums, *work; int top_k; int *cls; float *topk; };
hipError_t launch_view_reduce(const ViewReduceArgs &a, hipStream_t s);

// ---- vector-input networks and sequences (seq_ops.hip; DN/examples/rnn.c test_char_rnn, DN/utils.c:592-603 sample_array) ----
// x fp32 [n][len] -> rows [n][row_stride] of `dt` (bf16 / fp16 / fp32), the elements len .. row_stride - 1 of every row zero; row_stride a multiple of 8
hipError_t launch_vector_in(const float *x, int n, int len, void *rows, int row_stride, int dt, hipStream_t s);
// tokens int32 [n] -> one-hot rows of the same form, each written whole (a token outside 0 .. len - 1: a row of zeros)
hipError_t launch_token_in(const int32_t *tokens, int n, int len, void *rows, int row_stride, int dt, hipStream_t s);
// One workgroup per stream samples a token from its fp32 probability row (probs [n][p_stride], len <= CLS_SOFTMAX_MAX values) as rnn.c:290-293 and
// sample_array do, in their order, in fp32: p < clip -> 0; the sum in index order; every element times (float)(1. / sum); r = u, r -= a[i] until r <= 0,
// else len - 1 (a row that is clipped whole included: NaN compares false).  tokens_out [n]; next_rows (may be null): the stream's one-hot row as
// launch_token_in writes it; probs_out (may be null): the row as it was read, dense [n][len]
struct SampleArgs {
    const float *probs; int p_stride, n, len;
    const float *uniforms; float clip;
    int32_t *tokens_out;
    void *next_rows; int row_stride, dt;
    float *probs_out;
};
hipError_t launch_sample(const SampleArgs &a, hipStream_t s);

// ---- hierarchical softmax: darknet's softmax trees (tree_ops.hip; DN/tree.c, DN/softmax_layer.c:41-48, DN/region_layer.c:171-181) ----
// A tree on the device.  parent / child / leaf [n], goff / gsize [groups] as DN/tree.c:83-139 builds them; order [groups]: the groups
// sorted by depth (the root group first), lvl [levels + 1]: where each depth begins in `order`.  A group's parent node lies in a
// shallower group, so a pass over `order` level by level forms every absolute probability as cond[j] * abs[parent[j]] exactly.
struct TreeDev { int n, groups, levels; const int *parent, *child, *goff, *gsize, *leaf, *order, *lvl; };
// where the n logits of row r lie: x + (r / na) * cell_stride + (r % na) * an_stride + off (a dense matrix: na 1, cell_stride = its
// row stride; a [region] head's raw tensor: one cell per pixel, na boxes of 5 + classes values each, off 5)
struct TreeRows { const float *x; size_t rows; int na, cell_stride, an_stride, off; };
enum { TREE_CONDITIONAL = 0, TREE_ABSOLUTE = 1, TREE_LEAVES = 2 };
// one softmax per group with e = exp(x / t - max / t) (DN/blas.c:305-321) -> out [rows][out_stride]; mode TREE_ABSOLUTE: then
// hierarchy_predictions (DN/tree.c:37-51), TREE_LEAVES: with only_leaves.  top_k > 0: the best top_k of every row (the order of
// launch_softmax_topk) to cls / topk_probs [rows][top_k]
hipError_t launch_tree_softmax(const TreeDev &t, const TreeRows &x, float temperature, int mode, float *out, int out_stride,
                               int top_k, int *cls, float *topk_probs, hipStream_t s);
// hierarchy_top_prediction (DN/tree.c:53-81) of every row, walking down from the root over the raw logits: per step one group's
// softmax (temperature 1), scaled by the parent's absolute probability.  labels [rows]
hipError_t launch_tree_top(const TreeDev &t, const TreeRows &x, float hier_thresh, int *labels, hipStream_t s);
struct DecodeArgs;
// [region] head with a tree, full form: det rows (x, y, w, h, objectness, ABSOLUTE class probabilities)
hipError_t launch_decode_region_tree(const DecodeArgs &a, const TreeDev &t, hipStream_t s);
// ... its rows scored from those absolute probabilities: scores[row] = objectness, labels[row] = hierarchy_top_prediction;
// det / scores / labels are [nrows] consecutive rows
hipError_t launch_tree_score_rows(const float *det, size_t nrows, int attrs, const TreeDev &t, float hier_thresh, float *scores, int *labels, hipStream_t s);
// ... descent form (yolo_detect*): box4, scores, labels of every row straight from the raw head tensor, no decoded tensor; the tree is
// walked for the boxes whose objectness reaches a.reject_below only (the others: label 0)
hipError_t launch_decode_region_tree_lean(const DecodeArgs &a, const TreeDev &t, float hier_thresh, float *scores, int *labels, hipStream_t s);
// get_region_detections with a tree (DN/region_layer.c:412-424) over the records launch_darknet_boxes wrote (rec [count][attrs], src:
// the decoded row of each): the class columns become zeros but prob[top prediction] = objectness > thresh ? objectness : 0, or,
// with map (200 device ints), prob[j < 200] = objectness * abs[map[j]] gated by thresh
hipError_t launch_darknet_tree_probs(const float *det, int attrs, const TreeDev &t, float thresh, float hier_thresh, const int *map200,
                                     float *rec, const int *src, const int *count, int cap, hipStream_t s);
// the tree form of launch_head_darknet_layout's region branch: conditional probabilities, planar
hipError_t launch_head_darknet_layout_tree(const float *raw, int raw_stride, int cells, int na, int classes, const TreeDev &t, float *out, hipStream_t s);

// ---- head decode + postprocess (post_ops.hip) ---------------------------------------------------
struct DecodeArgs {
    const float *raw; int raw_stride;   // [n, gh*gw, raw_stride] fp32 head conv output, cell = row * gw + col
    int n, gh, gw, na, classes;         // grid rows x columns
    float anchors[2 * 16];              // yolo: (w / stride_x, h / stride_y); region: grid units; masked order
    int img_h, img_w;                   // network input; per-axis strides img_w / gw, img_h / gh
    int mode;                           // yolo_decode
    int region;                         // 1: softmax/region head
    float *det; int rows_total; int row_off;   // det [n, rows_total, 5+classes]; nullptr: the decoded tensor is not materialised ...
    float *box4;                        // ... only (cx, cy, w, h) of every row, [n, rows_total, 4] (yolo heads, with scores/labels)
    float reject_below;                 // lean form: a box whose objectness is below this cannot reach the caller's score threshold
                                        // (score = objectness * class probability <= objectness): its class work is skipped and its
                                        // score is reported as the objectness itself.  -inf: every box is scored
};
#ifdef __HIPCC__
// Box and objectness of one [region] box, the ONE place this arithmetic is written (V2/decode.py:13-47; k_decode_region and its tree
// twins; on a gh x gw grid DN/region_layer.c get_region_box): p the box's 5 + classes raw values, o (cx, cy, w, h, objectness), x and w
// normalised by the grid's columns gw, y and h by its rows gh
__device__ __forceinline__ float region_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
// In two steps: region_act, the value darknet's [region] layer holds in l.output for k < 5 (logistic on x, y and objectness, w and h raw), and
// region_box_form, the box formula on such a value; the frame-averaged decode (k_decode_avg<true>) takes the mean between the two
__device__ __forceinline__ float region_act(int k, float x) { return (k == 2 || k == 3) ? x : region_sigmoid(x); }
__device__ __forceinline__ float region_box_form(int k, float v, int cell, int gw, int gh, const float *anchor_wh)
{
    const float GW = (float)gw, GH = (float)gh;
    if (k == 0) return ((float)(cell % gw) + v) / GW;
    if (k == 1) return ((float)(cell / gw) + v) / GH;
    if (k == 2) return (anchor_wh[0] * expf(v)) / GW;
    if (k == 3) return (anchor_wh[1] * expf(v)) / GH;
    return v;
}
__device__ __forceinline__ float region_box_attr(int k, const float *p, int cell, int gw, int gh, const float *anchor_wh)
{
    return region_box_form(k, region_act(k, p[k < 4 ? k : 4]), cell, gw, gh, anchor_wh);
}
// Attribute k < 5 of a box in darknet's layer-output layout (DN/yolo_layer.c:143-152, DN/region_layer.c:163-173): the logistic,
// 1. / (1. + exp(-x)) in double like DN/activations.h:38, on x, y and objectness; w and h stay raw
__device__ __forceinline__ float darknet_layout_box_attr(int k, const float *p)
{
    return (k == 2 || k == 3) ? p[k] : (float)(1. / (1. + exp(-(double)p[k])));
}
#endif
// Lean decode of up to four [yolo] heads in ONE launch (yolo_detect*: the decodes of a three-scale network are three short,
// latency-bound launches otherwise; the head tensors keep their own buffers, so the early heads can wait for the last one)
struct LeanHead { const float *raw; const float *obj; int raw_stride, gh, gw, na, row_off; long box_begin; float sx, sy; float anchors[2 * 16]; };      // obj: compact objectness-logit plane [n * gh * gw][na] written by the head conv, or nullptr (read from raw); sx, sy: the strides img_w / gw, img_h / gh (integer divisions) as floats
struct LeanArgs {
    int nheads; LeanHead h[4];
    long total;                          // boxes of all heads: n * sum(gh * gw * na)
    int n, classes, mode, rows_total;
    float *box4; float reject_below;
    uint4 *list; unsigned *list_count; unsigned list_cap;      // boxes that pass the objectness pre-filter (descriptor each); *list_count = entries, zero between launches
};
hipError_t launch_decode_lean(const LeanArgs &a, float *scores, int *labels, hipStream_t s);
// scores/labels (nullable): per-row max_k(obj*cls_k) and its first argmax, written alongside the decode
hipError_t launch_decode(const DecodeArgs &a, float *scores, int *labels, hipStream_t s);
// Frame averaging ("Frame averaging"; DN/examples/demo.c remember_network + avg_predictions): a ring of the last K ACTIVATED head tensors per
// stream -- what darknet holds in l.output: logistic on x, y, objectness (and a [yolo] head's classes), a [region] head's class softmax, w and h raw.
// ring [K][max_batch][E] fp32, E = sum over the heads of cells * na * (5 + classes), a head's part at `off` in its own [cell][anchor * attrs] order;
// pos [max_batch]: the slot the stream's next step writes.  Both live in device memory: a captured step replays with these arguments.
struct RingArgs { float *ring; const int *pos; int K, max_batch; size_t E, off; float alpha; };      // alpha = (float)(1. / K)
// launch_decode's full form over the mean: per (stream, cell) one wave writes the activated values to slot pos[stream], forms avg = sum over the slots
// j = 0 .. K - 1 (slot order) of alpha * slot[j], and applies the box arithmetic to it.  a.det, scores, labels non-null; a [yolo] head or a
// [region] head without a tree, 5 + classes <= 128, raw_stride >= na * (5 + classes).  The positions are not advanced: launch_ring_advance, once all heads of the step are decoded
hipError_t launch_decode_avg(const DecodeArgs &a, const RingArgs &g, float *scores, int *labels, hipStream_t s);
hipError_t launch_ring_advance(int *pos, int n, int K, hipStream_t s);      // pos[b] = (pos[b] + 1) % K for the streams b < n
// keep[b][e] <-> ring[pos[b]][b][e] for every stream: the one slot a step writes while the positions stand still (the timing entry points)
hipError_t launch_ring_slot_move(float *ring, float *keep, const int *pos, int max_batch, size_t E, int restore, hipStream_t s);
// YOLOv1 [detection] head (row D1): raw [n][raw_stride] fp32 = [cls S*S*C | conf S*S*B | box S*S*B*4] -> det rows (cx, cy, w, h, conf, cls...)
hipError_t launch_decode_v1(const float *raw, int raw_stride, int n, int side, int num, int classes, int sqr, float *det, int rows_total,
                            int row_off, float *scores, int *labels, hipStream_t s);

struct PostArgs {
    const float *det; int n, rows, attrs;
    float score_thr, iou_thr; int max_out, nms_mode, select_mode;
    const float *box4;                  // non-null: [n, rows, 4] (cx,cy,w,h) rows written by the lean decode; `det` is not read
    int scores_ready;                   // 1: scores/labels were produced by the decode kernel already
    int corners_in;                     // 1: det rows already hold (x0,y0,x1,y1) instead of (cx,cy,w,h)
    int img_h, img_w;                   // V2 numpy flavour only: pixel box scaling (V2/utils.py:32-43); 0 = off
    // workspace (device), sized for n images: scores/labels/cand/slabel/sscore [n*rows], sbox float4 [n*rows],
    // keys u64 [n*rows_pow2]
    float *scores; int *labels; int *cand; unsigned long long *keys; int rows_pow2;
    float4 *sbox; int *slabel; float *sscore;
    void *boxes_out; int *counts_out;   // yolo_box [n*max_out], int [n] (device)
    // optional: the decoded-tensor row (0 .. rows-1, within its image) every kept record came from, [n*max_out], -1 in unused slots;
    // needs the workspace srow [n*rows].  nullptr: not reported
    int *rows_out; int *srow;
    unsigned *zero_word;                // optional: a device word this launch resets to 0 (the lean decode's list counter)
    // optional per-image source geometry (yolo_detect_images_*): nullptr keeps the single-shape path above.  fit FIT_LETTERBOX: every
    // candidate box is un-letterboxed for its image (correct_yolo_boxes) before NMS, in source pixels unless geom_relative; the other
    // fits: NMS runs in network space and, with geom_pixels, the kept records are scaled to the image afterwards (a separate launch).
    // NMS_PER_CLASS with geom_pixels: the image's (h, w) is V2's image_shape.
    const ImgDesc *geom; int geom_fit, geom_pixels, geom_relative, netw, neth;
    int geom_net_pixels;                // 1: the decoded boxes are in network-input pixels (DECODE_PIXEL [yolo] heads), 0: normalised
};
hipError_t launch_postprocess(const PostArgs &a, hipStream_t s);
// Cross-window merge of yolo_detect_tiled_u8 ("Tiled detection").  After a network step over the windows first .. first + nb - 1
// of the window table (batch slot b holds window first + b), every row that passes select_mode against score_thr is mapped to its source
// image's pixels and written to that image's merged list, ordered by (window, row) whatever the scheduling: launch 1 counts the passing rows
// of every window; launch 2 places a window behind what its image held before the step (run_in) and behind the image's earlier windows of
// the step, and writes its rows in row order.  run_in / run_out are two arrays the caller swaps between steps (a step never writes what it
// reads); the block of an image's LAST window writes total[image] and, above `cap`, reports ((image << 32) | count) to *overflow by an
// atomic minimum (the lowest such image wins; the word starts as all ones).  Rows beyond cap are counted, not written.
#define TILE_MERGE_CAP 32768             // k_nms_image's limit: one image's merged candidates
struct TileMergeArgs {
    const WinDesc *wins; int nwin, first, nb;
    int rows, attrs;                     // rows per window, attributes of a `det` row
    const float *det, *box4;             // the step's boxes, as PostArgs: box4 non-null = the lean decode's [nb, rows, 4], det is not read
    const float *scores; const int *labels;      // [nb, rows]
    float score_thr; int select_mode;
    int fit, netw, neth;                 // FIT_STRETCH / FIT_LETTERBOX of the windows into netw x neth
    int net_pixels;                      // 1: the boxes are in network-input pixels (DECODE_PIXEL [yolo] heads): divided by the network size first
    int centre;                          // 1: merged boxes are (cx, cy, w, h) (YOLO_NMS_DARKNET reads that form), 0: corners (x0, y0, x1, y1)
    int cap;                             // merged rows per image (<= TILE_MERGE_CAP)
    float *m_scores; int *m_labels; float4 *m_box;      // [images, cap]
    int *wcount;                         // [nb]: passing rows per window of this step
    const int *run_in; int *run_out; int *total;        // [images]
    unsigned long long *overflow;
};
hipError_t launch_tile_merge(const TileMergeArgs &a, hipStream_t s);
// the kept records of image i divided by that image's width (x0, x1) and height (y0, y1): relative = 1 of yolo_detect_tiled_u8
hipError_t launch_tile_relative(void *boxes, const int *counts, int max_out, const ImgDesc *descs, int n, hipStream_t s);
// row S on its own: score = max_k(obj * cls_k), label = first arg-max, of nrows decoded rows (objectness_mode: V3/yolo_v3.py:385,397)
void launch_score_rows(const float *det, size_t nrows, int attrs, float *scores, int *labels, hipStream_t s, int objectness_mode = 0);
hipError_t launch_letterbox_chw(const float *img, int iw, int ih, int net_h, int net_w, void *out, int out_dt, int out_stride, hipStream_t s, int nch = 3);
hipError_t launch_nms_dets(const float4 *boxes, float *prob, float *objectness, int n, int classes, float thresh, int by_obj, hipStream_t s);
// darknet get_network_boxes on the device (post_ops.hip): ordered compaction + letterbox correction of one image's decoded rows
struct DnBoxesArgs {
    const float *det; int attrs;          // decoded rows of ONE image [rows][attrs]
    int nheads, kind[8], cells[8], na[8], off[8];   // per head: 0 yolo / 1 region, grid cells (rows x columns), anchors, first row
    float thresh; int w, h, netw, neth, relative;
    // kind 2, a [detection] head (get_detection_detections, DN/detection_layer.c:225-254): every one of the side * side * num boxes,
    // straight from the layer's input vector (= its output in inference): raw [classes | confidences | boxes]
    const float *raw; int side, classes, sqr;
    float *rec;                           // [cap][attrs]: x, y, w, h, objectness, prob[classes]; nullptr = count only
    int *src;                             // workspace [>= cap] (row index of every kept box)
    int *count; int cap;
};
hipError_t launch_darknet_boxes(const DnBoxesArgs &a, hipStream_t s);
// last head's raw output -> darknet's layer-output layout (planar, activations applied); image 0
hipError_t launch_head_darknet_layout(const float *raw, int raw_stride, int cells, int na, int classes, int region, float *out, hipStream_t s);
// darknet letterbox_image / resize_image on a planar float image -> planar float canvas w x h (DN/image.c:960-981)
hipError_t launch_letterbox_planar(const float *img, int iw, int ih, int w, int h, int embed, float *out, hipStream_t s);
hipError_t launch_boxes_to_corners(const float *in, float *out, size_t nrows, int attrs, hipStream_t s);
