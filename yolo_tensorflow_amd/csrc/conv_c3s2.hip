// conv 3x3/s1 32 -> 64 + shortcut, immediately consumed by conv 3x3/s2/pad 1 64 -> 128, for gfx950: darknet-53's cfg layers 3, 4 and 5
// in ONE launch.  Run as conv_halo_c32_c64 + conv_s2_c64_c128 the layer-4 tensor (208 x 208 x 64 at 416 x 416: 177 MB at batch 32) is
// written once and read once; here it lives in LDS only.  A persistent workgroup owns 4 x 8 stride-2 output pixels at a time:
//
//   windows    the 9 x 17 layer-4 pixels a tile needs are computed from an 11 x 19 window of layer 2 (32 channels, 64-B records, the
//              chunk swizzle of conv_halo_c32_c64) and the 9 x 17 window of the shortcut source (64 channels).  Both come by LDS-DMA
//              one step ahead.  The shortcut window is fetched STRAIGHT INTO the layer-4 tile, in the record layout of
//              conv_s2_c64_c128 (144-B pixel records, 16-B piece index XOR ((window row >> 1) & 1)): conv3's epilogue adds its result
//              to the record in place.  Pixels outside the image arrive as zeros and are written back as zeros, by position: the
//              stride-2 conv pads LAYER 4, and conv3 of a padded window (bias, leaky) is not zero.
//   waves      0-3 PRODUCE: conv3 of tile i+1, one group of 16 window pixels at a time x 64 channels, filters in registers (144), the
//              rounding points of conv_halo_c32_c64 (bias, leaky, round; + shortcut, round).  4-7 CONSUME: the stride-2 conv of tile i,
//              wave w = output channels 32 w .. 32 w + 31 x the tile's 32 pixels, the K order (tap, channel half) and the
//              register-resident filters (144) of conv_s2_c64_c128, results staged in LDS; the whole-line stores of tile i-1 go first.
//              A wave cannot hold both filter sets, so the roles are split as in the stem -- and every SIMD then has one wave of each.
//   ring       layer-4 tiles: three slots (filled by DMA for i+2 | conv3 of i+1 | read by the stride-2 conv of i); layer-2 windows and
//              staged output tiles: two each.  ONE barrier per step; only producers issue LDS-DMA, so their vmcnt(0) before it is
//              exact, and consumers never wait for their stores.
//   LDS        3 x 22528 + 2 x 14336 + 2 x 8704 = 113664 bytes
// Bit-identical to the two launches: same K order per accumulator, same rounding points.
#include "kernels.h"
#include "device_common.h"

constexpr int CS_TH = 4, CS_TW = 8;                          // stride-2 output tile
constexpr int CS_LH = 2 * CS_TH + 1, CS_LW = 2 * CS_TW + 1;  // layer-4 window: 9 x 17
constexpr int CS_LPIX = CS_LH * CS_LW;                       // 153
constexpr int CS_GROUPS = (CS_LPIX + 15) / 16;               // 10 groups of 16 window pixels (the last holds 9)
[[maybe_unused]] constexpr int CS_NG = (CS_GROUPS + 3) / 4;                   // groups per producer wave: 3 (waves 0-1) or 2
constexpr int CS_PITCH = 144;                                // bytes of one layer-4 pixel record: 8 data pieces + 1 pad piece
constexpr int CS_L4_CHUNKS = (CS_LPIX * (CS_PITCH / 16) + 63) / 64;      // 22 LDS-DMA instructions per tile
constexpr int CS_L4_BYTES = CS_L4_CHUNKS * 1024;             // 22528
[[maybe_unused]] constexpr int CS_L4_K = (CS_L4_CHUNKS + 3) / 4;              // per producer wave: 6
constexpr int CS_IH = CS_LH + 2, CS_IW = CS_LW + 2;          // layer-2 window: 11 x 19
constexpr int CS_INPIX = CS_IH * CS_IW;                      // 209
constexpr int CS_IN_CHUNKS = (CS_INPIX * 4 + 63) / 64;       // 14
constexpr int CS_IN_BYTES = CS_IN_CHUNKS * 1024;             // 14336
[[maybe_unused]] constexpr int CS_IN_K = (CS_IN_CHUNKS + 3) / 4;              // per producer wave: 4
constexpr int CS_OPITCH = 128 * 2 + 16;                      // staged output rows
constexpr int CS_OUT_BYTES = CS_TH * CS_TW * CS_OPITCH;      // 8704
constexpr int CS_NW = 8;
constexpr size_t CS_LDS = (size_t)3 * CS_L4_BYTES + 2 * CS_IN_BYTES + 2 * CS_OUT_BYTES;
// the lanes of the last group that hold no window pixel read defined bytes of the fetched pieces
static_assert(((CS_GROUPS * 16 - 1) / CS_LW + 2) * CS_IW + (CS_GROUPS * 16 - 1) % CS_LW + 2 < CS_IN_CHUNKS * 16, "conv3: reads past the layer-2 window slot");

template <bool H16>
__global__ __launch_bounds__(64 * CS_NW) void conv_c3s2_c32_c64_c128(const C3S2Args a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (H16) fp16_saturating_mode();      // fp16 conversions saturate
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int sub = wave & 3;                                    // index among the four waves of this wave's role

    const int Ho = (a.H - 1) / 2 + 1, Wo = (a.W - 1) / 2 + 1;
    const int tiles_x = (Wo + CS_TW - 1) / CS_TW, tiles_y = (Ho + CS_TH - 1) / CS_TH;
    const int per_img = tiles_x * tiles_y, ntiles = a.N * per_img;
    const int G = (int)gridDim.x;
    const int nt = (ntiles - (int)blockIdx.x + G - 1) / G;       // tiles of this workgroup: blockIdx.x + j * G, j < nt
    struct TilePos { int n, ty, tx; };
    auto tile_pos = [&](int j) { const int tile = (int)blockIdx.x + j * G; TilePos q; q.n = tile / per_img; const int tr = tile - q.n * per_img; q.ty = tr / tiles_x; q.tx = tr - q.ty * tiles_x; return q; };

    char *const l4b = smem, *const inb = smem + 3 * CS_L4_BYTES, *const lob = inb + 2 * CS_IN_BYTES;

    if (wave < 4) {
        // =========================================== producers ===========================================
        bf16x8 fw[4][9];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int t = 0; t < 9; ++t)
                fw[ct][t] = *(const bf16x8 *)((const bf16_t *)a.w3 + (size_t)(ct * 16 + l15) * a.Kpad3 + t * 32 + lq * 8);
        f32x4 bv[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) bv[ct] = *(const f32x4 *)(a.b3 + ct * 16 + lq * 4);
        const float slope = act_slope(a.act3);
        __amdgpu_buffer_rsrc_t rin = buf_rsrc(a.in);
        __amdgpu_buffer_rsrc_t rres = buf_rsrc(a.res);

        // the pieces this lane requests for every tile.  Shortcut window -> layer-4 slot: LDS piece g = (sub + 4 k) * 64 + lane is piece
        // g % 9 of window pixel g / 9 (conv_s2_c64_c128's layout); layer-2 window: piece g & 3 of window pixel g >> 2 (conv_halo_c32_c64's)
        unsigned relr[CS_L4_K]; int wyxr[CS_L4_K];               // byte offset from the window's first pixel; window row | column << 8 (-1: no request)
#pragma unroll
        for (int k = 0; k < CS_L4_K; ++k) {
            const int g = (sub + 4 * k) * 64 + lane;
            const int px = g / 9, j = g - px * 9;
            const int wy = px / CS_LW, wx = px - wy * CS_LW;
            const bool valid = px < CS_LPIX && j < 8;
            relr[k] = (unsigned)(((wy * a.W + wx) * a.res_stride + ((j ^ ((wy >> 1) & 1)) * 8)) * 2);
            wyxr[k] = valid ? (wy | (wx << 8)) : -1;
        }
        unsigned reli[CS_IN_K]; int wyxi[CS_IN_K];
#pragma unroll
        for (int k = 0; k < CS_IN_K; ++k) {
            const int g = (sub + 4 * k) * 64 + lane;
            const int px = g >> 2, pc = g & 3;
            const int ry = px / CS_IW, rx = px - ry * CS_IW;
            const int sc = pc ^ (2 * ((px >> 2) & 1));           // source chunk that belongs in this physical slot
            reli[k] = (unsigned)(((ry * a.W + rx) * a.in_stride + sc * 8) * 2);
            wyxi[k] = px < CS_INPIX ? (ry | (rx << 8)) : -1;
        }
        // one producer step: request the windows of tile jf, run conv3 of tile jc (its windows landed before the previous barrier).
        // Every LDS region is its own __restrict__ parameter, so that the requests cannot alias conv3's reads.
        auto produce = [&](int jf, int jc, char *__restrict__ l4_fill, char *__restrict__ in_fill, const char *__restrict__ in_cur, char *__restrict__ l4) {
            if (jf < nt) {
                const TilePos q = tile_pos(jf);
                const int iy0 = 2 * q.ty * CS_TH - 1, ix0 = 2 * q.tx * CS_TW - 1;      // layer-4 pixel of window record (0, 0)
                // (mod 2^32: the sum with rel is a valid offset wherever the pixel is inside the image)
                const unsigned baser = (unsigned)(((q.n * a.H + iy0) * a.W + ix0) * a.res_stride * 2);
                const unsigned basei = (unsigned)(((q.n * a.H + iy0 - 1) * a.W + ix0 - 1) * a.in_stride * 2);
#pragma unroll
                for (int k = 0; k < CS_L4_K; ++k) {
                    const int c = sub + 4 * k;
                    if (c < CS_L4_CHUNKS) {
                        const int wy = wyxr[k] & 0xff, wx = (wyxr[k] >> 8) & 0xff;
                        const bool ok = wyxr[k] >= 0 && (unsigned)(iy0 + wy) < (unsigned)a.H && (unsigned)(ix0 + wx) < (unsigned)a.W;
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rres, (lds_void *)(l4_fill + c * 1024), 16, ok ? baser + relr[k] : 0x80000000u, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int k = 0; k < CS_IN_K; ++k) {
                    const int c = sub + 4 * k;
                    if (c < CS_IN_CHUNKS) {
                        const int ry = wyxi[k] & 0xff, rx = (wyxi[k] >> 8) & 0xff;
                        const bool ok = wyxi[k] >= 0 && (unsigned)(iy0 - 1 + ry) < (unsigned)a.H && (unsigned)(ix0 - 1 + rx) < (unsigned)a.W;
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(rin, (lds_void *)(in_fill + c * 1024), 16, ok ? basei + reli[k] : 0x80000000u, 0, 0, 0);
                    }
                }
            }
            if (jc < nt) {
                const TilePos q = tile_pos(jc);
                const int iy0 = 2 * q.ty * CS_TH - 1, ix0 = 2 * q.tx * CS_TW - 1;
                // (a group's geometry is a dozen integer operations: formed again in every step, not kept in registers the filters
                //  need across the loop -- the compiler would hoist it and spill, and a reload waits for the requests in flight)
                int l15s = l15, lqs = lq;
                asm volatile("" : "+v"(l15s), "+v"(lqs));
#pragma unroll
                for (int jj = 0; jj < CS_NG; ++jj) {
                    const int g = sub + 4 * jj;
                    if (g < CS_GROUPS) {
                        const int idx = g * 16 + l15s;
                        const int ly = (idx * 3856) >> 16;       // idx / 17 for idx < 160
                        const int lx = idx - ly * CS_LW;
                        // layer-4 window pixel (ly, lx) is layer-2 window pixel (ly + 1, lx + 1); tap (kh, kw) reads (ly + kh, lx + kw)
                        const int p0 = ly * CS_IW + lx;
                        f32x4 acc[4];
#pragma unroll
                        for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < 9; ++t) {
                            const int kh = t / 3, kw = t - kh * 3;
                            const int p = p0 + kh * CS_IW + kw;
                            const bf16x8 x = *(const bf16x8 *)(in_cur + p * 64 + ((lqs ^ (2 * ((p >> 2) & 1))) << 4));
#pragma unroll
                            for (int ct = 0; ct < 4; ++ct) acc[ct] = mma16<H16>(fw[ct][t], x, acc[ct]);
                        }
                        // layer 5 pads LAYER 4: a window pixel outside the image is zero, whatever conv3 makes of its padded input
                        const bool inside = (unsigned)(iy0 + ly) < (unsigned)a.H && (unsigned)(ix0 + lx) < (unsigned)a.W;
                        char *const rec = l4 + (ly * CS_LW + lx) * CS_PITCH + (lqs & 1) * 8;
                        const int swz = (ly >> 1) & 1;
                        if (idx < CS_LPIX) {
#pragma unroll
                            for (int ct = 0; ct < 4; ++ct) {
                                uint2 *const q4 = (uint2 *)(rec + (((ct * 2 + (lqs >> 1)) ^ swz) << 4));
                                const uint2 r = *q4;                             // the shortcut source, fetched into the record
                                const uint2 pk = leaky_pack4<H16>(acc[ct], bv[ct], slope);      // conv3's own output, rounded first
                                uint2 o;
                                o.x = pack16x2<H16>(unpack16_lo<H16>(pk.x) + unpack16_lo<H16>(r.x), unpack16_hi<H16>(pk.x) + unpack16_hi<H16>(r.x));
                                o.y = pack16x2<H16>(unpack16_lo<H16>(pk.y) + unpack16_lo<H16>(r.y), unpack16_hi<H16>(pk.y) + unpack16_hi<H16>(r.y));
                                o.x = inside ? o.x : 0u; o.y = inside ? o.y : 0u;
                                *q4 = o;
                            }
                        }
                    }
                }
            }
        };
        if (nt > 0) produce(0, nt, l4b, inb, inb + CS_IN_BYTES, l4b + CS_L4_BYTES);      // (requests only)
        __builtin_amdgcn_s_waitcnt(waitcnt_imm(0, 0));
        __builtin_amdgcn_s_barrier();
        // step i: requests of tile i + 2, conv3 of tile i + 1; c3 = (i + 1) % 3, par = (i + 1) & 1
        for (int i = -1, c3 = 0, par = 0; i <= nt; ++i, c3 = c3 == 2 ? 0 : c3 + 1, par ^= 1) {
            const int f3 = c3 == 2 ? 0 : c3 + 1;
            produce(i + 2, i + 1, l4b + f3 * CS_L4_BYTES, inb + (par ^ 1) * CS_IN_BYTES, inb + par * CS_IN_BYTES, l4b + c3 * CS_L4_BYTES);
            __builtin_amdgcn_s_waitcnt(waitcnt_imm(0, 0));       // the requested windows have landed, the layer-4 tile is written
            __builtin_amdgcn_s_barrier();
        }
    } else {
        // =========================================== consumers ===========================================
        const int grp = sub;                                     // channel group: 32 output channels
        // this wave's filters: 2 channel tiles x 18 K-slices (tap * 2 + channel half), rows K-contiguous with k = tap * 64 + c
        bf16x8 fw[2][18];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int ks = 0; ks < 18; ++ks)
                fw[ct][ks] = *(const bf16x8 *)((const bf16_t *)a.w5 + (size_t)(grp * 32 + ct * 16 + l15) * a.Kpad5 + ks * 32 + lq * 8);
        f32x4 bv[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) bv[ct] = *(const f32x4 *)(a.b5 + grp * 32 + ct * 16 + lq * 4);
        const float slope = act_slope(a.act5);
        const int ctid = tid - 256;
        // LDS byte offset of this lane's window pixel for tap (0, 0), per sub-tile (two output rows of 8 pixels); the tap adds (kh * 17 + kw) * 144
        int pb[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {
            const int r = 2 * sb + (l15 >> 3), c = l15 & 7;
            pb[sb] = ((2 * r) * CS_LW + 2 * c) * CS_PITCH;
        }
        const int rpar = (l15 >> 3) & 1;                         // parity of this lane's output row within the tile (sub-tiles start on even rows)
        auto consume = [&](int jprev, int jcur, const char *__restrict__ lo_prev, const char *__restrict__ l4, char *__restrict__ lo) {
            if (jprev >= 0) {                                    // whole-line stores of the tile staged in the previous step
                const TilePos q = tile_pos(jprev);
                const int oy0 = q.ty * CS_TH, ox0 = q.tx * CS_TW;
#pragma unroll
                for (int it = 0; it < CS_TH * CS_TW * 16 / 256; ++it) {
                    const int c = ctid + it * 256;
                    const int px = c >> 4, chunk = c & 15;
                    const int oy = oy0 + (px >> 3), ox = ox0 + (px & 7);
                    const uint4 o = *(const uint4 *)(lo_prev + px * CS_OPITCH + chunk * 16);
                    const unsigned so = (oy < Ho && ox < Wo) ? (unsigned)((((size_t)(q.n * Ho + oy) * Wo + ox) * a.out_stride + chunk * 8) * 2) : 0x80000000u;
                    out_store16_at(a.out, so, o.x, o.y, o.z, o.w);
                }
            }
            if (jcur >= 0 && jcur < nt) {
                f32x4 acc[2][2];
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) acc[sb][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int t = 0; t < 9; ++t) {
                    const int kh = t / 3, kw = t - kh * 3;
                    const int swz = rpar ^ (kh >> 1);            // ((window row) >> 1) & 1 of this lane's pixel for this tap
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const int coff = ((hh * 4 + lq) ^ swz) << 4;
#pragma unroll
                        for (int sb = 0; sb < 2; ++sb) {
                            const bf16x8 x = *(const bf16x8 *)(l4 + pb[sb] + (kh * CS_LW + kw) * CS_PITCH + coff);
#pragma unroll
                            for (int ct = 0; ct < 2; ++ct) acc[sb][ct] = mma16<H16>(fw[ct][t * 2 + hh], x, acc[sb][ct]);
                        }
                    }
                }
#pragma unroll
                for (int sb = 0; sb < 2; ++sb)
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct)
                        *(uint2 *)(lo + (sb * 16 + l15) * CS_OPITCH + (grp * 32 + ct * 16 + lq * 4) * 2) = leaky_pack4<H16>(acc[sb][ct], bv[ct], slope);
            }
        };
        __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, 0));
        __builtin_amdgcn_s_barrier();
        // step i: stores of tile i - 1, stride-2 conv of tile i; c3 = (i + 1) % 3, par = (i + 1) & 1
        for (int i = -1, c3 = 0, par = 0; i <= nt; ++i, c3 = c3 == 2 ? 0 : c3 + 1, par ^= 1) {
            const int u3 = c3 == 0 ? 2 : c3 - 1;                 // i % 3
            consume(i >= 1 ? i - 1 : -1, i, lob + par * CS_OUT_BYTES, l4b + u3 * CS_L4_BYTES, lob + (par ^ 1) * CS_OUT_BYTES);
            __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, 0));      // the staged tile is written, the layer-4 tile is read
            __builtin_amdgcn_s_barrier();
        }
    }
#endif
}

bool conv_c3s2_ok(const C3S2Args &a)
{
    // 32-bit buffer offsets below 0x80000000 (the out-of-range sentinel): every window must stay under 2 GiB
    const double pin = (double)a.N * a.H * a.W, pout = (double)a.N * ((a.H - 1) / 2 + 1) * ((a.W - 1) / 2 + 1);
    if (pin * a.in_stride * 2.0 >= 2147483648.0 || pin * a.res_stride * 2.0 >= 2147483648.0 || pout * a.out_stride * 2.0 >= 2147483648.0) return false;
    return (a.dt == DT_BF16 || a.dt == DT_F16) && a.in && a.res && a.out && a.Kpad3 >= 288 && a.Kpad5 >= 576 && a.N >= 1 && a.H >= 2 && a.W >= 2 &&
           (a.in_stride % 8) == 0 && a.in_stride >= 32 && (a.res_stride % 8) == 0 && a.res_stride >= 64 && (a.out_stride % 8) == 0 && a.out_stride >= 128;
}
hipError_t launch_conv_c3s2(const C3S2Args &a, hipStream_t s)
{
    if (!conv_c3s2_ok(a)) return hipErrorInvalidValue;
    const bool h16 = a.dt == DT_F16;
    { hipError_t e = conv_opt_in_lds(h16 ? (const void *)conv_c3s2_c32_c64_c128<true> : (const void *)conv_c3s2_c32_c64_c128<false>, CS_LDS); if (e != hipSuccess) return e; }
    const int Ho = (a.H - 1) / 2 + 1, Wo = (a.W - 1) / 2 + 1;
    const long tiles = (long)a.N * ((Wo + CS_TW - 1) / CS_TW) * ((Ho + CS_TH - 1) / CS_TH);
    long blocks = 256; if (blocks > tiles) blocks = tiles;          // persistent: one workgroup per CU
    if (h16) hipLaunchKernelGGL(conv_c3s2_c32_c64_c128<true>, dim3((unsigned)blocks), dim3(64 * CS_NW), CS_LDS, s, a);
    else hipLaunchKernelGGL(conv_c3s2_c32_c64_c128<false>, dim3((unsigned)blocks), dim3(64 * CS_NW), CS_LDS, s, a);
    return hipGetLastError();
}
