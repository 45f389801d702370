// XNOR convolution ([convolutional] with xnor=1, DN/convolutional_layer.c:28-49, 451-485) on NHWC tensors: see XConvArgs (kernels.h) for the
// semantics, the window, the channel chunks and the K order.
//
// k_xconv: one workgroup of four waves computes a te x te block of output pixels of one image against `fper` tiles of XCONV_CO_TILE filters
// with v_mfma_i32_16x16x64_i8.  The binarisation is part of the staging: the block's input window is read from the producer's tensor as it
// is stored (bf16, fp16 or fp32), eight channels per thread and step, and written to LDS as int8 -- +1 where the value is > 0, -1 elsewhere
// (so +0, -0 and NaN give -1: the test is on the value, not a copy of the sign bit), 0 outside the image and in the channels past C.  Every
// tap of every pixel of the block then reads that one copy.  Where all channels fit one chunk the window is staged once and serves every
// filter tile of the workgroup; a layer of more channels stages chunk by chunk for each filter tile.
// As in gconv.hip the FILTERS are the A operand (rows = output channels) and the pixels the B operand: the accumulator has its pixel on
// the lane (lane & 15) and four consecutive channels in its registers ((lane >> 4) * 4 + j), stored as one 8-byte (16-bit) or 16-byte
// (fp32) piece.  A lane's A and B fragments of one K step are the same granule -- 16 consecutive channels of one tap, lane group lane >> 4
// takes granule 4 * step + (lane >> 4) -- so the sum does not depend on the order of the 16 bytes inside a fragment.  The A fragments come
// straight from global memory in fragment order (one contiguous KiB per wave and load), the B fragments from the window with ds_read_b128;
// a window position is cc + 16 bytes apart from the next, which spreads the sixteen pixels of a fragment load over the banks.
// The epilogue is float(acc) * scale + bias, then the side convs' store (side_epilogue.h).
#include "kernels.h"
#include "device_common.h"
#include "side_epilogue.h"
#include <algorithm>

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// eight stored values -> eight int8 signs, the low byte first; `live` of them are channels of the tensor, the others give 0
template <typename T> __device__ __forceinline__ uint2 sign8(const T *p, int live);
template <bool H16> __device__ __forceinline__ uint2 sign8_bits(const uint16_t *p, int live)
{
    const uint4 u = *(const uint4 *)p;
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const uint32_t b = (w[e >> 1] >> ((e & 1) * 16)) & 0xffffu;
        // > 0: the bits are not zero, the sign is clear and the value is no NaN -- 1 .. the bits of +infinity
        const uint32_t s = (b - 1u) < (H16 ? 0x7c00u : 0x7f80u) ? 0x01u : 0xffu;
        o[e >> 2] |= (e < live ? s : 0u) << ((e & 3) * 8);
    }
    return uint2{o[0], o[1]};
}
template <> __device__ __forceinline__ uint2 sign8<bf16_t>(const bf16_t *p, int live) { return sign8_bits<false>(p, live); }
template <> __device__ __forceinline__ uint2 sign8<f16_t>(const f16_t *p, int live) { return sign8_bits<true>((const uint16_t *)p, live); }
template <> __device__ __forceinline__ uint2 sign8<float>(const float *p, int live)
{
    const float4 x = *(const float4 *)p, y = *(const float4 *)(p + 4);
    const float v[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
    uint32_t o[2] = {0u, 0u};
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e >> 2] |= (e < live ? (v[e] > 0.f ? 0x01u : 0xffu) : 0u) << ((e & 3) * 8);
    return uint2{o[0], o[1]};
}

template <typename T>
__global__ __launch_bounds__(256) void k_xconv(const XConvArgs a, const int fper)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t win[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, lq = lane >> 4;
    const int te = a.te, tsh = te == 8 ? 3 : 2, bx = (a.Wo + te - 1) >> tsh, by = (a.Ho + te - 1) >> tsh;
    const int n = blockIdx.x / (bx * by), brem = blockIdx.x - n * (bx * by), oy0 = (brem / bx) << tsh, ox0 = (brem % bx) << tsh;
    const int iy0 = oy0 * a.stride - a.pad, ix0 = ox0 * a.stride - a.pad;
    const int ww = a.ww, rs = a.rs, pitch = a.cc + 16, taps = a.size * a.size, cp = (a.C + 15) & ~15;
    const int ftiles = a.cout_pad / XCONV_CO_TILE, f0 = blockIdx.y * fper, f1 = min(ftiles, f0 + fper);
    const int KS = a.kpad >> 6, chunk_steps = (taps * a.cc + 63) >> 6;          // K steps of a filter row; of a whole chunk
    const int wp = wave & 1, wf = wave >> 1;          // this wave: pixels wp * 32 .. + 31 of the block, filters wf * 32 .. + 31 of the tile
    // this lane's two pixels (column l15 of the two B operands and of the accumulators): where their taps begin in the window
    int wpos[2]; bool pv[2]; long opix[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = wp * 32 + j * 16 + l15, y = p >> tsh, x = p & (te - 1);
        const bool in_block = p < te * te;          // (a 4 x 4 block has 16 pixels: the other columns compute nothing that is stored)
        pv[j] = in_block && oy0 + y < a.Ho && ox0 + x < a.Wo;
        wpos[j] = in_block ? (y * rs * ww + x * rs) * pitch : 0;
        opix[j] = ((long)n * a.Ho + oy0 + y) * a.Wo + ox0 + x;
    }
    const T *in = (const T *)a.in + (long)n * a.H * a.W * a.in_stride;
    const float slope = act_slope(a.act);
    for (int ft = f0; ft < f1; ++ft) {
        i32x4 acc[2][2];          // [filter tile of 16][pixel tile of 16]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = i32x4{0, 0, 0, 0};
        for (int ch = 0; ch < a.nchunks; ++ch) {
            const int c0 = ch * a.cc, ccj = min(a.cc, cp - c0);
            if (a.nchunks > 1 || ft == f0) {          // (uniform over the workgroup)
                __syncthreads();          // the last reads of what the window held
                const int c8n = ccj >> 3, units = ww * ww * c8n;
                for (int u = tid; u < units; u += 256) {
                    const int pos = u / c8n, c8 = u - pos * c8n, r = pos / ww, q = pos - r * ww;
                    const int iy = iy0 + (r / rs) * a.stride + r % rs, ix = ix0 + (q / rs) * a.stride + q % rs, c = c0 + c8 * 8;
                    uint2 s = uint2{0u, 0u};
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W && c < a.C) s = sign8<T>(in + ((long)iy * a.W + ix) * a.in_stride + c, a.C - c);
                    *(uint2 *)(win + pos * pitch + c8 * 8) = s;
                }
                __syncthreads();
            }
            const int ccg = ccj >> 4, ng = taps * ccg, nsteps = (ng + 3) >> 2;
            const int8_t *wt = (const int8_t *)a.wt + ((((long)(ft * 4 + wf * 2) * KS + ch * chunk_steps) * 64 + lane) << 4);
            // this lane's granule 4 * step + lq as (tap row, tap column, granule of the chunk), advanced by 4 per step without a division
            int gi = lq, ty = 0, tx = 0;
            while (gi >= ccg) { gi -= ccg; if (++tx == a.size) { tx = 0; ++ty; } }
            for (int st = 0; st < nsteps; ++st) {
                const i32x4 w0 = *(const i32x4 *)(wt + ((long)st << 10)), w1 = *(const i32x4 *)(wt + (((long)KS + st) << 10));
                i32x4 b[2] = {i32x4{0, 0, 0, 0}, i32x4{0, 0, 0, 0}};
                if (ty < a.size) {          // (past the chunk's last granule: the K padding, zero filters against zeros)
                    const int off = (ty * ww + tx) * pitch + gi * 16;
                    b[0] = *(const i32x4 *)(win + wpos[0] + off); b[1] = *(const i32x4 *)(win + wpos[1] + off);
                }
                acc[0][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, b[0], acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w0, b[1], acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, b[0], acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w1, b[1], acc[1][1], 0, 0, 0);
                gi += 4;
                while (gi >= ccg) { gi -= ccg; if (++tx == a.size) { tx = 0; ++ty; } }
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int co = ft * XCONV_CO_TILE + wf * 32 + i * 16 + lq * 4;
            if (co >= a.Cstore) continue;          // (co and Cstore are multiples of 4: the four channels are in or out together)
            const float4 sc = *(const float4 *)(a.scale + co), bv = *(const float4 *)(a.bias + co);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (!pv[j]) continue;
                const float v[4] = {(float)acc[i][j][0] * sc.x + bv.x, (float)acc[i][j][1] * sc.y + bv.y, (float)acc[i][j][2] * sc.z + bv.z, (float)acc[i][j][3] * sc.w + bv.w};
                side_store4(a.out, opix[j] * a.out_stride + co, a.out_dt, slope, v);
            }
        }
    }
}

template <typename T> hipError_t launch_t(const XConvArgs &a, const dim3 grid, int fper, size_t lds, hipStream_t s)
{
    if (lds > 64 * 1024) { const hipError_t e = conv_opt_in_lds((const void *)k_xconv<T>, XCONV_LDS_BYTES); if (e != hipSuccess) return e; }
    hipLaunchKernelGGL(k_xconv<T>, grid, dim3(256), lds, s, a, fper);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_xconv(const XConvArgs &a, hipStream_t s)
{
    if (a.C < 1 || a.Cout < 1 || !xconv_served(a.size, a.stride, a.pad, a.H, a.W)) return hipErrorInvalidValue;
    XConvArgs g = a; xconv_layout(g);
    if (g.te != a.te || g.rs != a.rs || g.ww != a.ww || g.cc != a.cc || g.nchunks != a.nchunks || g.kpad != a.kpad || g.cout_pad != a.cout_pad) return hipErrorInvalidValue;
    if (!side_conv_args_ok(a, a.cout_pad) || ((uintptr_t)a.scale & 15) || a.in_stride < (a.C + 7) / 8 * 8 ||
        a.Ho != (a.H + 2 * a.pad - a.size) / a.stride + 1 || a.Wo != (a.W + 2 * a.pad - a.size) / a.stride + 1) return hipErrorInvalidValue;
    if (a.in_dt != DT_BF16 && a.in_dt != DT_F16 && a.in_dt != DT_F32) return hipErrorInvalidValue;
    if (a.out_dt != DT_BF16 && a.out_dt != DT_F16 && a.out_dt != DT_F32) return hipErrorInvalidValue;
    const size_t lds = (size_t)a.ww * a.ww * (a.cc + 16);
    if (lds > XCONV_LDS_BYTES) return hipErrorInvalidValue;
    const long blocks = (long)a.N * ((a.Ho + a.te - 1) / a.te) * ((a.Wo + a.te - 1) / a.te);
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    // filter tiles per workgroup: one staged window serves them all where the channels fit one chunk, so as many as leave the chip about four
    // workgroups per compute unit; a layer of more chunks stages per filter tile anyway and takes one tile per workgroup
    const int ftiles = a.cout_pad / XCONV_CO_TILE;
    int split = a.nchunks > 1 ? ftiles : (int)std::min<long>(ftiles, std::max<long>(1, (1024 + blocks - 1) / blocks));
    const int fper = (ftiles + split - 1) / split;
    split = (ftiles + fper - 1) / fper;
    if (split > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks, (unsigned)split);
    if (a.in_dt == DT_F32) return launch_t<float>(a, grid, fper, lds, s);
    if (a.in_dt == DT_F16) return launch_t<f16_t>(a, grid, fper, lds, s);
    return launch_t<bf16_t>(a, grid, fper, lds, s);
}
