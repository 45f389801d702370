// JPEG files, device stage: the 8 x 8 integer IDCT of every block of a batch, in one launch.  The arithmetic is jpeg_idct_1d of kernels.h, the
// reference's (stb_image.h stbi__idct_block) restated; what is decided here is who holds what.
//   Eight lanes share a block, a wave holds eight blocks, a workgroup four waves.  A lane loads one ROW of coefficients with one 16-byte load (a block is 128
//   contiguous bytes, a wave reads 1 KiB contiguous), the block is transposed through LDS, the lane transforms one COLUMN, the result is transposed back, and the
//   lane transforms one row.  For that last pass the wave is re-dealt: lane L takes row L >> 3 of block L & 7, so lanes 0..7 store the same row of eight
//   neighbouring blocks -- 64 contiguous bytes of the plane where the blocks are neighbours in it --, 8 bytes per lane.
//   LDS layout (dwords), per wave: element (row, col) of block k at 72 k + 4 (k >> 2) + 9 row + col.  ds_read_b32 / ds_write_b32 bank by (dword address) mod 32
//   within each 32-lane half.  Writing rows (half = 4 blocks x 8 rows, col fixed): 8 (k + row) + row + const, distinct.  Reading columns (4 blocks x 8 cols, row
//   fixed): 8 k + col + const, distinct.  The re-dealt read (8 blocks x 4 rows, col fixed): 8 (k + row) + 4 (k >> 2) + row + const, distinct -- the 4 (k >> 2)
//   term separates blocks k and k + 4, which 72 k alone would put on one bank.
#include "kernels.h"

namespace {

constexpr int WAVE_LDS = 8 * 72 + 8;          // dwords of a wave's eight blocks
__device__ __forceinline__ int lds_at(int k, int row, int col) { return 72 * k + 4 * (k >> 2) + 9 * row + col; }

__global__ __launch_bounds__(256) void k_jpeg_idct(const int16_t *__restrict__ coef, const JpegPlane *__restrict__ planes, int nplanes, unsigned blocks,
                                                   uint8_t *__restrict__ out, unsigned out_bytes)
{
    __shared__ int lds[4 * WAVE_LDS];
    const int lane = threadIdx.x & 63, k = lane >> 3, l8 = lane & 7;
    int *t = lds + (threadIdx.x >> 6) * WAVE_LDS;
    const unsigned wave0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 8u;          // the wave's first block
    int s[8], o[8];
    // row l8 of block wave0 + k: 8 coefficients, 16 bytes.  A block past the batch's end is zeros and stores nothing; every lane reaches every barrier
    int4 raw = make_int4(0, 0, 0, 0);
    if (wave0 + (unsigned)k < blocks) raw = *reinterpret_cast<const int4 *>(coef + ((size_t)(wave0 + (unsigned)k) * 64 + (size_t)l8 * 8));
    s[0] = (int)(short)raw.x; s[1] = raw.x >> 16; s[2] = (int)(short)raw.y; s[3] = raw.y >> 16;
    s[4] = (int)(short)raw.z; s[5] = raw.z >> 16; s[6] = (int)(short)raw.w; s[7] = raw.w >> 16;
#pragma unroll
    for (int j = 0; j < 8; ++j) t[lds_at(k, l8, j)] = s[j];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 8; ++r) s[r] = t[lds_at(k, r, l8)];          // column l8
    __syncthreads();
    jpeg_idct_1d(s, JPEG_IDCT_COL_BIAS, JPEG_IDCT_COL_SHIFT, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) t[lds_at(k, r, l8)] = o[r];
    __syncthreads();
    // re-dealt: row `row` of block wave0 + kb
    const int kb = lane & 7, row = lane >> 3;
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = t[lds_at(kb, row, j)];
    jpeg_idct_1d(s, JPEG_IDCT_ROW_BIAS, JPEG_IDCT_ROW_SHIFT, o);
    const unsigned b = wave0 + (unsigned)kb;
    if (b >= blocks) return;
    // the plane block b lies in: the last one that begins at or before it
    int lo = 0, hi = nplanes - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (planes[mid].block0 <= b) lo = mid; else hi = mid - 1;
    }
    const JpegPlane p = planes[lo];
    const unsigned i = b - p.block0, by = i / p.bw, bx = i - by * p.bw;
    const unsigned long long off = (unsigned long long)p.offset + (unsigned long long)(by * 8u + (unsigned)row) * p.pitch + bx * 8u;
    if (off + 8 > out_bytes) return;          // (the host sized the surface for every plane: never taken)
    // The shifted sums are made opaque before they are clamped and packed.  Left to itself the compiler fuses `clamp8(x >> 17) | clamp8(y >> 17) << 8` into
    // v_ashr_pk_u8_i32 and ORs the other two bytes into that register's upper half, which it takes to be zero; on the MI355X the upper half came back holding
    // bits of the instruction's old destination, and bytes 2, 3, 6 and 7 of every row were wrong while bytes 0, 1, 4 and 5 were right (NOTEBOOK "JPEG files").
    // To re-check when the compiler changes: `llvm-objdump -d` of this object must show no v_ashr_pk_u8_i32; the fixtures of tests/test_gpu_jpeg.py pin the bytes
#pragma unroll
    for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(o[j]));
    uint2 px;
    px.x = (unsigned)clamp8(o[0]) | (unsigned)clamp8(o[1]) << 8 | (unsigned)clamp8(o[2]) << 16 | (unsigned)clamp8(o[3]) << 24;
    px.y = (unsigned)clamp8(o[4]) | (unsigned)clamp8(o[5]) << 8 | (unsigned)clamp8(o[6]) << 16 | (unsigned)clamp8(o[7]) << 24;
    *reinterpret_cast<uint2 *>(out + off) = px;
}

}  // namespace

hipError_t launch_jpeg_idct(const int16_t *coef, const JpegPlane *d_planes, int nplanes, size_t blocks, uint8_t *out, size_t out_bytes, hipStream_t s)
{
    if (!coef || !d_planes || !out || nplanes < 1 || blocks < 1 || blocks > 0xffffffffull - 32 || out_bytes > 0xffffffffull || ((uintptr_t)coef & 15) || ((uintptr_t)out & 7)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_jpeg_idct, dim3((unsigned)((blocks + 31) / 32)), dim3(256), 0, s, coef, d_planes, nplanes, (unsigned)blocks, out, (unsigned)out_bytes);
    return hipGetLastError();
}
