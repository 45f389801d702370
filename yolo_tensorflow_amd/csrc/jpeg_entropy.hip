// JPEG files, the entropy stage on the device: Huffman decoding over restart intervals, one LANE per interval.  The decoding itself is
// jpeg_decode_interval of jpeg_entropy.h, the function the host compiles too; what is decided here is who holds what.
//   A workgroup is one wave of 64 lanes and serves 64 consecutive slots of the batch's interval table, all of one file (the host pads every file's intervals to a
//   multiple of 64 with idle slots): the file's six Huffman tables and three quantisation tables and its geometry, 8944 bytes, are staged into LDS once per workgroup, with dword
//   copies that 64 lanes share.  A table look-up is then a 2-byte LDS read at an address the lane's own bits choose: the lanes of a wave sit in 64 different symbol
//   states, so these reads bank-conflict as chance has it (32 banks of 4 bytes; `look` spans 256 dwords) -- inherent to the method, and cheaper than the same
//   reads from global memory by the whole L1 round trip.
//   The stream is read per lane through aligned 32-bit words (JpegIntervalBits): 64 lanes read 64 unrelated cache lines, a line of 128 bytes then serves the lane's
//   next 32 fetches from the cache.  A wider word would save instructions, not lines, and costs registers the divergent loop has better use for.
//   No barrier lies behind the decode: a lane whose interval fails stores its status word and is done.
#include <hip/hip_runtime.h>
#include "jpeg_entropy.h"

using namespace yolo_impl;

namespace {

__global__ __launch_bounds__(JPEG_ENTROPY_LANES) void k_jpeg_entropy(const uint8_t *__restrict__ stream, unsigned long long stream_bytes, const JpegDevFile *__restrict__ files,
                                                                     unsigned nfiles, const uint32_t *__restrict__ wg_file, const JpegInterval *__restrict__ iv, unsigned slots,
                                                                     int16_t *__restrict__ coef, unsigned long long coef_blocks, uint32_t *__restrict__ status)
{
    struct Staged { JpegEntropyTables t; JpegGeom g; };
    __shared__ Staged S;
    static_assert(sizeof(Staged) % 4 == 0 && offsetof(JpegDevFile, t) == 0 && offsetof(JpegDevFile, g) == offsetof(Staged, g), "tables and geometry are copied as dwords from the head of the record");
    const unsigned slot = blockIdx.x * JPEG_ENTROPY_LANES + threadIdx.x;
    const unsigned fi = wg_file[blockIdx.x];
    // (wave-uniform: the whole workgroup leaves, before the barrier.)  A record the host did not make: every lane reports it
    if (fi >= nfiles) { if (slot < slots) status[slot] = JPEG_IV_STORE; return; }
    const JpegDevFile &F = files[fi];
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&F);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&S);
        for (unsigned i = threadIdx.x; i < sizeof(Staged) / 4; i += JPEG_ENTROPY_LANES) dst[i] = src[i];
    }
    __syncthreads();
    if (slot >= slots) return;
    const JpegInterval v = iv[slot];
    unsigned st = JPEG_IV_OK;
    if (v.mcus) {
        // the file's bytes lie inside the stream buffer, the interval inside the file, the file's blocks inside the array (the host laid them out so: never taken)
        if (F.stream0 > stream_bytes || F.bytes > stream_bytes - F.stream0 || v.end > F.bytes || v.begin > v.end || F.block0 > coef_blocks || F.blocks > coef_blocks - F.block0) st = JPEG_IV_STORE;
        else st = jpeg_decode_interval(stream + F.stream0, v.begin, v.end, S.t, v.first_mcu, v.mcus, S.g, coef + F.block0 * 64, F.blocks);
    }
    status[slot] = st;
}

}  // namespace

hipError_t launch_jpeg_entropy(const uint8_t *d_stream, size_t stream_bytes, const JpegDevFile *d_files, int nfiles, const uint32_t *d_wg_file, const JpegInterval *d_iv, size_t slots,
                               int16_t *coef, size_t coef_blocks, uint32_t *d_status, hipStream_t s)
{
    if (!d_stream || !d_files || !d_wg_file || !d_iv || !coef || !d_status || nfiles < 1 || slots < JPEG_ENTROPY_LANES || slots % JPEG_ENTROPY_LANES || slots > 0x7fffffc0ull ||
        stream_bytes < 1 || coef_blocks < 1 || ((uintptr_t)d_stream & 15) || ((uintptr_t)d_files & 7) || ((uintptr_t)d_wg_file & 3) || ((uintptr_t)d_iv & 15) || ((uintptr_t)coef & 15) ||
        ((uintptr_t)d_status & 3))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(slots / JPEG_ENTROPY_LANES)), block(JPEG_ENTROPY_LANES);
    hipLaunchKernelGGL(k_jpeg_entropy, grid, block, 0, s, d_stream, (unsigned long long)stream_bytes, d_files, (unsigned)nfiles, d_wg_file, d_iv, (unsigned)slots, coef, (unsigned long long)coef_blocks, d_status);
    return hipGetLastError();
}
