// JPEG files, the entropy stage over restart intervals: ONE decoder of one restart interval, compiled for the host (yolo_jpeg.cpp, the sanitizer
// run of tests/c/jpeg_intervals.cpp) and for the device (k_jpeg_entropy, jpeg_entropy.hip).  A restart interval is byte-aligned, begins with zeroed DC predictors
// and ends at a marker: the intervals of a file are independent streams.  jpeg_decode_interval restates what jpeg_decode (yolo_jpeg.cpp) does for the interval's
// MCUs -- the same symbol decode, EXTEND, unsigned DC prediction, 16-bit wrap of the dequantising multiply, zig-zag and the same four failures -- and adds one
// verdict of its own, "doubtful".  Plain C++: no HIP header is needed to read this file.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__          // (inlined into the kernel: the tables are then known to lie in LDS, the stream in global memory)
#else
#define JPEG_HD inline
#endif

namespace yolo_impl {

// what an interval came to.  0: every MCU decoded and fewer than one whole unread byte lies before its end.  DOUBTFUL: every MCU decoded, whole bytes are left over
// (a well-formed encoder pads the last byte and puts the marker directly behind it; whether the host reader accepts such an interval depends on how far its
// read-ahead got).  A file with any non-zero interval is decoded again, in full, by jpeg_decode, whose verdict stands
enum { JPEG_IV_OK = 0, JPEG_IV_BAD_DC = 1, JPEG_IV_BAD_AC = 2, JPEG_IV_RUN = 3, JPEG_IV_OVERRUN = 4, JPEG_IV_DOUBTFUL = 5, JPEG_IV_STORE = 6 };

// one restart interval of a file: bytes [begin, end) of it hold MCUs first_mcu .. first_mcu + mcus - 1.  mcus == 0: an idle lane of the device's table
struct JpegInterval { uint32_t begin, end, first_mcu, mcus; };

// a Huffman table as the decoder reads it (JpegHuff of yolo_jpeg.h without its flag), 1420 bytes
struct JpegHuffTable {
    uint16_t look[512];        // (length << 8) | symbol of every code of at most 9 bits, 0: longer
    int32_t maxcode[18];       // largest code of each length, left-aligned to 16 bits, + 1; [17] ends every search
    int32_t delta[17];         // index of the first value of a length minus its first code
    uint8_t vals[256];
};
// the tables of a file by COMPONENT (a table two components share is stated twice: the decoder indexes by component alone), and its geometry
struct JpegEntropyTables {
    JpegHuffTable dc[3], ac[3];
    uint16_t quant[3][64];     // natural order
};
struct JpegGeom {
    int32_t comps, hs, vs, mcux;          // components, the luma sampling, MCUs across
    uint32_t bw[3], block0[3];            // blocks across every component plane, and the plane's first block in the file's coefficient array
};

// the entropy-coded bytes [pos, end) of a file as a bit stream: Bits of yolo_jpeg.cpp, bounded by `end` where that one is bounded by the file.  0xFF00 is a stuffed
// 0xFF; any other 0xFF, or `end`, is where the stream stops: past it the reader yields zero bits and counts them.  Bytes are fetched through whole aligned
// 32-bit words where such a word lies inside [begin, end) -- on the device the 64 lanes of a wave read 64 unrelated addresses, and a word fetched once serves four
// steps of the loop -- and one by one at the interval's two ragged ends; no byte outside [begin, end) is ever read
struct JpegIntervalBits {
    const uint8_t *p; uint32_t begin, end, pos;
    uint64_t buf = 0; int cnt = 0, pad = 0; bool stop = false;
    uint32_t word = 0, word_at = 0xffffffffu;          // the cached word and the offset of its first byte
    JPEG_HD JpegIntervalBits(const uint8_t *p_, uint32_t begin_, uint32_t end_) : p(p_), begin(begin_), end(end_), pos(begin_) {}
    JPEG_HD unsigned byte_at(uint32_t at)          // begin <= at < end
    {
        const uint32_t mis = (uint32_t)((uintptr_t)(p + at) & 3u);
        if (at - begin < mis || end - at < 4u - mis) return p[at];          // the aligned word around `at` begins before `begin` or ends past `end`
        const uint32_t base = at - mis;
        if (base != word_at) { __builtin_memcpy(&word, __builtin_assume_aligned(p + base, 4), 4); word_at = base; }          // (one aligned 32-bit load on either side)
        return (word >> (8u * mis)) & 255u;
    }
    JPEG_HD void fill()
    {
        while (cnt <= 56) {
            unsigned b = 0;
            if (!stop && pos < end) {
                b = byte_at(pos);
                if (b != 0xff) ++pos;
                else if (pos + 1 < end && byte_at(pos + 1) == 0) pos += 2;
                else { stop = true; b = 0; }
            } else stop = true;
            if (stop) pad += 8;
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    JPEG_HD unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }          // 1 <= k <= 32
    JPEG_HD void skip(int k) { buf <<= k; cnt -= k; }
    JPEG_HD bool overrun() const { return cnt < pad; }
    // whole bytes of the interval nobody consumed a bit of: those not yet fetched, and those in the buffer
    JPEG_HD bool bytes_left() const { return pos < end || cnt - pad >= 8; }
};

// T.81 F.2.2.3 DECODE: the next symbol of table t, or -1 where no code matches (huff_symbol of yolo_jpeg.cpp)
JPEG_HD int jpeg_interval_symbol(JpegIntervalBits &b, const JpegHuffTable &t)
{
    b.fill();
    const unsigned e = t.look[b.peek(9)];
    if (e) { b.skip((int)(e >> 8)); return (int)(e & 255u); }
    const int c16 = (int)b.peek(16);
    int len = 10;
    while (len < 17 && c16 >= t.maxcode[len]) ++len;          // (maxcode[17] ends the search on the host's tables; the bound holds for any table)
    if (len > 16) return -1;
    const int idx = (c16 >> (16 - len)) + t.delta[len];
    if (idx < 0 || idx > 255) return -1;
    b.skip(len);
    return t.vals[idx];
}
// T.81 F.2.2.1 EXTEND of the next s bits (1 <= s <= 16); the caller has filled
JPEG_HD int jpeg_interval_extend(JpegIntervalBits &b, int s)
{
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// MCUs first_mcu .. first_mcu + mcus - 1 of a file from bytes [begin, end) of it, into coef[blocks][64] (16-byte aligned; dequantised, natural order: the layout of jpeg_decode).
// Every block is zeroed here before its coefficients are stored: the blocks come out fully written.
// Returns a JPEG_IV_* word; after a failure nothing more is decoded.  Every read of the stream is bounded by `end`, every store by `blocks`, and every loop by
// the geometry (mcus x blocks of an MCU x 63 AC steps, each of which advances k): no input makes it spin
JPEG_HD unsigned jpeg_decode_interval(const uint8_t *file, uint32_t begin, uint32_t end, const JpegEntropyTables &T, uint32_t first_mcu, uint32_t mcus, const JpegGeom &g,
                                      int16_t *coef, size_t blocks)
{
    // T.81 figure A.6: zigzag index -> natural index
    const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    if (g.mcux < 1 || g.comps < 1 || g.comps > 3 || begin > end) return JPEG_IV_STORE;          // (no geometry the host makes)
    coef = (int16_t *)__builtin_assume_aligned(coef, 16);          // (what lets the clearing of a block be eight 16-byte stores)
    JpegIntervalBits b(file, begin, end);
    unsigned pred0 = 0, pred1 = 0, pred2 = 0;          // (three names, not an array the component indexes: they stay in registers on the device)
    uint32_t my = first_mcu / (uint32_t)g.mcux, mx = first_mcu - my * (uint32_t)g.mcux;
    for (uint32_t m = 0; m < mcus; ++m) {
        for (int c = 0; c < g.comps; ++c) {
            const uint32_t nh = c ? 1u : (uint32_t)g.hs, nv = c ? 1u : (uint32_t)g.vs;
            const JpegHuffTable &hd = T.dc[c], &ha = T.ac[c];
            const uint16_t *q = T.quant[c];
            unsigned pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
            for (uint32_t v = 0; v < nv; ++v)
                for (uint32_t u = 0; u < nh; ++u) {
                    const size_t at = (size_t)g.block0[c] + (size_t)(my * nv + v) * g.bw[c] + (size_t)(mx * nh + u);
                    if (at >= blocks) return JPEG_IV_STORE;          // (the host laid the array out for every MCU: never taken)
                    int16_t *d = coef + at * 64;
                    for (int i = 0; i < 64; ++i) d[i] = 0;
                    const int t = jpeg_interval_symbol(b, hd);
                    if (t < 0 || t > 15) return JPEG_IV_BAD_DC;
                    // the prediction wraps like the reference's int would not: unsigned, so that a malformed stream overflows nothing
                    if (t) pred += (unsigned)jpeg_interval_extend(b, t);
                    d[0] = (int16_t)(uint16_t)(pred * q[0]);          // stb_image.h:1969: (short)(dc * dequant[0])
                    for (int k = 1, step = 0; k < 64 && step < 63; ++step) {
                        const int rs = jpeg_interval_symbol(b, ha);
                        if (rs < 0) return JPEG_IV_BAD_AC;
                        const int r = rs >> 4, s = rs & 15;
                        if (s == 0) {
                            if (rs != 0xf0) break;          // end of block
                            k += 16;
                            continue;
                        }
                        k += r;
                        if (k > 63) return JPEG_IV_RUN;
                        const int z = ZIGZAG[k++];
                        d[z] = (int16_t)(uint16_t)((unsigned)jpeg_interval_extend(b, s) * q[z]);          // stb_image.h:1999: (short)(value * dequant[zig])
                    }
                    if (b.overrun()) return JPEG_IV_OVERRUN;
                }
            if (c == 0) pred0 = pred; else if (c == 1) pred1 = pred; else pred2 = pred;
        }
        if (++mx == (uint32_t)g.mcux) { mx = 0; ++my; }
    }
    return b.bytes_left() ? JPEG_IV_DOUBTFUL : JPEG_IV_OK;
}

// ---- the device stage (jpeg_entropy.hip) ----
// one file of a batch as k_jpeg_entropy reads it: its tables and geometry, where its bytes begin in the batch's stream buffer (a multiple of 16) and how many they
// are, where its blocks begin in the batch's coefficient array and how many they are
struct JpegDevFile { JpegEntropyTables t; JpegGeom g; unsigned long long stream0, block0; uint32_t bytes, blocks; };
enum { JPEG_ENTROPY_LANES = 64 };

}  // namespace yolo_impl

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// One lane per restart interval over a whole batch: slot i of d_iv (slots: a multiple of JPEG_ENTROPY_LANES) is an interval of file d_wg_file[i / JPEG_ENTROPY_LANES]
// (offsets inside that file) or, mcus == 0, an idle lane -- a workgroup's lanes belong to one file, whose tables it stages into LDS once.  Every lane stores its
// JPEG_IV_* word into d_status[i] (idle lanes 0).  Every lane zeroes each block before it fills it.  coef: the array launch_jpeg_idct reads (16-byte aligned),
// coef_blocks its size
hipError_t launch_jpeg_entropy(const uint8_t *d_stream, size_t stream_bytes, const yolo_impl::JpegDevFile *d_files, int nfiles, const uint32_t *d_wg_file,
                               const yolo_impl::JpegInterval *d_iv, size_t slots, int16_t *coef, size_t coef_blocks, uint32_t *d_status, hipStream_t s);
#endif
