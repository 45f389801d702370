// JPEG files, host stage (yolo_jpeg.h).  Written from ITU-T T.81: marker segments (annex B), Huffman tables (annex C), the
// sequential decoding procedures (annex F.2).  What must match the reference bit for bit is one line, the dequantising multiply truncated
// to 16 bits (stb_image.h:1969, 1986, 1999); it is restated where it happens.
#include "yolo_jpeg.h"
#include "../../include/yolo_hip.h"
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

namespace yolo_impl {
namespace {

// T.81 figure A.6: zigzag index -> natural index
const uint8_t ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                            35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Fail {
    int index; std::string &msg;
    int operator()(int code, const char *fmt, ...) const __attribute__((format(printf, 3, 4)))
    {
        char b[256];
        va_list ap; va_start(ap, fmt); vsnprintf(b, sizeof b, fmt, ap); va_end(ap);
        msg = "file " + std::to_string(index) + ": " + b;
        return code;
    }
};

// T.81 C.2: code lengths -> canonical codes.  false: the lengths do not form a prefix code
bool build_huffman(JpegHuff &t, const uint8_t *counts, const uint8_t *vals, int n)
{
    memset(t.look, 0, sizeof t.look);
    memcpy(t.vals, vals, (size_t)n);
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        t.delta[len] = k - code;
        for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code)
            if (len <= 9) for (int fill = 0; fill < (1 << (9 - len)); ++fill) t.look[(code << (9 - len)) | fill] = (uint16_t)((len << 8) | vals[k]);
        if (code > (1 << len)) return false;
        t.maxcode[len] = code << (16 - len);
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    t.set = true;
    return true;
}

// the entropy-coded segment as a bit stream (T.81 F.2.2.5): 0xFF00 is a stuffed 0xFF, any other 0xFF xx a marker, where the stream ends.  Past
// its end the stream yields zero bits and counts them: a decoder that consumed one of them read past the data
struct Bits {
    const uint8_t *p; size_t n, pos;
    uint64_t buf = 0; int cnt = 0, pad = 0; bool stop = false;
    Bits(const uint8_t *p_, size_t n_, size_t pos_) : p(p_), n(n_), pos(pos_) {}
    void fill()
    {
        while (cnt <= 56) {
            unsigned b = 0;
            if (!stop && pos < n) {
                b = p[pos];
                if (b != 0xff) ++pos;
                else if (pos + 1 < n && p[pos + 1] == 0) pos += 2;
                else { stop = true; b = 0; }
            } else stop = true;
            if (stop) pad += 8;
            buf |= (uint64_t)b << (56 - cnt);
            cnt += 8;
        }
    }
    unsigned peek(int k) const { return (unsigned)(buf >> (64 - k)); }          // 1 <= k <= 32
    void skip(int k) { buf <<= k; cnt -= k; }
    bool overrun() const { return cnt < pad; }
    // T.81 E.2.4: the rest of the interval is dropped, the next bytes are the RSTm marker (fill bytes 0xFF may precede it)
    bool restart()
    {
        buf = 0; cnt = 0; pad = 0; stop = false;
        while (pos + 1 < n && p[pos] == 0xff && p[pos + 1] == 0xff) ++pos;
        if (pos + 1 >= n || p[pos] != 0xff || p[pos + 1] < 0xd0 || p[pos + 1] > 0xd7) return false;
        pos += 2;
        return true;
    }
};

// T.81 F.2.2.3 DECODE: the next symbol of table t, or -1 where no code matches
inline int huff_symbol(Bits &b, const JpegHuff &t)
{
    b.fill();
    const unsigned e = t.look[b.peek(9)];
    if (e) { b.skip((int)(e >> 8)); return (int)(e & 255u); }
    const int c16 = (int)b.peek(16);
    int len = 10;
    while (c16 >= t.maxcode[len]) ++len;
    if (len > 16) return -1;
    const int idx = (c16 >> (16 - len)) + t.delta[len];
    if (idx < 0 || idx > 255) return -1;
    b.skip(len);
    return t.vals[idx];
}
// T.81 F.2.2.1 EXTEND of the next s bits (1 <= s <= 16); the caller has filled
inline int receive_extend(Bits &b, int s)
{
    const int v = (int)b.peek(s);
    b.skip(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

}  // namespace

int jpeg_parse(const uint8_t *p, size_t n, int index, JpegFile *out, std::string &msg)
{
    const Fail fail{index, msg};
    if (!p || !out) return fail(YOLO_ERR_INVALID, "file == NULL");
    JpegFile &f = *out;
    f = JpegFile();
    if (n < 4 || p[0] != 0xff || p[1] != 0xd8) return fail(YOLO_ERR_INVALID, "no SOI marker at offset 0: not a JPEG file");
    size_t pos = 2;
    bool jfif = false, have_sof = false;
    int adobe = -1, cid[3] = {0, 0, 0}, ch[3] = {1, 1, 1}, cv[3] = {1, 1, 1};
    for (;;) {
        if (pos + 2 > n) return fail(YOLO_ERR_INVALID, "truncated: the file ends at offset %zu before a scan", n);
        if (p[pos] != 0xff) return fail(YOLO_ERR_INVALID, "expected a marker at offset %zu, found 0x%02x", pos, p[pos]);
        while (pos + 1 < n && p[pos + 1] == 0xff) ++pos;          // fill bytes (T.81 B.1.1.2)
        if (pos + 2 > n) return fail(YOLO_ERR_INVALID, "truncated: the file ends at offset %zu inside a marker", n);
        const unsigned m = p[pos + 1];
        const size_t at = pos;
        pos += 2;
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd7)) continue;          // stand-alone markers
        if (m == 0xd8) return fail(YOLO_ERR_INVALID, "a second SOI marker at offset %zu", at);
        if (m == 0xd9) return fail(YOLO_ERR_INVALID, "EOI at offset %zu before any scan", at);
        if (m == 0x00) return fail(YOLO_ERR_INVALID, "marker 0xFF00 at offset %zu outside a scan", at);
        if (pos + 2 > n) return fail(YOLO_ERR_INVALID, "truncated: the file ends at offset %zu inside a segment header", n);
        const size_t L = ((size_t)p[pos] << 8) | p[pos + 1];
        if (L < 2) return fail(YOLO_ERR_INVALID, "segment 0x%02x at offset %zu states the length %zu", m, at, L);
        if (pos + L > n) return fail(YOLO_ERR_INVALID, "truncated: segment 0x%02x at offset %zu ends past the file's %zu bytes", m, at, n);
        const uint8_t *s = p + pos + 2;
        const size_t sl = L - 2;
        pos += L;
        if (m == 0xc2) return fail(YOLO_ERR_UNSUPPORTED, "progressive JPEG (SOF2) is not served");
        if (m == 0xc3 || m == 0xc7 || m == 0xcb || m == 0xcf) return fail(YOLO_ERR_UNSUPPORTED, "lossless JPEG (SOF%u) is not served", m - 0xc0);
        if (m == 0xc9 || m == 0xca || m == 0xcd || m == 0xce) return fail(YOLO_ERR_UNSUPPORTED, "arithmetic-coded JPEG (SOF%u) is not served", m - 0xc0);
        if (m == 0xc5 || m == 0xc6) return fail(YOLO_ERR_UNSUPPORTED, "hierarchical JPEG (SOF%u) is not served", m - 0xc0);
        if (m == 0xcc) return fail(YOLO_ERR_UNSUPPORTED, "arithmetic-coded JPEG (DAC) is not served");
        if (m == 0xc8 || m == 0xdc || m == 0xde || m == 0xdf) return fail(YOLO_ERR_UNSUPPORTED, "marker 0x%02x (DNL / hierarchical) is not served", m);
        if (m == 0xc0 || m == 0xc1) {
            if (have_sof) return fail(YOLO_ERR_INVALID, "a second frame header at offset %zu", at);
            if (sl < 6) return fail(YOLO_ERR_INVALID, "frame header at offset %zu is %zu bytes", at, L);
            if (s[0] == 12) return fail(YOLO_ERR_UNSUPPORTED, "12-bit JPEG is not served");
            if (s[0] != 8) return fail(YOLO_ERR_INVALID, "frame header at offset %zu: sample precision %u", at, s[0]);
            f.h = (s[1] << 8) | s[2]; f.w = (s[3] << 8) | s[4]; f.comps = s[5];
            if (f.h == 0) return fail(YOLO_ERR_UNSUPPORTED, "a frame whose height comes from a DNL segment is not served");
            if (f.w == 0) return fail(YOLO_ERR_INVALID, "frame header at offset %zu: width 0", at);
            if (f.comps == 4) return fail(YOLO_ERR_UNSUPPORTED, "4-component JPEG (CMYK / YCCK) is not served");
            if (f.comps != 1 && f.comps != 3) return fail(YOLO_ERR_INVALID, "frame header at offset %zu: %d components", at, f.comps);
            if (sl != 6 + 3 * (size_t)f.comps) return fail(YOLO_ERR_INVALID, "frame header at offset %zu: length %zu for %d components", at, L, f.comps);
            for (int c = 0; c < f.comps; ++c) {
                cid[c] = s[6 + 3 * c]; ch[c] = s[7 + 3 * c] >> 4; cv[c] = s[7 + 3 * c] & 15; f.tq[c] = s[8 + 3 * c];
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) return fail(YOLO_ERR_INVALID, "frame header at offset %zu: component %d sampled %d x %d", at, c, ch[c], cv[c]);
                if (f.tq[c] > 3) return fail(YOLO_ERR_INVALID, "frame header at offset %zu: component %d names quantisation table %d", at, c, f.tq[c]);
            }
            have_sof = true;
        } else if (m == 0xdb) {
            for (size_t o = 0; o < sl;) {
                const int pq = s[o] >> 4, t = s[o] & 15;
                if (pq > 1 || t > 3) return fail(YOLO_ERR_INVALID, "DQT at offset %zu: precision %d, table %d", at, pq, t);
                const size_t need = pq ? 129 : 65;
                if (o + need > sl) return fail(YOLO_ERR_INVALID, "DQT at offset %zu: table %d passes the segment's end", at, t);
                for (int i = 0; i < 64; ++i) f.quant[t][ZIGZAG[i]] = pq ? (uint16_t)((s[o + 1 + 2 * i] << 8) | s[o + 2 + 2 * i]) : s[o + 1 + i];
                f.qset[t] = true;
                o += need;
            }
        } else if (m == 0xc4) {
            for (size_t o = 0; o < sl;) {
                const int tc = s[o] >> 4, th = s[o] & 15;
                if (tc > 1 || th > 3) return fail(YOLO_ERR_INVALID, "DHT at offset %zu: class %d, table %d", at, tc, th);
                if (o + 17 > sl) return fail(YOLO_ERR_INVALID, "DHT at offset %zu: table %d passes the segment's end", at, th);
                int cnt = 0;
                for (int i = 0; i < 16; ++i) cnt += s[o + 1 + i];
                if (cnt > 256 || o + 17 + (size_t)cnt > sl) return fail(YOLO_ERR_INVALID, "DHT at offset %zu: table %d lists %d codes", at, th, cnt);
                if (!build_huffman(tc ? f.ac[th] : f.dc[th], s + o + 1, s + o + 17, cnt)) return fail(YOLO_ERR_INVALID, "DHT at offset %zu: the code lengths of table %d form no prefix code", at, th);
                o += 17 + (size_t)cnt;
            }
        } else if (m == 0xdd) {
            if (sl != 2) return fail(YOLO_ERR_INVALID, "DRI at offset %zu: length %zu", at, L);
            f.restart = (s[0] << 8) | s[1];
        } else if (m == 0xe0) {
            if (sl >= 5 && !memcmp(s, "JFIF", 5)) jfif = true;
        } else if (m == 0xee) {
            if (sl >= 12 && !memcmp(s, "Adobe", 5)) adobe = s[11];
        } else if (m == 0xda) {
            if (!have_sof) return fail(YOLO_ERR_INVALID, "scan header at offset %zu before a frame header", at);
            if (sl < 1) return fail(YOLO_ERR_INVALID, "scan header at offset %zu is %zu bytes", at, L);
            const int ns = s[0];
            if (ns < 1 || ns > 4 || sl != 4 + 2 * (size_t)ns) return fail(YOLO_ERR_INVALID, "scan header at offset %zu: %d components in %zu bytes", at, ns, L);
            if (ns != f.comps) return fail(YOLO_ERR_UNSUPPORTED, "a multi-scan sequential JPEG (a scan of %d of the %d components) is not served", ns, f.comps);
            for (int c = 0; c < ns; ++c) {
                if (s[1 + 2 * c] != cid[c]) return fail(YOLO_ERR_INVALID, "scan header at offset %zu: component %d is not the frame's", at, s[1 + 2 * c]);
                f.td[c] = s[2 + 2 * c] >> 4; f.ta[c] = s[2 + 2 * c] & 15;
                if (f.td[c] > 3 || f.ta[c] > 3) return fail(YOLO_ERR_INVALID, "scan header at offset %zu: Huffman tables %d / %d", at, f.td[c], f.ta[c]);
                if (!f.dc[f.td[c]].set || !f.ac[f.ta[c]].set) return fail(YOLO_ERR_INVALID, "scan header at offset %zu: Huffman table %d / %d was never defined", at, f.td[c], f.ta[c]);
                if (!f.qset[f.tq[c]]) return fail(YOLO_ERR_INVALID, "scan header at offset %zu: quantisation table %d was never defined", at, f.tq[c]);
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0) return fail(YOLO_ERR_INVALID, "scan header at offset %zu: spectral selection %u..%u, approximation 0x%02x in a sequential file", at, s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns]);
            f.scan = pos;
            break;
        }
        // APPn, COM and everything else with a length: skipped
    }
    if (f.comps == 3) {
        // what the reference would read as RGB, not YCbCr (stb_image.h:3587: component ids 'R','G','B', or Adobe transform 0 without JFIF)
        if (cid[0] == 'R' && cid[1] == 'G' && cid[2] == 'B') return fail(YOLO_ERR_UNSUPPORTED, "a 3-component JPEG stored as RGB (component ids R, G, B) is not served");
        if (adobe == 0 && !jfif) return fail(YOLO_ERR_UNSUPPORTED, "a 3-component JPEG stored as RGB (Adobe APP14 transform 0, no JFIF) is not served");
        if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1 || !(ch[0] <= 2 && cv[0] <= 2))
            return fail(YOLO_ERR_UNSUPPORTED, "chroma subsampling %dx%d,%dx%d,%dx%d is not served (4:4:4, 4:2:2, 4:2:0 and 4:4:0 are)", ch[0], cv[0], ch[1], cv[1], ch[2], cv[2]);
        f.hs = ch[0]; f.vs = cv[0];
        f.format = f.hs == 1 ? (f.vs == 1 ? YOLO_PIX_JPEG_444 : YOLO_PIX_JPEG_440) : f.vs == 1 ? YOLO_PIX_JPEG_422 : YOLO_PIX_JPEG_420;
    } else {
        f.hs = f.vs = 1;          // one component in its scan: 8 x 8 data units in raster order, whatever its sampling factors say (T.81 A.2.2)
        f.format = YOLO_PIX_JPEG_GREY;
    }
    f.mcux = (f.w + 8 * f.hs - 1) / (8 * f.hs); f.mcuy = (f.h + 8 * f.vs - 1) / (8 * f.vs);
    for (int c = 0; c < f.comps; ++c) {
        f.bw[c] = f.mcux * (c ? 1 : f.hs); f.bh[c] = f.mcuy * (c ? 1 : f.vs);
        f.block0[c] = f.blocks;
        f.blocks += (size_t)f.bw[c] * f.bh[c];
    }
    // a block costs two bits at the least (one DC code, one end-of-block): fewer bytes than that cannot hold the frame
    if (f.blocks > 4 * (n - f.scan)) return fail(YOLO_ERR_INVALID, "truncated: %zu bytes follow the scan header at offset %zu, too few for the %zu blocks of a %d x %d frame", n - f.scan, f.scan, f.blocks, f.h, f.w);
    return YOLO_OK;
}

int jpeg_decode(const uint8_t *p, size_t n, int index, const JpegFile &f, int16_t *coef, std::string &msg)
{
    const Fail fail{index, msg};
    if (!p || !coef || f.scan > n) return fail(YOLO_ERR_INVALID, "file / coefficients == NULL");
    Bits b(p, n, f.scan);
    int pred[3] = {0, 0, 0};
    const size_t mcus = (size_t)f.mcux * f.mcuy;
    size_t m = 0;
    for (int my = 0; my < f.mcuy; ++my)
        for (int mx = 0; mx < f.mcux; ++mx, ++m) {
            if (f.restart && m && m % (size_t)f.restart == 0) {
                if (!b.restart()) return fail(YOLO_ERR_INVALID, "no restart marker at offset %zu, after %zu of %zu MCUs", b.pos, m, mcus);
                pred[0] = pred[1] = pred[2] = 0;
            }
            for (int c = 0; c < f.comps; ++c) {
                const int nh = c ? 1 : f.hs, nv = c ? 1 : f.vs;
                const JpegHuff &hd = f.dc[f.td[c]], &ha = f.ac[f.ta[c]];
                const uint16_t *q = f.quant[f.tq[c]];
                for (int v = 0; v < nv; ++v)
                    for (int u = 0; u < nh; ++u) {
                        int16_t *d = coef + (f.block0[c] + (size_t)(my * nv + v) * f.bw[c] + (size_t)(mx * nh + u)) * 64;
                        memset(d, 0, 64 * sizeof(int16_t));
                        const int t = huff_symbol(b, hd);
                        if (t < 0 || t > 15) return fail(YOLO_ERR_INVALID, "bad DC code near offset %zu (MCU %zu of %zu)", b.pos, m, mcus);
                        // the prediction wraps like the reference's int would not: unsigned, so that a malformed stream overflows nothing
                        if (t) pred[c] = (int)((unsigned)pred[c] + (unsigned)receive_extend(b, t));
                        d[0] = (int16_t)(uint16_t)((unsigned)pred[c] * q[0]);          // stb_image.h:1969: (short)(dc * dequant[0])
                        for (int k = 1; k < 64;) {
                            const int rs = huff_symbol(b, ha);
                            if (rs < 0) return fail(YOLO_ERR_INVALID, "bad AC code near offset %zu (MCU %zu of %zu)", b.pos, m, mcus);
                            const int r = rs >> 4, s = rs & 15;
                            if (s == 0) {
                                if (rs != 0xf0) break;          // end of block
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) return fail(YOLO_ERR_INVALID, "a run passes the block's end near offset %zu (MCU %zu of %zu)", b.pos, m, mcus);
                            const int z = ZIGZAG[k++];
                            d[z] = (int16_t)(uint16_t)((unsigned)receive_extend(b, s) * q[z]);          // stb_image.h:1999: (short)(value * dequant[zig])
                        }
                        if (b.overrun()) return fail(YOLO_ERR_INVALID, "truncated: the entropy-coded data ends at offset %zu, in MCU %zu of %zu", b.pos, m, mcus);
                    }
            }
        }
    return YOLO_OK;
}

int jpeg_decode_some(const uint8_t *const *files, const size_t *bytes, const int *which, int count, const JpegFile *parsed, const size_t *first_block, int16_t *coef, std::string &msg)
{
    const auto file_of = [&](int k) { return which ? which[k] : k; };
    if (count == 1) { const int i = file_of(0); return jpeg_decode(files[i], bytes[i], i, parsed[i], coef + first_block[i] * 64, msg); }
    std::atomic<int> next{0};
    std::mutex mu;
    int bad = 0x7fffffff, bad_rc = YOLO_OK;
    auto work = [&]() {
        for (int k; (k = next.fetch_add(1)) < count;) {
            const int i = file_of(k);
            std::string m;
            const int r = jpeg_decode(files[i], bytes[i], i, parsed[i], coef + first_block[i] * 64, m);
            if (r) { std::lock_guard<std::mutex> lock(mu); if (i < bad) { bad = i; bad_rc = r; msg = m; } }
        }
    };
    std::vector<std::thread> pool;
    // a thread the system will not start (or a table it will not allocate) is done without: the threads that did start and the caller share the files
    try { for (int t = 1; t < (count < 8 ? count : 8); ++t) pool.emplace_back(work); } catch (const std::system_error &) {} catch (const std::bad_alloc &) {}
    work();
    for (auto &t : pool) t.join();
    return bad_rc;
}

int jpeg_decode_batch(const uint8_t *const *files, const size_t *bytes, int n, const JpegFile *parsed, const size_t *first_block, int16_t *coef, std::string &msg)
{
    return jpeg_decode_some(files, bytes, nullptr, n, parsed, first_block, coef, msg);
}

bool jpeg_intervals(const uint8_t *p, size_t n, const JpegFile &f, std::vector<JpegInterval> &out)
{
    out.clear();
    const size_t mcus = (size_t)f.mcux * f.mcuy;
    if (!p || f.restart < 1 || n > 0xffffffffull || f.scan > n || mcus < 1 || mcus > 0xffffffffull || f.blocks > 0xffffffffull) return false;
    const size_t count = (mcus + (size_t)f.restart - 1) / (size_t)f.restart;
    if (count > (n - f.scan) / 2 + 1) return false;          // every marker takes two bytes: the file cannot hold them (and the table is not sized from a header alone)
    out.reserve(count);
    // where Bits::restart() would find a marker at `at`: behind any fill bytes.  0: none
    const auto marker = [&](size_t at) -> size_t {
        while (at + 1 < n && p[at] == 0xff && p[at + 1] == 0xff) ++at;
        return at + 1 < n && p[at] == 0xff && p[at + 1] >= 0xd0 && p[at + 1] <= 0xd7 ? at + 2 : 0;
    };
    size_t pos = f.scan;
    for (size_t i = 0; i < count; ++i) {
        const size_t begin = pos;
        while (pos < n) {
            const uint8_t *ff = (const uint8_t *)memchr(p + pos, 0xff, n - pos);
            if (!ff) { pos = n; break; }
            pos = (size_t)(ff - p);
            if (pos + 1 < n && p[pos + 1] == 0) pos += 2; else break;
        }
        out.push_back(JpegInterval{(uint32_t)begin, (uint32_t)pos, (uint32_t)(i * (size_t)f.restart), (uint32_t)std::min<size_t>((size_t)f.restart, mcus - i * (size_t)f.restart)});
        const size_t next = marker(pos);
        if ((i + 1 < count) != (next != 0)) { out.clear(); return false; }          // a marker missing, something else in its place, or one marker too many
        pos = next;
    }
    return true;
}

void jpeg_entropy_tables(const JpegFile &f, JpegEntropyTables *t, JpegGeom *g)
{
    memset(t, 0, sizeof *t); memset(g, 0, sizeof *g);
    const auto put = [](JpegHuffTable &d, const JpegHuff &s) {
        memcpy(d.look, s.look, sizeof d.look); memcpy(d.vals, s.vals, sizeof d.vals);
        memcpy(d.maxcode, s.maxcode, sizeof d.maxcode); memcpy(d.delta, s.delta, sizeof d.delta);
        d.delta[0] = 0; d.maxcode[0] = 0;          // (never read, and never set by build_huffman)
    };
    g->comps = f.comps; g->hs = f.hs; g->vs = f.vs; g->mcux = f.mcux;
    for (int c = 0; c < f.comps; ++c) {
        put(t->dc[c], f.dc[f.td[c]]); put(t->ac[c], f.ac[f.ta[c]]);
        memcpy(t->quant[c], f.quant[f.tq[c]], sizeof t->quant[c]);
        g->bw[c] = (uint32_t)f.bw[c]; g->block0[c] = (uint32_t)f.block0[c];
    }
}

void JpegEntropyPlan::add(const JpegFile &f, size_t bytes, const std::vector<JpegInterval> &intervals, size_t block0)
{
    files.emplace_back();
    JpegDevFile &d = files.back();
    jpeg_entropy_tables(f, &d.t, &d.g);
    d.stream0 = stream_bytes; d.block0 = block0; d.bytes = (uint32_t)bytes; d.blocks = (uint32_t)f.blocks;
    stream_bytes += (bytes + 15) & ~(size_t)15;
    iv.insert(iv.end(), intervals.begin(), intervals.end());
    iv.resize((iv.size() + JPEG_ENTROPY_LANES - 1) / JPEG_ENTROPY_LANES * JPEG_ENTROPY_LANES, JpegInterval{0, 0, 0, 0});
    wg_file.resize(iv.size() / JPEG_ENTROPY_LANES, (uint32_t)(files.size() - 1));
    first_slot.push_back(iv.size());
}

}  // namespace yolo_impl
