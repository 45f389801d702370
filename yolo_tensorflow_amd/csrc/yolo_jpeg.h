// JPEG files, host stage: marker parsing and Huffman entropy decoding of sequential 8-bit JPEG (ITU-T T.81), down to the
// DEQUANTISED coefficient blocks.  Everything behind that -- IDCT, chroma upsampling, colour -- is the rule of kernels.h, evaluated by
// the device (k_jpeg_idct, AtFrame) and by the host twin alike.  Plain C++: no HIP, no context; compiles alone for the sanitizer run
// of tests/c/jpeg_malformed.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "jpeg_entropy.h"

namespace yolo_impl {

// a canonical Huffman table (T.81 annex C) with a 9-bit first-level lookup
struct JpegHuff {
    bool set = false;
    uint8_t vals[256];
    uint16_t look[512];        // (length << 8) | symbol of every code of at most 9 bits, 0: longer
    int32_t maxcode[18];       // largest code of each length, left-aligned to 16 bits, + 1; [17] ends every search
    int32_t delta[17];         // index of the first value of a length minus its first code
};

// one file after its headers: geometry, tables, where the entropy-coded segment begins
struct JpegFile {
    int h = 0, w = 0, comps = 0, hs = 1, vs = 1;     // (hs, vs): the luma sampling; chroma is 1 x 1.  Grey: 1 x 1 whatever the file states
    int format = 0;                                  // YOLO_PIX_JPEG_*
    int restart = 0;                                 // MCUs per restart interval, 0: none
    int mcux = 0, mcuy = 0;                          // MCUs across and down
    int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};        // blocks across and down every component plane (whole MCUs); the plane is 8 bw x 8 bh bytes
    size_t block0[3] = {0, 0, 0}, blocks = 0;        // first block of every plane in the coefficient array (plane by plane, row-major), and their count
    size_t scan = 0;                                 // byte offset of the entropy-coded segment
    int tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    uint16_t quant[4][64];                           // natural (de-zigzagged) order
    bool qset[4] = {false, false, false, false};
    JpegHuff dc[4], ac[4];
};

// headers of file `index` of a batch: YOLO_OK, YOLO_ERR_UNSUPPORTED (a kind of JPEG that is not served: msg names the file and the feature) or
// YOLO_ERR_INVALID (malformed or truncated: msg names the file and the byte offset)
int jpeg_parse(const uint8_t *file, size_t bytes, int index, JpegFile *out, std::string &msg);
// the entropy-coded segment of a parsed file -> coef[f.blocks][64] int16, dequantised, natural order: exactly what the reference hands to its IDCT,
// its wrap to 16 bits on the dequantising multiply included (stb_image.h stbi__jpeg_decode_block).  YOLO_OK or YOLO_ERR_INVALID
int jpeg_decode(const uint8_t *file, size_t bytes, int index, const JpegFile &f, int16_t *coef, std::string &msg);

// a parsed batch: file i into coef + first_block[i] * 64, by min(n, 8) threads that take one file at a time each (one thread, the caller's, when n == 1; the
// pool is never sized from the machine's processor count).  The failure of the lowest index is the one reported
int jpeg_decode_batch(const uint8_t *const *files, const size_t *bytes, int n, const JpegFile *parsed, const size_t *first_block, int16_t *coef, std::string &msg);
// the same for files which[0 .. count) of the batch alone (ascending indices; each keeps its index in the batch, in its messages too)
int jpeg_decode_some(const uint8_t *const *files, const size_t *bytes, const int *which, int count, const JpegFile *parsed, const size_t *first_block, int16_t *coef, std::string &msg);

// ---- the entropy stage over restart intervals (jpeg_entropy.h) ----
// One pass over the entropy-coded segment of a parsed file: its ceil(mcus / restart) restart intervals, `begin` the byte behind the preceding RSTm marker (f.scan
// for the first), `end` the offset of the first 0xFF that no 0x00 follows, or the file's end.  true: the file is ELIGIBLE for the interval decoder -- it has a DRI,
// its offsets fit 32 bits, and behind every interval but the last lies exactly what Bits::restart() accepts (fill bytes 0xFF, then one of 0xFF 0xD0 .. 0xD7) and
// behind the last no further such marker.  false is no error: the file goes to jpeg_decode, whose verdict stands; `out` is then left empty
bool jpeg_intervals(const uint8_t *file, size_t bytes, const JpegFile &f, std::vector<JpegInterval> &out);
// the tables and the geometry of a parsed file as the interval decoder reads them
void jpeg_entropy_tables(const JpegFile &f, JpegEntropyTables *t, JpegGeom *g);
// the eligible files of a batch as k_jpeg_entropy reads them (launch_jpeg_entropy, jpeg_entropy.h): one record per file, the interval table with every file's
// intervals padded to whole workgroups by idle slots, the file of every workgroup.  Entry k's slots are first_slot[k] .. first_slot[k + 1] - 1; its bytes begin at
// files[k].stream0 of a stream buffer of stream_bytes bytes
struct JpegEntropyPlan {
    std::vector<JpegDevFile> files; std::vector<uint32_t> wg_file; std::vector<JpegInterval> iv; std::vector<size_t> first_slot{0};
    size_t stream_bytes = 0;
    void clear() { files.clear(); wg_file.clear(); iv.clear(); first_slot.assign(1, 0); stream_bytes = 0; }
    // one more file: parsed, `bytes` long, with the intervals jpeg_intervals found, its blocks at block0 of the batch's coefficient array
    void add(const JpegFile &f, size_t bytes, const std::vector<JpegInterval> &intervals, size_t block0);
};

}  // namespace yolo_impl
