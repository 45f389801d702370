// The restart-interval entropy decoder (yolo_tensorflow_amd/csrc/jpeg_entropy.h, the function k_jpeg_entropy runs per lane) against malformed input and against
// the host decoder, as a stand-alone program for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I<repo> jpeg_intervals.cpp <repo>/yolo_tensorflow_amd/csrc/yolo_jpeg.cpp -pthread
//   ./a.out file.jpg [file.jpg ...]          (files with a restart interval)
// Every prefix of every file and 2000 seeded single-byte corruptions of each go through jpeg_parse -> jpeg_intervals -> jpeg_decode_interval, over an array filled
// with a pattern, so that a coefficient the decoder leaves unwritten shows.  The file lies in a heap block of exactly its size
// and the coefficients in one of exactly blocks x 64 shorts, so that the sanitizers turn any access outside either into a non-zero exit.  The contract checked on
// every eligible input: all intervals 0 => jpeg_decode returns YOLO_OK with the same coefficients; jpeg_decode refuses => some interval is not 0.
#include "include/yolo_hip.h"
#include "yolo_tensorflow_amd/csrc/yolo_jpeg.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace yolo_impl;

static long g_not_eligible = 0, g_clean = 0, g_handed_back = 0, g_host_refused = 0;

static unsigned decode_all(const unsigned char *file, const std::vector<JpegInterval> &iv, const JpegEntropyTables &t, const JpegGeom &g, int16_t *coef, size_t blocks)
{
    unsigned worst = 0;
    for (const JpegInterval &v : iv) {
        const unsigned st = jpeg_decode_interval(file, v.begin, v.end, t, v.first_mcu, v.mcus, g, coef, blocks);
        if (st > JPEG_IV_STORE) { fprintf(stderr, "status %u\n", st); exit(1); }
        if (st && !worst) worst = st;
    }
    return worst;
}

// one input; false: the contract is broken
static bool run(const unsigned char *data, size_t n, bool must_be_clean)
{
    unsigned char *exact = (unsigned char *)malloc(n ? n : 1);
    memcpy(exact, data, n);
    JpegFile *f = new JpegFile;
    std::string msg;
    bool good = true;
    std::vector<JpegInterval> iv;
    if (jpeg_parse(exact, n, 0, f, msg) != YOLO_OK || !jpeg_intervals(exact, n, *f, iv)) {
        ++g_not_eligible;
        if (must_be_clean) { fprintf(stderr, "the intact file is not eligible\n"); good = false; }
    } else {
        const size_t mcus = (size_t)f->mcux * f->mcuy, shorts = f->blocks * 64;
        if (iv.size() != (mcus + f->restart - 1) / f->restart) { fprintf(stderr, "%zu intervals for %zu MCUs in steps of %d\n", iv.size(), mcus, f->restart); good = false; }
        for (size_t i = 0; i < iv.size(); ++i)
            if (iv[i].begin > iv[i].end || iv[i].end > n || iv[i].first_mcu != i * (size_t)f->restart || iv[i].first_mcu + iv[i].mcus > mcus || !iv[i].mcus) { fprintf(stderr, "interval %zu is malformed\n", i); good = false; }
        JpegEntropyTables *t = new JpegEntropyTables; JpegGeom g;
        jpeg_entropy_tables(*f, t, &g);
        int16_t *host = (int16_t *)malloc(shorts * 2), *a = (int16_t *)malloc(shorts * 2);
        memset(a, 0x55, shorts * 2);
        const int r = jpeg_decode(exact, n, 0, *f, host, msg);
        const unsigned sa = good ? decode_all(exact, iv, *t, g, a, f->blocks) : 0;
        if (r != YOLO_OK && r != YOLO_ERR_INVALID) { fprintf(stderr, "host status %d\n", r); good = false; }
        if (r != YOLO_OK) ++g_host_refused;
        if (!sa) {
            ++g_clean;
            if (r != YOLO_OK) { fprintf(stderr, "every interval is clean, the host refuses: %s\n", msg.c_str()); good = false; }
            else if (memcmp(host, a, shorts * 2)) { fprintf(stderr, "every interval is clean, the coefficients differ\n"); good = false; }
        } else {
            ++g_handed_back;
            if (must_be_clean) { fprintf(stderr, "the intact file: status %u\n", sa); good = false; }
        }
        free(host); free(a); delete t;
    }
    delete f;
    free(exact);
    return good;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s file.jpg ...\n", argv[0]); return 2; }
    for (int a = 1; a < argc; ++a) {
        FILE *fp = fopen(argv[a], "rb");
        if (!fp) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        std::vector<unsigned char> file;
        for (int ch; (ch = fgetc(fp)) != EOF;) file.push_back((unsigned char)ch);
        fclose(fp);
        if (!run(file.data(), file.size(), true)) { fprintf(stderr, "%s: the intact file\n", argv[a]); return 1; }
        for (size_t n = 0; n < file.size(); ++n)
            if (!run(file.data(), n, false)) { fprintf(stderr, "%s: prefix of %zu bytes\n", argv[a], n); return 1; }
        unsigned long long s = 0x9e3779b97f4a7c15ull * (unsigned long long)(a + 1);          // xorshift64*, seeded per file
        for (int k = 0; k < 2000; ++k) {
            s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
            const unsigned long long v = s * 0x2545f4914f6cdd1dull;
            std::vector<unsigned char> bad = file;
            const size_t at = (size_t)((v >> 16) % file.size());
            unsigned char b = (unsigned char)(v & 255);
            if (b == bad[at]) b ^= 0x80;
            bad[at] = b;
            if (!run(bad.data(), bad.size(), false)) { fprintf(stderr, "%s: byte %zu set to 0x%02x\n", argv[a], at, b); return 1; }
        }
    }
    printf("not_eligible %ld clean %ld handed_back %ld host_refused %ld\n", g_not_eligible, g_clean, g_handed_back, g_host_refused);
    return 0;
}
