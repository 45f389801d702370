// Malformed JPEG input against the host stage (yolo_tensorflow_amd/csrc/yolo_jpeg.cpp), as a stand-alone program for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I<repo> jpeg_malformed.cpp <repo>/yolo_tensorflow_amd/csrc/yolo_jpeg.cpp -pthread
//   ./a.out file.jpg [file.jpg ...]
// Every prefix of every file and 2000 seeded single-byte corruptions of each go through jpeg_parse and, where the headers pass, jpeg_decode.  Each
// call must come back with YOLO_OK or a YOLO_ERR_* and a message; the sanitizers turn any out-of-bounds access or undefined operation into a non-zero
// exit.  The input is copied into a heap block of exactly its size, so that one byte past the data is one byte past the allocation.
#include "include/yolo_hip.h"
#include "yolo_tensorflow_amd/csrc/yolo_jpeg.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

using namespace yolo_impl;

static long g_ok = 0, g_invalid = 0, g_unsupported = 0;

// one input through the decoder; false: a status that is no status, or a refusal without a message
static bool run(const unsigned char *data, size_t n)
{
    unsigned char *exact = (unsigned char *)malloc(n ? n : 1);
    memcpy(exact, data, n);
    JpegFile *f = new JpegFile;
    std::string msg;
    int r = jpeg_parse(exact, n, 0, f, msg);
    if (r == YOLO_OK) {
        std::vector<int16_t> coef(f->blocks * 64);
        r = jpeg_decode(exact, n, 0, *f, coef.data(), msg);
    }
    delete f;
    free(exact);
    if (r == YOLO_OK) { ++g_ok; return true; }
    if (r == YOLO_ERR_INVALID) ++g_invalid; else if (r == YOLO_ERR_UNSUPPORTED) ++g_unsupported; else { fprintf(stderr, "status %d\n", r); return false; }
    if (msg.compare(0, 8, "file 0: ") != 0) { fprintf(stderr, "a refusal without the file's index: \"%s\"\n", msg.c_str()); return false; }
    return true;
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
        const long ok0 = g_ok;
        if (!run(file.data(), file.size()) || g_ok != ok0 + 1) { fprintf(stderr, "%s: the intact file is refused\n", argv[a]); return 1; }
        for (size_t n = 0; n < file.size(); ++n)
            if (!run(file.data(), n)) { fprintf(stderr, "%s: prefix of %zu bytes\n", argv[a], n); return 1; }
        unsigned long long s = 0x9e3779b97f4a7c15ull * (unsigned long long)(a + 1);          // xorshift64*, seeded per file
        for (int k = 0; k < 2000; ++k) {
            s ^= s >> 12; s ^= s << 25; s ^= s >> 27;
            const unsigned long long v = s * 0x2545f4914f6cdd1dull;
            std::vector<unsigned char> bad = file;
            const size_t at = (size_t)((v >> 16) % file.size());
            unsigned char b = (unsigned char)(v & 255);
            if (b == bad[at]) b ^= 0x80;
            bad[at] = b;
            if (!run(bad.data(), bad.size())) { fprintf(stderr, "%s: byte %zu set to 0x%02x\n", argv[a], at, b); return 1; }
        }
    }
    printf("ok %ld invalid %ld unsupported %ld\n", g_ok, g_invalid, g_unsupported);
    return 0;
}
