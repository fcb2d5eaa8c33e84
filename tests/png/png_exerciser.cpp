// png_exerciser.cpp -- the PNG filtering's shared source (csrc/rrt_png_core.h: the definition's functions, the plan, the host
// conversion, the inverse, the Adler fold and the header writer that librrt_png.so's host entry points call) as a program of its
// own, for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_png_host.py builds it with g++ and runs it as a child process).
//
//   png_exerciser frames FILE
//     FILE holds any number of cases: a line `DEPTH FILTER W H`, then W*H hexadecimal words (depth 8: a pixel's four bytes, R in the
//     low byte) or W*H*4 (depth 16: a float's bits each).  Input, payload, row sums and raw scanlines are allocated at exactly their
//     sizes, so a read or a write past either end is reported.  Per case it prints the payload, the row sums, the Adler-32 and the
//     header in hexadecimal, one line each, after checking that the payload un-filters to what the same frame gives with no filter.
//   png_exerciser refusals FILE
//     FILE is not read.  Every refusal of step 7, the size-1 frames and the exact-fit header buffer.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../relativisticraytracer_amd/csrc/rrt_png_core.h"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; }    \
    } while (0)

static int convert(void* out, uint32_t* sums, const void* src, int w, int h, const rrt_png_format* fmt) {
    return fmt && fmt->depth == 16 ? png_host<true>(out, sums, src, w, h, fmt) : png_host<false>(out, sums, src, w, h, fmt);
}

static int frames(const char* path) {
    FILE* fh = fopen(path, "r");
    if (!fh) { perror("fopen"); return 2; }
    rrt_png_format fmt;
    fmt.struct_size = sizeof(fmt);
    int w, h;
    while (fscanf(fh, "%d %d %d %d", &fmt.depth, &fmt.filter, &w, &h) == 4) {
        PngPlan p;
        CHECK(png_plan(&fmt, w, h, p) == RRT_OK);
        const size_t words = (size_t)w * h * (fmt.depth == 16 ? 4 : 1);
        uint32_t* src = static_cast<uint32_t*>(malloc(words * 4));
        for (size_t i = 0; i < words; ++i) {
            unsigned u;
            if (fscanf(fh, "%x", &u) != 1) { fprintf(stderr, "short case\n"); return 1; }
            src[i] = u;
        }
        const size_t n = (size_t)png_bytes(p), raw_bytes = (size_t)p.n * h;
        uint8_t* out = static_cast<uint8_t*>(malloc(n));
        uint32_t* sums = static_cast<uint32_t*>(malloc(8 * (size_t)h));
        CHECK(convert(out, sums, src, w, h, &fmt) == RRT_OK);
        // the inverse equals the unfiltered frame: its rows are the type byte 0 and the raw bytes
        rrt_png_format plain = fmt;
        plain.filter = RRT_PNG_NONE;
        uint8_t* none = static_cast<uint8_t*>(malloc(n));
        uint32_t* none_sums = static_cast<uint32_t*>(malloc(8 * (size_t)h));
        uint8_t* raw = static_cast<uint8_t*>(malloc(raw_bytes));
        CHECK(convert(none, none_sums, src, w, h, &plain) == RRT_OK);
        CHECK(png_unfilter(raw, out, w, h, &fmt) == RRT_OK);
        for (int r = 0; r < h; ++r) {
            CHECK(none[(size_t)r * p.stride] == 0);
            CHECK(memcmp(raw + (size_t)r * p.n, none + (size_t)r * p.stride + 1, p.n) == 0);
        }
        for (size_t i = 0; i < n; ++i) printf("%02x", out[i]);
        printf("\n");
        for (int i = 0; i < 2 * h; ++i) printf("%x ", sums[i]);
        printf("\n");
        uint32_t adler = 0;
        CHECK(png_adler32(sums, w, h, &fmt, &adler) == RRT_OK);
        printf("%08x\n", adler);
        size_t len = 0, len2 = 0;
        uint8_t probe[256];
        CHECK(png_header(&fmt, w, h, probe, sizeof(probe), &len) == RRT_OK);
        uint8_t* head = static_cast<uint8_t*>(malloc(len));          // an exact fit is enough
        CHECK(png_header(&fmt, w, h, head, len, &len2) == RRT_OK && len2 == len);
        for (size_t i = 0; i < len; ++i) printf("%02x", head[i]);
        printf("\n");
        free(head); free(raw); free(none_sums); free(none); free(sums); free(out); free(src);
    }
    fclose(fh);
    printf("frames ok\n");
    return 0;
}

static int refusals() {
    const int INVALID = RRT_ERR_INVALID_ARGUMENT;
    rrt_png_format ok;
    ok.struct_size = sizeof(ok);
    ok.depth = 8;
    ok.filter = RRT_PNG_ADAPTIVE;
    PngPlan p;
    CHECK(png_plan(&ok, 1, 1, p) == RRT_OK && g_png_err[0] == 0);
    CHECK(p.stride == 4 && png_bytes(p) == 4 && p.chunks == 2 && p.seg_chunks == 2);
    CHECK(png_plan(nullptr, 1, 1, p) == INVALID && g_png_err[0] != 0);
    CHECK(png_plan(&ok, 0, 1, p) == INVALID && png_plan(&ok, 1, 0, p) == INVALID && png_plan(&ok, -1, 4, p) == INVALID);
    rrt_png_format bad = ok;
    bad.struct_size = 8;
    CHECK(png_plan(&bad, 4, 4, p) == INVALID);
    for (int d : {0, 1, 4, 10, 24, -8}) { bad = ok; bad.depth = d; CHECK(png_plan(&bad, 4, 4, p) == INVALID); }
    for (int f : {-1, 6, 100}) { bad = ok; bad.filter = f; CHECK(png_plan(&bad, 4, 4, p) == INVALID); }
    for (int f = 0; f <= 5; ++f) { bad = ok; bad.filter = f; CHECK(png_plan(&bad, 4, 4, p) == RRT_OK); }
    // width * height >= 2^31, and below it a payload of 2^32 bytes or more: (1 + 3 w) h, (1 + 6 w) h
    CHECK(png_plan(&ok, 1 << 16, 1 << 15, p) == INVALID && png_plan(&ok, 46341, 46341, p) == INVALID);
    CHECK(png_plan(&ok, 46340, 46340, p) == INVALID);                   // 2147395600 pixels: the payload is 6.4e9 bytes
    CHECK(png_plan(&ok, 37838, 37838, p) == INVALID && png_plan(&ok, 37837, 37837, p) == RRT_OK);       // 4295180570 | 4294953544 bytes
    CHECK(png_plan(&ok, 1431655764, 1, p) == RRT_OK && p.stride == 4294967293u && png_plan(&ok, 1431655765, 1, p) == INVALID);
    bad = ok;
    bad.depth = 16;
    CHECK(png_plan(&bad, 715827882, 1, p) == RRT_OK && p.stride == 4294967293u && png_plan(&bad, 715827883, 1, p) == INVALID);
    CHECK(png_plan(&bad, 26755, 26755, p) == INVALID && png_plan(&bad, 26754, 26754, p) == RRT_OK);       // 4295006905 | 4294685850 bytes
    int32_t rows, n;
    CHECK(png_plan(&ok, 3840, 2160, p) == RRT_OK);
    png_slices(p, rows, n);
    CHECK(rows == 92 && n == 24);                                      // ceil(2^20 / 11521), ceil(2160 / 92)
    CHECK(png_plan(&ok, 1, 5, p) == RRT_OK);
    png_slices(p, rows, n);
    CHECK(rows == 5 && n == 1);
    // the size-1 frames, buffers sized exactly, every filter
    for (int depth : {8, 16})
        for (int f = 0; f <= 5; ++f) {
            rrt_png_format fmt = ok;
            fmt.depth = depth;
            fmt.filter = f;
            CHECK(png_plan(&fmt, 1, 1, p) == RRT_OK);
            const size_t in_bytes = depth == 8 ? 4 : 16, n_out = (size_t)png_bytes(p);
            uint8_t* px = static_cast<uint8_t*>(malloc(in_bytes));
            if (depth == 8) { px[0] = 10; px[1] = 200; px[2] = 0; px[3] = 77; }
            else { const float v[4] = {0.0f, -1.0f, 1.0e30f, 1.0f}; memcpy(px, v, 16); }
            uint8_t* out = static_cast<uint8_t*>(malloc(n_out));
            uint8_t* back = static_cast<uint8_t*>(malloc(n_out - 1));
            uint32_t* sums = static_cast<uint32_t*>(malloc(8));
            CHECK(convert(out, sums, px, 1, 1, &fmt) == RRT_OK);
            CHECK(out[0] == (f == RRT_PNG_ADAPTIVE ? 0 : f));           // one pixel under a zero row: five equal scores, the lowest type
            CHECK(png_unfilter(back, out, 1, 1, &fmt) == RRT_OK);
            if (depth == 8) { const uint8_t want[3] = {10, 200, 0}; CHECK(memcmp(back, want, 3) == 0); }
            else { const uint8_t want[6] = {0, 0, 0, 0, 0xff, 0xff}; CHECK(memcmp(back, want, 6) == 0); }
            CHECK(convert(nullptr, sums, px, 1, 1, &fmt) == INVALID && convert(out, nullptr, px, 1, 1, &fmt) == INVALID);
            CHECK(convert(out, sums, nullptr, 1, 1, &fmt) == INVALID);
            CHECK(convert(px + 1, sums, px, 1, 1, &fmt) == INVALID);                               // the output inside the input
            CHECK(convert(out, reinterpret_cast<uint32_t*>(out), px, 1, 1, &fmt) == INVALID);     // the sums inside the output
            // the other entry point's depth: refused before a byte is read
            CHECK((depth == 16 ? png_host<false>(out, sums, px, 1, 1, &fmt) : png_host<true>(out, sums, px, 1, 1, &fmt)) == INVALID);
            free(sums); free(back); free(out); free(px);
        }
    uint8_t pay[4] = {5, 1, 2, 3}, raw[3];
    CHECK(png_unfilter(raw, pay, 1, 1, &ok) == INVALID);                // a type byte off the list
    pay[0] = 1;
    CHECK(png_unfilter(nullptr, pay, 1, 1, &ok) == INVALID && png_unfilter(raw, nullptr, 1, 1, &ok) == INVALID);
    CHECK(png_unfilter(pay + 1, pay, 1, 1, &ok) == INVALID);
    CHECK(png_unfilter(raw, pay, 1, 1, &ok) == RRT_OK && raw[0] == 1 && raw[1] == 2 && raw[2] == 3);
    uint32_t sums[2] = {7, 9}, adler = 0;
    CHECK(png_adler32(nullptr, 1, 1, &ok, &adler) == INVALID && png_adler32(sums, 1, 1, &ok, nullptr) == INVALID);
    CHECK(png_adler32(sums, 1, 1, &ok, &adler) == RRT_OK && adler == (((9u + 4u) << 16) | 8u));
    uint8_t head[256];
    size_t len = 0, len2 = 0;
    CHECK(png_header(&ok, 2, 1, nullptr, 256, &len) == INVALID && png_header(&ok, 2, 1, head, 256, nullptr) == INVALID);
    CHECK(png_header(&ok, 0, 1, head, 256, &len) == INVALID);
    CHECK(png_header(&ok, 2, 1, head, 256, &len) == RRT_OK && len == 8 + 25 + 13 + 12 + 9 + 25);
    memset(head, 0xee, sizeof(head));
    CHECK(png_header(&ok, 2, 1, head, len - 1, &len2) == INVALID && head[0] == 0xee);      // too small: nothing is written
    int32_t g[8];
    CHECK(png_plan(&ok, 1, 1, p) == RRT_OK);
    png_geometry(p, 0, g);
    CHECK(g[0] == kPngWideThreads && g[6] == 1 && g[4] == 1);
    png_geometry(p, 4, g);
    CHECK(g[0] == kPngNarrowThreads && g[6] == 0 && g[5] == 0);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "frames") == 0) return frames(argv[2]);
    if (argc == 3 && strcmp(argv[1], "refusals") == 0) return refusals();
    fprintf(stderr, "usage: png_exerciser frames|refusals FILE\n");
    return 2;
}
