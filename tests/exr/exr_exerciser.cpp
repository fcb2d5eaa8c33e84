// exr_exerciser.cpp -- the EXR packing's shared source (csrc/rrt_exr_core.h: the definition's functions, the plan, the host
// conversion, the filter's inverse and the header writer that librrt_exr.so's host entry points call) as a program of its own, for
// AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_exr_host.py builds it with g++ and runs it as a child process).
//
//   exr_exerciser frames FILE
//     FILE holds any number of cases: a line `TYPE COMPRESSION HALF_MAX_BITS W H` (the format's codes; half_max as the hexadecimal
//     bits of its float), then W*H*4 hexadecimal words, a float's bits each.  Input and output buffers are allocated at exactly
//     their sizes, so a read or a write past either end is reported.  Per case it prints the payload and the header in hexadecimal,
//     one line each, after checking that every filtered chunk un-filters to the chunk the same frame gives without compression.
//   exr_exerciser refusals FILE
//     FILE is not read.  Every refusal of the host entry points, the size-1 cases and the exact-fit header buffer.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../relativisticraytracer_amd/csrc/rrt_exr_core.h"

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 1; }    \
    } while (0)

static float bits_float(unsigned u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

static int frames(const char* path) {
    FILE* fh = fopen(path, "r");
    if (!fh) { perror("fopen"); return 2; }
    rrt_exr_format fmt;
    fmt.struct_size = sizeof(fmt);
    unsigned max_bits;
    int w, h;
    while (fscanf(fh, "%d %d %x %d %d", &fmt.type, &fmt.compression, &max_bits, &w, &h) == 5) {
        fmt.half_max = bits_float(max_bits);
        ExrPlan p;
        CHECK(exr_plan(&fmt, w, h, p) == RRT_OK);
        const size_t n = (size_t)w * h * 4;
        float* lin = static_cast<float*>(malloc(n * sizeof(float)));
        for (size_t i = 0; i < n; ++i) {
            unsigned u;
            if (fscanf(fh, "%x", &u) != 1) { fprintf(stderr, "short case\n"); return 1; }
            lin[i] = bits_float(u);
        }
        const size_t out_bytes = (size_t)exr_bytes(p);
        uint8_t* out = static_cast<uint8_t*>(malloc(out_bytes));
        CHECK(exr_host(out, lin, w, h, &fmt) == RRT_OK);
        if (fmt.compression != RRT_EXR_NONE) {      // every chunk's inverse, into a buffer of exactly its size
            rrt_exr_format plain = fmt;
            plain.compression = RRT_EXR_NONE;
            uint8_t* raw = static_cast<uint8_t*>(malloc(out_bytes));
            CHECK(exr_host(raw, lin, w, h, &plain) == RRT_OK);
            for (int y = 0; y < h; y += p.lines) {
                int y0, rows;
                size_t offset;
                exr_chunk_of(p, y, y0, rows, offset);
                const size_t bytes = (size_t)rows * w * 3 * p.bps;
                uint8_t* back = static_cast<uint8_t*>(malloc(bytes));
                CHECK(exr_unfilter(back, out + offset, bytes) == RRT_OK);
                CHECK(memcmp(back, raw + offset, bytes) == 0);
                free(back);
            }
            free(raw);
        }
        for (size_t i = 0; i < out_bytes; ++i) printf("%02x", out[i]);
        printf("\n");
        size_t len = 0;
        uint8_t probe[1024];
        CHECK(exr_header(&fmt, w, h, 24, 1, probe, sizeof(probe), &len) == RRT_OK);
        uint8_t* head = static_cast<uint8_t*>(malloc(len));          // an exact fit is enough
        size_t len2 = 0;
        CHECK(exr_header(&fmt, w, h, 24, 1, head, len, &len2) == RRT_OK && len2 == len);
        for (size_t i = 0; i < len; ++i) printf("%02x", head[i]);
        printf("\n");
        free(head); free(out); free(lin);
    }
    fclose(fh);
    printf("frames ok\n");
    return 0;
}

static int refusals() {
    const int INVALID = RRT_ERR_INVALID_ARGUMENT;
    rrt_exr_format ok;
    ok.struct_size = sizeof(ok);
    ok.type = RRT_EXR_HALF;
    ok.compression = RRT_EXR_ZIP;
    ok.half_max = 65504.0f;
    ExrPlan p;
    CHECK(exr_plan(&ok, 1, 1, p) == RRT_OK && g_exr_err[0] == 0);
    CHECK(p.n_chunks == 1 && exr_bytes(p) == 6);
    CHECK(exr_plan(nullptr, 1, 1, p) == INVALID && g_exr_err[0] != 0);
    CHECK(exr_plan(&ok, 0, 1, p) == INVALID && exr_plan(&ok, 1, 0, p) == INVALID && exr_plan(&ok, -1, 4, p) == INVALID);
    rrt_exr_format bad = ok;
    bad.struct_size = 12;
    CHECK(exr_plan(&bad, 4, 4, p) == INVALID);
    for (int t : {0, 3, -1}) { bad = ok; bad.type = t; CHECK(exr_plan(&bad, 4, 4, p) == INVALID); }
    for (int c : {1, 4, -1}) { bad = ok; bad.compression = c; CHECK(exr_plan(&bad, 4, 4, p) == INVALID); }
    const float inf = std::numeric_limits<float>::infinity();
    for (float m : {0.0f, -1.0f, inf, std::nanf(""), 65520.0f, 1024.5f, 1.0e-9f, 65505.0f}) { bad = ok; bad.half_max = m; CHECK(exr_plan(&bad, 4, 4, p) == INVALID); }
    for (float m : {65504.0f, 1024.0f, 1.0f, 5.9604644775390625e-8f, 6.103515625e-5f}) { bad = ok; bad.half_max = m; CHECK(exr_plan(&bad, 4, 4, p) == RRT_OK); }
    // a chunk of 2^31 bytes or more: 16 rows x 3 channels x 2 bytes x width
    CHECK(exr_plan(&ok, 22369622, 16, p) == INVALID && exr_plan(&ok, 22369621, 16, p) == RRT_OK);
    bad = ok;
    bad.type = RRT_EXR_FLOAT;
    bad.compression = RRT_EXR_ZIPS;
    CHECK(exr_plan(&bad, 178956971, 1, p) == INVALID && exr_plan(&bad, 178956970, 1 << 20, p) == RRT_OK);
    // the size-1 frame, buffers sized exactly, every format
    for (int t : {RRT_EXR_HALF, RRT_EXR_FLOAT})
        for (int c : {RRT_EXR_NONE, RRT_EXR_ZIPS, RRT_EXR_ZIP}) {
            rrt_exr_format f = ok;
            f.type = t;
            f.compression = c;
            CHECK(exr_plan(&f, 1, 1, p) == RRT_OK);
            float* px = static_cast<float*>(malloc(16));
            px[0] = 1.0f; px[1] = 0.5f; px[2] = -2.0f; px[3] = 1.0f;
            const size_t n = (size_t)exr_bytes(p);
            uint8_t* out = static_cast<uint8_t*>(malloc(n));
            uint8_t* back = static_cast<uint8_t*>(malloc(n));
            CHECK(exr_host(out, px, 1, 1, &f) == RRT_OK);
            if (c != RRT_EXR_NONE) CHECK(exr_unfilter(back, out, n) == RRT_OK); else memcpy(back, out, n);
            if (t == RRT_EXR_HALF) { const uint8_t want[6] = {0x00, 0xc0, 0x00, 0x38, 0x00, 0x3c}; CHECK(memcmp(back, want, 6) == 0); }
            else { const float want[3] = {-2.0f, 0.5f, 1.0f}; CHECK(memcmp(back, want, 12) == 0); }
            CHECK(exr_host(nullptr, px, 1, 1, &f) == INVALID && exr_host(out, nullptr, 1, 1, &f) == INVALID);
            CHECK(exr_host(reinterpret_cast<uint8_t*>(px) + 4, px, 1, 1, &f) == INVALID);      // the output inside the input
            free(back); free(out); free(px);
        }
    uint8_t a[8] = {1, 2, 3, 4, 5, 6, 7, 8}, b[8];
    CHECK(exr_unfilter(nullptr, a, 8) == INVALID && exr_unfilter(b, nullptr, 8) == INVALID);
    CHECK(exr_unfilter(b, a, 0) == INVALID && exr_unfilter(b, a, 7) == INVALID && exr_unfilter(a, a, 8) == INVALID && exr_unfilter(a + 2, a, 4) == INVALID);
    CHECK(exr_unfilter(b, a, 2) == RRT_OK && b[0] == 1 && b[1] == (uint8_t)(1 + 2 - 128));
    uint8_t head[1024];
    size_t len = 0;
    CHECK(exr_header(&ok, 2, 1, 24, 1, nullptr, 1024, &len) == INVALID && exr_header(&ok, 2, 1, 24, 1, head, 1024, nullptr) == INVALID);
    CHECK(exr_header(&ok, 2, 1, 0, 1, head, 1024, &len) == INVALID && exr_header(&ok, 2, 1, 24, 0, head, 1024, &len) == INVALID);
    CHECK(exr_header(&ok, 0, 1, 24, 1, head, 1024, &len) == INVALID);
    CHECK(exr_header(&ok, 2, 1, 24, 1, head, 1024, &len) == RRT_OK && len > 8);
    memset(head, 0xee, sizeof(head));
    size_t len2 = 0;
    CHECK(exr_header(&ok, 2, 1, 24, 1, head, len - 1, &len2) == INVALID && head[0] == 0xee);      // too small: nothing is written
    int32_t g[8];
    exr_geometry(p, 0, g);
    CHECK(g[0] == kExrBlockX * kExrBlockY && g[6] == 0);
    printf("refusals ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && strcmp(argv[1], "frames") == 0) return frames(argv[2]);
    if (argc == 3 && strcmp(argv[1], "refusals") == 0) return refusals();
    fprintf(stderr, "usage: exr_exerciser frames|refusals FILE\n");
    return 2;
}
