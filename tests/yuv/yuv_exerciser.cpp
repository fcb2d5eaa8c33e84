// yuv_exerciser.cpp -- the Y'CbCr packing's shared source (csrc/rrt_yuv_core.h: the definition's functions, the plan and the host
// conversions librrt_yuv.so's *_host entry points call) as a program of its own, for AddressSanitizer and
// UndefinedBehaviorSanitizer (tests/test_yuv_host.py builds it with g++ and runs it as a child process).
//
//   yuv_exerciser frames FILE
//
// FILE holds any number of cases: a line `rgba|hdr CHROMA RANGE BITS W H`, then W*H*4 hexadecimal words -- a byte per component, or
// a float's bits.  Input and output buffers are allocated at exactly their sizes, so a read or a write past either end is
// reported.  Prints one line of hexadecimal frame bytes per case, then `frames ok`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../relativisticraytracer_amd/csrc/rrt_yuv_core.h"

int main(int argc, char** argv) {
    if (argc != 3 || strcmp(argv[1], "frames") != 0) { fprintf(stderr, "usage: yuv_exerciser frames FILE\n"); return 2; }
    FILE* fh = fopen(argv[2], "r");
    if (!fh) { perror("fopen"); return 2; }
    char kind[8];
    rrt_yuv_format fmt;
    fmt.struct_size = sizeof(fmt);
    int w, h;
    while (fscanf(fh, "%7s %d %d %d %d %d", kind, &fmt.chroma, &fmt.range, &fmt.bits, &w, &h) == 6) {
        const bool hdr = strcmp(kind, "hdr") == 0;
        const size_t n = (size_t)w * h * 4;
        YuvPlan p;
        if (yuv_plan(&fmt, w, h, p) != RRT_OK) { fprintf(stderr, "refused: %s %d %d %d %d %d\n", kind, fmt.chroma, fmt.range, fmt.bits, w, h); return 1; }
        uint8_t* bytes = hdr ? nullptr : static_cast<uint8_t*>(malloc(n));
        float* lin = hdr ? static_cast<float*>(malloc(n * sizeof(float))) : nullptr;
        for (size_t i = 0; i < n; ++i) {
            unsigned u;
            if (fscanf(fh, "%x", &u) != 1) { fprintf(stderr, "short case\n"); return 1; }
            if (hdr) lin[i] = rrt_u2f(u); else bytes[i] = (uint8_t)u;
        }
        const size_t out_bytes = (size_t)yuv_bytes(p);
        uint8_t* out = static_cast<uint8_t*>(malloc(out_bytes));
        const int rc = hdr ? yuv_host<true>(out, lin, w, h, &fmt) : yuv_host<false>(out, bytes, w, h, &fmt);
        if (rc != RRT_OK) { fprintf(stderr, "conversion refused: %d\n", rc); return 1; }
        for (size_t i = 0; i < out_bytes; ++i) printf("%02x", out[i]);
        printf("\n");
        free(out); free(bytes); free(lin);
    }
    fclose(fh);
    printf("frames ok\n");
    return 0;
}
