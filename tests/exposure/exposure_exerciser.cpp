// Host-only driver of csrc/rrt_exposure.h's bin rule and resolve walk for tests/test_exposure_host.py: plain C++, no HIP, built with
// -fsanitize=address,undefined and run as a program.
//   exposure_exerciser walk FILE   runs the sequences FILE describes through exposure_resolve_step, the source the resolve kernel
//                                  runs, and prints one line per frame; floats travel as their bits in hex, both ways.  FILE:
//                                    case NAME key ev low high min_ev max_ev adapt_up adapt_down N_FRAMES
//                                    frame K  b c  b c ...          (N_FRAMES lines: the K non-empty bins of the frame's histogram)
//                                  Output: NAME FRAME N m target ev scale frames
//   exposure_exerciser bins FILE   FILE holds luma bits in hex, one per line; prints each one's bin (-1: not metered)
// The histogram and the table live in heap cells of exactly 256 entries: an access outside them is the sanitizer's finding.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../relativisticraytracer_amd/csrc/rrt_math.h"
#include "../../relativisticraytracer_amd/csrc/rrt_exposure.h"

static float bits_f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t f_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint64_t d_bits(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }

static int run_walk(FILE* in) {
    std::unique_ptr<double[]> table(new double[kExposureBins]);
    for (int b = 0; b < kExposureBins; ++b) table[b] = exposure_bin_centre(b);
    char name[64];
    uint32_t key, ev, mn, mx, up, down;
    int low, high, n_frames;
    while (fscanf(in, " case %63s %" SCNx32 " %" SCNx32 " %d %d %" SCNx32 " %" SCNx32 " %" SCNx32 " %" SCNx32 " %d", name, &key, &ev, &low,
                  &high, &mn, &mx, &up, &down, &n_frames) == 10) {
        ExposureMeter s;
        s.log2_key = std::log2((double)bits_f(key));
        s.ev = bits_f(ev); s.min_ev = bits_f(mn); s.max_ev = bits_f(mx); s.adapt_up = bits_f(up); s.adapt_down = bits_f(down);
        s.low_permille = low; s.high_permille = high;
        ExposureState st;
        memset(&st, 0, sizeof(st));                                  // what exposure_reset leaves
        for (int f = 0; f < n_frames; ++f) {
            std::unique_ptr<uint32_t[]> hist(new uint32_t[kExposureBins]());
            int k;
            if (fscanf(in, " frame %d", &k) != 1) { fprintf(stderr, "exposure exerciser: case %s: frame %d missing\n", name, f); return 1; }
            for (int i = 0; i < k; ++i) {
                int b;
                uint32_t c;
                if (fscanf(in, "%d %" SCNu32, &b, &c) != 2 || b < 0 || b >= kExposureBins) {
                    fprintf(stderr, "exposure exerciser: case %s frame %d: bad bin\n", name, f);
                    return 1;
                }
                hist[b] = c;
            }
            exposure_resolve_step(hist.get(), table.get(), s, st);
            printf("%s %d %" PRIu64 " %016" PRIx64 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %" PRIu32 "\n", name, f, st.n, d_bits(st.m),
                   f_bits(st.target), f_bits(st.ev), f_bits(st.scale), st.frames);
        }
    }
    return 0;
}

static int run_bins(FILE* in) {
    uint32_t u;
    while (fscanf(in, "%" SCNx32, &u) == 1) printf("%08" PRIx32 " %d\n", u, exposure_bin(bits_f(u)));
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3 || (strcmp(argv[1], "walk") && strcmp(argv[1], "bins"))) {
        fprintf(stderr, "usage: exposure_exerciser walk|bins FILE\n");
        return 2;
    }
    FILE* in = fopen(argv[2], "r");
    if (!in) { fprintf(stderr, "exposure exerciser: cannot open %s\n", argv[2]); return 2; }
    const int rc = strcmp(argv[1], "walk") ? run_bins(in) : run_walk(in);
    fclose(in);
    if (rc == 0) printf("%s ok\n", argv[1]);
    return rc;
}
