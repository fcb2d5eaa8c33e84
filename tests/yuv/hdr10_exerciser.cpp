// hdr10_exerciser.cpp -- the HDR10 leg's shared source (csrc/rrt_hdr10_core.h: steps A-F, the plan, the strips' loader, the fold) as
// a program of its own, for AddressSanitizer and UndefinedBehaviorSanitizer (tests/test_yuv_hdr10_host.py builds it with g++ and runs
// it as a child process).
//
//   hdr10_exerciser frames FILE
//
// FILE holds any number of cases: a line `CHROMA RANGE W H WHITE PEAK KNEE` (the three settings as a float's bits, hexadecimal), then
// W*H*4 hexadecimal words, a float's bits each.  The input is allocated at exactly its size.  The planes are written one by one
// into a buffer that keeps kGuard sentinel bytes in front of, between and behind them (the plan's plane offsets are moved apart),
// and the light-level state sits between sentinels too: a write outside a plane or the state is reported even where it would land in
// the neighbouring plane.  Prints per case one line of hexadecimal frame bytes and one of the state's 32 bytes, then `frames ok`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../relativisticraytracer_amd/csrc/rrt_hdr10_core.h"

constexpr size_t kGuard = 32;
constexpr uint8_t kSentinel = 0xA5;

struct GuardedLight {
    uint8_t before[16];
    Hdr10Light light;
    uint8_t after[16];
};

static bool all_sentinel(const uint8_t* p, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (p[i] != kSentinel) return false;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 3 || strcmp(argv[1], "frames") != 0) { fprintf(stderr, "usage: hdr10_exerciser frames FILE\n"); return 2; }
    FILE* fh = fopen(argv[2], "r");
    if (!fh) { perror("fopen"); return 2; }
    rrt_yuv_format fmt;
    fmt.struct_size = sizeof(fmt);
    fmt.bits = 10;
    rrt_yuv_hdr10 set;
    set.struct_size = sizeof(set);
    int w, h;
    unsigned uw, up, uk;
    while (fscanf(fh, "%d %d %d %d %x %x %x", &fmt.chroma, &fmt.range, &w, &h, &uw, &up, &uk) == 7) {
        set.white_nits = rrt_u2f(uw); set.peak_nits = rrt_u2f(up); set.knee = rrt_u2f(uk);
        YuvPlan p;
        Hdr10Plan t;
        if (hdr10_plan(&fmt, &set, w, h, p, t) != RRT_OK) { fprintf(stderr, "refused: %d %d %d %d\n", fmt.chroma, fmt.range, w, h); return 1; }
        const size_t n = (size_t)w * h * 4;
        float* lin = static_cast<float*>(malloc(n * sizeof(float)));
        for (size_t i = 0; i < n; ++i) {
            unsigned u;
            if (fscanf(fh, "%x", &u) != 1) { fprintf(stderr, "short case\n"); return 1; }
            lin[i] = rrt_u2f(u);
        }
        // the tight layout's plane sizes; then the planes moved apart
        const size_t size[3] = {(size_t)(p.plane[1] - p.plane[0]), (size_t)(p.plane[2] - p.plane[1]), (size_t)(p.plane[2] - p.plane[1])};
        const size_t total = 4 * kGuard + size[0] + size[1] + size[2];
        p.plane[0] = kGuard;
        p.plane[1] = p.plane[0] + size[0] + kGuard;
        p.plane[2] = p.plane[1] + size[1] + kGuard;
        uint8_t* out = static_cast<uint8_t*>(malloc(total));
        memset(out, kSentinel, total);
        GuardedLight g;
        memset(&g, kSentinel, sizeof(g));
        g.light = Hdr10Light{0, 0, 0, 0, 0, 0};
        // one frame, twice: the second fold must leave the maxima and count two frames
        for (int pass = 0; pass < 2; ++pass) {
            Hdr10Meter m = {0, 0};
            const Hdr10NarrowLoad load = {lin, &t, &m, w, h};
            for (int sy = 0; sy < p.strips_y; ++sy)
                for (int sx = 0; sx < p.strips_x; ++sx) yuv_strip_narrow_with(out, p, sx, sy, load);
            g.light.frame_sum += m.sum;
            if (m.max > g.light.frame_max) g.light.frame_max = m.max;
            hdr10_fold(&g.light);
        }
        bool ok = all_sentinel(out, kGuard) && all_sentinel(out + total - kGuard, kGuard) && all_sentinel(g.before, sizeof(g.before)) &&
                  all_sentinel(g.after, sizeof(g.after));
        for (int c = 1; c < 3; ++c) ok = ok && all_sentinel(out + p.plane[c] - kGuard, kGuard);
        if (!ok) { fprintf(stderr, "a guard was overwritten: %d %d %d %d\n", fmt.chroma, fmt.range, w, h); return 1; }
        for (int c = 0; c < 3; ++c)
            for (size_t i = 0; i < size[c]; ++i) printf("%02x", out[p.plane[c] + i]);
        printf("\n");
        const uint8_t* s = reinterpret_cast<const uint8_t*>(&g.light);
        for (size_t i = 0; i < sizeof(Hdr10Light); ++i) printf("%02x", s[i]);
        printf("\n");
        free(out); free(lin);
    }
    fclose(fh);
    printf("frames ok\n");
    return 0;
}
