// Host-only driver of csrc/rrt_projection.h's lens_ray and lens_points for tests/test_lens_host.py: plain C++, no HIP, built with
// -fsanitize=address,undefined and run as a program.  Each case is a command-line word; a case prints "<case> ok" and exits 0, or
// says which expectation failed and exits 1.
//   rays      lens_ray over whole frames, cameras, lens points and focus distances -- zeros of both signs, denormals and huge values
//             among them: a finite origin and a unit direction, the zero rules bit for bit, (k, 0) == stereo_ray's eye bit for bit
//   points    lens_points into buffers of exactly 2 n floats (a write past the end is the sanitizer's finding): n = 1 is (0, 0),
//             every radius <= aperture, every refusal leaves the buffer untouched
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "../../include/rrt.h"

#define __host__
#define __device__
#define __forceinline__ inline
static inline void rrt_sincosf(float x, float* s, float* c) { *s = sinf(x); *c = cosf(x); }     // equirect only: not exercised here
#include "../../relativisticraytracer_amd/csrc/rrt_projection.h"

#define EXPECT(cond)                                                                    \
    do { if (!(cond)) { fprintf(stderr, "lens exerciser: %s failed (line %d)\n", #cond, __LINE__); return 1; } } while (0)

static bool same(const float* a, const float* b, int n) { return memcmp(a, b, n * sizeof(float)) == 0; }

static const rrt_camera kCams[] = {
    {{0.0f, 10.0f, -60.0f}, {0.0f, -0.17364818f, 0.98480775f}, {1.0f, 0.0f, 0.0f}, {0.0f, 0.98480775f, 0.17364818f}},
    {{-0.0f, 0.0f, -0.0f}, {0.6f, 0.0f, 0.8f}, {0.8f, 0.0f, -0.6f}, {0.0f, 1.0f, 0.0f}},
    {{12.0f, -3.0f, 40.0f}, {-0.63f, 0.37f, -0.68f}, {0.73f, 0.0f, -0.68f}, {0.25f, 0.93f, 0.27f}},
};

static int case_rays() {
    const float lens[] = {0.0f, -0.0f, 0.5f, -0.5f, 1e-42f, -1e-42f, 3.25f, 1e30f, -1e30f};
    const float focus[] = {12.0f, 1e-30f, 0.75f, 1e30f};
    const int sizes[][2] = {{1, 1}, {7, 3}, {33, 29}};
    long n = 0;
    for (const rrt_camera& cam : kCams)
        for (const auto& wh : sizes)
            for (float lx : lens)
                for (float ly : lens)
                    for (float z : focus) {
                        const int W = wh[0], H = wh[1];
                        const float cx = lx / z, cy = ly / z;
                        // one heap cell per output: a write outside them is the sanitizer's finding
                        std::unique_ptr<float[]> o(new float[3]), d(new float[3]);
                        for (int y = 0; y < H; ++y)
                            for (int x = 0; x < W; ++x) {
                                float uvx, uvy;
                                lens_ray(W, H, x, y, cam, 0, 0.0f, lx, ly, cx, cy, o.get(), d.get(), uvx, uvy);
                                ++n;
                                EXPECT(uvx == (float)x / (float)W && uvy == (float)y / (float)H);
                                if (std::isfinite(cx) && std::isfinite(cy) && fabsf(cx) < 1e18f && fabsf(cy) < 1e18f) {
                                    const double m = sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]);
                                    EXPECT(fabs(m - 1.0) < 1e-5);
                                }
                                if (fabsf(lx) < 1e29f && fabsf(ly) < 1e29f) EXPECT(std::isfinite(o[0]) && std::isfinite(o[1]) && std::isfinite(o[2]));
                                if (lx == 0.0f && ly == 0.0f) EXPECT(same(o.get(), cam.pos, 3));          // a signed-zero pos included
                                if (ly == 0.0f) {       // the lens point (k, 0) is the stereo pinhole's eye with k = e hb, c = k / convergence
                                    ProjArgs pj{RRT_PROJ_PINHOLE, 0.0f, 0.0f};
                                    StereoArgs sa{};
                                    sa.W = W; sa.H = H;
                                    sa.k_right = lx; sa.c_right = cx;
                                    float so[3], sd[3], su, sv;
                                    stereo_ray(pj, sa, RRT_EYE_RIGHT, x, y, cam, 0, 0.0f, so, sd, su, sv);
                                    EXPECT(same(so, o.get(), 3) && same(sd, d.get(), 3) && su == uvx && sv == uvy);
                                }
                            }
                    }
    EXPECT(n > 100000);
    // the lens distortion feeds the direction and the uv the vignette reads, never the origin
    float o0[3], d0[3], o1[3], d1[3], u0, v0, u1, v1;
    lens_ray(33, 29, 5, 20, kCams[0], 0, 0.0f, 0.5f, -0.25f, 0.04f, -0.02f, o0, d0, u0, v0);
    lens_ray(33, 29, 5, 20, kCams[0], 1, 0.2f, 0.5f, -0.25f, 0.04f, -0.02f, o1, d1, u1, v1);
    EXPECT(same(o0, o1, 3) && !same(d0, d1, 3) && u0 != u1 && v0 != v1);
    return 0;
}

static int case_points() {
    for (int n : {1, 2, 4, 8, 16})
        for (float a : {0.0f, 0.3f, 1e-40f, 2.5e20f})
            for (float rot : {0.0f, 1.0f, -7.5f, 1e20f}) {
                std::unique_ptr<float[]> xy(new float[2 * n]);
                EXPECT(lens_points(a, n, rot, xy.get()));
                for (int k = 0; k < n; ++k) {
                    const double r = sqrt((double)xy[2 * k] * xy[2 * k] + (double)xy[2 * k + 1] * xy[2 * k + 1]);
                    EXPECT(r <= (double)a * (1.0 + 1e-6));
                    if (n == 1) EXPECT(xy[0] == 0.0f && xy[1] == 0.0f);
                }
            }
    float keep[2] = {7.0f, 7.0f};
    for (int n : {0, -1, 3, 5, 12, 32, 1 << 30}) EXPECT(!lens_points(0.3f, n, 0.0f, keep));
    EXPECT(!lens_points(-0.1f, 4, 0.0f, keep) && !lens_points(NAN, 4, 0.0f, keep) && !lens_points(INFINITY, 4, 0.0f, keep));
    EXPECT(!lens_points(0.3f, 4, NAN, keep) && !lens_points(0.3f, 4, -INFINITY, keep) && !lens_points(0.3f, 4, 0.0f, nullptr));
    EXPECT(keep[0] == 7.0f && keep[1] == 7.0f);
    return 0;
}

int main(int argc, char** argv) {
    const char* c = argc > 1 ? argv[1] : "";
    int rc = 2;
    if (!strcmp(c, "rays")) rc = case_rays();
    else if (!strcmp(c, "points")) rc = case_points();
    else fprintf(stderr, "usage: lens_exerciser rays | points\n");
    if (rc == 0) printf("%s ok\n", c);
    return rc;
}
