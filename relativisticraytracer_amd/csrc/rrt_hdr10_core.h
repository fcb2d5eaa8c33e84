/*
 * rrt_hdr10_core.h -- the HDR10 leg of include/rrt_yuv.h ("HDR10 output", steps A-F) as functions the host and the device share
 * (RRT_FN), next to rrt_yuv_core.h, whose strips, codes and plane layout it uses unchanged.  rrt_yuv.hip's kernels, its
 * rrt_yuv_hdr10_from_hdr_host and tests/yuv/hdr10_exerciser.cpp run this very source.
 *
 * Everything is binary32, one rounding per written operation in the written order (the translation units build with
 * -ffp-contract=off); the division of step D is the plain IEEE `/`.
 */
#ifndef RRT_HDR10_CORE_H
#define RRT_HDR10_CORE_H

#include <stdio.h>
#include <string.h>

#include "rrt_yuv_core.h"

constexpr double kHdr10Kr = 0.2627, kHdr10Kb = 0.0593;       /* BT.2020 non-constant luminance */

/* the settings and the three values the host derives from them once, passed to the kernels by value next to the YuvPlan */
struct Hdr10Plan {
    float white, peak, knee;
    float K, span, inv;       /* K = knee * peak, span = peak - K, inv = 1.0f / span (unused, 0, when knee == 1) */
};

/* step F's running values: 32 bytes, 16-byte aligned, owned by the caller */
struct Hdr10Light {
    uint64_t frame_sum, max_frame_sum;
    uint32_t frame_max, max_cll, frames, reserved;
};
static_assert(sizeof(Hdr10Light) == 32, "include/rrt_yuv.h states 32 bytes");

/* A: NaN and negative values compare false: 0.  +inf stays +inf. */
RRT_FN float hdr10_light(float H, float white) { return (H > 0.0f) ? H * white : 0.0f; }

/* B: BT.709 -> BT.2020 in linear light (BT.2087); every term is >= 0 */
RRT_FN void hdr10_gamut(const float a[3], float b[3]) {
    b[0] = (0.6274f * a[0] + 0.3293f * a[1]) + 0.0433f * a[2];
    b[1] = (0.0691f * a[0] + 0.9195f * a[1]) + 0.0114f * a[2];
    b[2] = (0.0164f * a[0] + 0.0880f * a[1]) + 0.8956f * a[2];
}

/* C: the identity up to K, then the renderer's exponential curve towards `peak` */
RRT_FN float hdr10_shoulder(float b, const Hdr10Plan& t) {
    float c;
    if (b <= t.K) c = b;
    else if (t.knee == 1.0f) c = t.peak;
    else c = t.K + t.span * (1.0f - rrt_expf(-((b - t.K) * t.inv)));
    return c < t.peak ? c : t.peak;
}

/* D: SMPTE ST 2084 of c nits as a sixteen-bit component.  0 <= c <= peak <= 10000, so e <= 1 up to rounding and the cast is
 * defined. */
RRT_FN int hdr10_pq(float c) {
    const float y = c * 1.0e-4f;
    const float p = rrt_powf(y, 0.1593017578125f);
    const float e = rrt_powf((0.8359375f + 18.8515625f * p) / (1.0f + 18.6875f * p), 78.84375f);
    const int q = (int)(e * 65535.0f + 0.5f);
    return q < 65535 ? q : 65535;
}

/* A-D and F's fx of one pixel: H is its linear RGB (alpha is not read) */
RRT_FN void hdr10_pixel(float Hr, float Hg, float Hb, const Hdr10Plan& t, int q[3], uint32_t& fx) {
    const float a[3] = {hdr10_light(Hr, t.white), hdr10_light(Hg, t.white), hdr10_light(Hb, t.white)};
    float b[3];
    hdr10_gamut(a, b);
    const float c0 = hdr10_shoulder(b[0], t), c1 = hdr10_shoulder(b[1], t), c2 = hdr10_shoulder(b[2], t);
    q[0] = hdr10_pq(c0); q[1] = hdr10_pq(c1); q[2] = hdr10_pq(c2);
    float m = c0 > c1 ? c0 : c1;
    m = m > c2 ? m : c2;
    fx = (uint32_t)(m * 64.0f);           /* m <= 10000: at most 640000 */
}

/* what a thread (or the host loop) has metered so far */
struct Hdr10Meter {
    uint64_t sum;
    uint32_t max;
};

/* the loader of yuv_strip_narrow_with for this leg: a pixel past the frame's edge (a 4:2:0 duplicate) is converted, not metered */
struct Hdr10NarrowLoad {
    const float* hdr;
    const Hdr10Plan* t;
    Hdr10Meter* m;           /* NULL: no metering */
    int w, h;
    RRT_YUV_MEMBER void operator()(int col, int row, bool real, int q[3]) const {
        const float* f = hdr + 4 * ((size_t)(h - 1 - row) * (size_t)w + (size_t)col);
        uint32_t fx;
        hdr10_pixel(f[0], f[1], f[2], *t, q, fx);
        if (m && real) {
            m->sum += fx;
            if (fx > m->max) m->max = fx;
        }
    }
};

/* F's fold, behind a frame's pack */
RRT_FN void hdr10_fold(Hdr10Light* s) {
    if (s->frame_sum > s->max_frame_sum) s->max_frame_sum = s->frame_sum;
    if (s->frame_max > s->max_cll) s->max_cll = s->frame_max;
    s->frames += 1;
    s->frame_sum = 0;
    s->frame_max = 0;
}

/* ---- host only ---- */

static inline int hdr10_check(const rrt_yuv_hdr10* s) {
    if (!s) return RRT_ERR_INVALID_ARGUMENT;
    if (s->struct_size != sizeof(rrt_yuv_hdr10)) return RRT_ERR_ABI_MISMATCH;
    if (!std::isfinite(s->white_nits) || !std::isfinite(s->peak_nits)) return RRT_ERR_INVALID_ARGUMENT;
    if (!(s->white_nits > 0.0f) || !(s->peak_nits > 0.0f) || s->white_nits > 10000.0f || s->peak_nits > 10000.0f)
        return RRT_ERR_INVALID_ARGUMENT;
    if (!(s->knee >= 0.0f && s->knee <= 1.0f)) return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}

/* the format's and the settings' checks, the YuvPlan with BT.2020's coefficients, the derived values */
static inline int hdr10_plan(const rrt_yuv_format* f, const rrt_yuv_hdr10* s, int w, int h, YuvPlan& p, Hdr10Plan& t) {
    int rc = yuv_plan(f, w, h, p);
    if (rc != RRT_OK) return rc;
    if (f->bits != 10) return RRT_ERR_INVALID_ARGUMENT;
    if ((rc = hdr10_check(s)) != RRT_OK) return rc;
    yuv_coefficients(*f, p.coef, p.off, kHdr10Kr, kHdr10Kb);
    t.white = s->white_nits;
    t.peak = s->peak_nits;
    t.knee = s->knee;
    t.K = s->knee * s->peak_nits;
    t.span = s->peak_nits - t.K;
    t.inv = s->knee == 1.0f ? 0.0f : 1.0f / t.span;
    return RRT_OK;
}

static inline int hdr10_host(void* yuv, const float* hdr, int w, int h, const rrt_yuv_format* fmt, const rrt_yuv_hdr10* s,
                             Hdr10Light* light) {
    if (!yuv || !hdr) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    Hdr10Plan t;
    const int rc = hdr10_plan(fmt, s, w, h, p, t);
    if (rc != RRT_OK) return rc;
    const uintptr_t out = (uintptr_t)yuv, in = (uintptr_t)hdr, in_bytes = (uintptr_t)w * h * 16;
    if (out < in + in_bytes && in < out + yuv_bytes(p)) return RRT_ERR_INVALID_ARGUMENT;
    if (light) {
        const uintptr_t l = (uintptr_t)light;
        if ((l < in + in_bytes && in < l + sizeof(Hdr10Light)) || (l < out + yuv_bytes(p) && out < l + sizeof(Hdr10Light)))
            return RRT_ERR_INVALID_ARGUMENT;
    }
    Hdr10Meter m = {0, 0};
    const Hdr10NarrowLoad load = {hdr, &t, light ? &m : nullptr, w, h};
    for (int sy = 0; sy < p.strips_y; ++sy)
        for (int sx = 0; sx < p.strips_x; ++sx) yuv_strip_narrow_with(static_cast<uint8_t*>(yuv), p, sx, sy, load);
    if (light) {
        light->frame_sum += m.sum;
        if (m.max > light->frame_max) light->frame_max = m.max;
        hdr10_fold(light);
    }
    return RRT_OK;
}

/* MaxCLL, MaxFALL (ceilings, in integers) and the number of frames folded */
static inline int hdr10_levels(const Hdr10Light* s, int w, int h, uint32_t out[3]) {
    if (!s || !out || w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31)) return RRT_ERR_INVALID_ARGUMENT;
    const uint64_t per = 64ull * (uint64_t)w * (uint64_t)h;
    out[0] = (s->max_cll + 63u) / 64u;
    out[1] = (uint32_t)((s->max_frame_sum + per - 1) / per);
    out[2] = s->frames;
    return RRT_OK;
}

/* step G's sidecar: the bytes of <path>.hdr10.json */
static inline int hdr10_sidecar(const rrt_yuv_hdr10* s, const uint32_t levels[3], char* buf, size_t cap, size_t* len) {
    if (!levels || !buf || !len) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = hdr10_check(s);
    if (rc != RRT_OK) return rc;
    char md[128], text[1024];
    snprintf(md, sizeof(md), "G(8500,39850)B(6550,2300)R(35400,14600)WP(15635,16450)L(%lld,1)",
             (long long)std::llround((double)s->peak_nits * 10000.0));
    const int n = snprintf(text, sizeof(text),
                           "{\n"
                           "  \"white_nits\": %.9g,\n"
                           "  \"peak_nits\": %.9g,\n"
                           "  \"knee\": %.9g,\n"
                           "  \"max_cll\": %u,\n"
                           "  \"max_fall\": %u,\n"
                           "  \"frames\": %u,\n"
                           "  \"master_display\": \"%s\",\n"
                           "  \"x265\": \"--colorprim bt2020 --transfer smpte2084 --colormatrix bt2020nc --master-display \\\"%s\\\" "
                           "--max-cll \\\"%u,%u\\\"\",\n"
                           "  \"ffmpeg\": \"-color_primaries bt2020 -color_trc smpte2084 -colorspace bt2020nc\"\n"
                           "}\n",
                           (double)s->white_nits, (double)s->peak_nits, (double)s->knee, levels[0], levels[1], levels[2], md, md,
                           levels[0], levels[1]);
    if (n <= 0 || (size_t)n >= sizeof(text) || (size_t)n > cap) return RRT_ERR_INVALID_ARGUMENT;
    memcpy(buf, text, (size_t)n);
    *len = (size_t)n;
    return RRT_OK;
}

#endif /* RRT_HDR10_CORE_H */
