/*
 * rrt_exr_core.h -- the definition of include/rrt_exr.h as functions the host and the device share (RRT_FN, as rrt_yuv_core.h):
 * plain C++ that g++ can include.  rrt_exr.hip's kernels and its *_host entry points, and tests/exr/exr_exerciser.cpp, run this
 * very source.
 *
 * A chunk's samples are numbered s = (row_in_chunk * 3 + channel) * width + x, channel 0 = B, 1 = G, 2 = R: the order of its raw
 * bytes.  exr_put_sample packs ONE sample -- the narrow path, at any size and alignment; the wide kernel of rrt_exr.hip calls the
 * same exr_sample / exr_filter_sample with vector loads and stores.
 */
#ifndef RRT_EXR_CORE_H
#define RRT_EXR_CORE_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../include/rrt_exr.h"
#include "rrt_math.h"     /* RRT_FN */

constexpr int kExrBlockX = 64, kExrBlockY = 4;      /* a workgroup: 64 units along a row (one wavefront) x 4 rows */
constexpr int kExrMaxGridY = 1024;                  /* beyond kExrBlockY * kExrMaxGridY = 4096 rows the workgroups take the rows in passes */
constexpr int kExrWidePixels = 8;                   /* the wide path: pixels of a row per thread */

/* What a launch needs of the format and the size, checked and computed once on the host (exr_plan) and passed by value */
struct ExrPlan {
    int32_t w, h;
    int32_t type, compression;
    int32_t lines;            /* scanlines per chunk: 1 | 16 */
    int32_t bps;              /* bytes per sample: 2 | 4 */
    int32_t n_chunks;
    uint32_t max_half;        /* the bits of half_max */
};

/* IEEE binary32 bits -> binary16 bits, round to nearest even, subnormal halves kept; NaN -> +0; what rounds above max_half (the
 * bits of a finite positive half), +-inf included, -> +-max_half.  Integer arithmetic only. */
RRT_FN uint32_t exr_half_bits(uint32_t u, uint32_t max_half) {
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return 0u;                      /* NaN */
    uint32_t h;
    if (a >= 0x47800000u) {                              /* >= 65536, inf included: above every finite half */
        h = 0x7c00u;
    } else if (a >= 0x38800000u) {                       /* >= 2^-14: a normal half -- re-bias the exponent, round 13 bits away */
        const uint32_t m = a - 0x38000000u;
        h = (m + 0xfffu + ((m >> 13) & 1u)) >> 13;       /* a carry out of the mantissa moves to the next exponent: up to 0x7c00 */
    } else if (a >= 0x33000000u) {                       /* [2^-25, 2^-14): a subnormal half, in units of 2^-24 */
        const uint32_t shift = 126u - (a >> 23);         /* 14 ... 24 */
        const uint32_t mant = (a & 0x7fffffu) | 0x800000u;
        const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        h = mant >> shift;
        if (rem > half || (rem == half && (h & 1u))) ++h;       /* 0x3ff + 1 is the smallest normal half */
    } else {
        h = 0u;                                          /* below 2^-25: nearer to 0 than to the smallest subnormal */
    }
    if (h > max_half) h = max_half;
    return sign | h;
}

/* the stored bits of one binary32 sample */
RRT_FN uint32_t exr_sample(const ExrPlan& p, uint32_t u) { return p.type == RRT_EXR_HALF ? exr_half_bits(u, p.max_half) : u; }

RRT_FN uint32_t exr_float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

/* channel c (0 B, 1 G, 2 R) of the pixel at EXR row y, column x: source row h - 1 - y, float 2 - c of the float4 */
RRT_FN uint32_t exr_load(const float* hdr, const ExrPlan& p, int y, int c, int x) {
    return exr_sample(p, exr_float_bits(hdr[((size_t)(p.h - 1 - y) * (size_t)p.w + (size_t)x) * 4 + (size_t)(2 - c)]));
}

/* the chunk that holds row y: its first row, its rows, its byte offset in the payload */
RRT_FN void exr_chunk_of(const ExrPlan& p, int y, int& y0, int& rows, size_t& offset) {
    y0 = y - y % p.lines;
    rows = p.h - y0 < p.lines ? p.h - y0 : p.lines;
    offset = (size_t)y0 * (size_t)p.w * 3u * (size_t)p.bps;
}

/* Step 3 for one sample v with predecessor q.  `first`: v is the chunk's sample 0 and q its LAST sample -- out[0] has no
 * predecessor, and the predecessor across the seam is the last byte of the first half.
 *   HALF:  lo[0] is out[s], hi[0] is out[n/2 + s].
 *   FLOAT: lo[0], lo[1] are out[2s], out[2s + 1] (bytes 0 and 2), hi[0], hi[1] are out[n/2 + 2s], out[n/2 + 2s + 1] (bytes 1 and 3). */
RRT_FN void exr_filter_sample(int type, uint32_t v, uint32_t q, bool first, uint8_t lo[2], uint8_t hi[2]) {
    if (type == RRT_EXR_HALF) {
        const uint32_t v0 = v & 255u, v1 = (v >> 8) & 255u, q0 = q & 255u, q1 = (q >> 8) & 255u;
        lo[0] = (uint8_t)(first ? v0 : v0 - q0 + 128u);
        hi[0] = (uint8_t)(v1 - (first ? q0 : q1) + 128u);
        lo[1] = hi[1] = 0;
    } else {
        const uint32_t v0 = v & 255u, v1 = (v >> 8) & 255u, v2 = (v >> 16) & 255u, v3 = v >> 24;
        const uint32_t q2 = (q >> 16) & 255u, q3 = q >> 24;
        lo[0] = (uint8_t)(first ? v0 : v0 - q2 + 128u);
        lo[1] = (uint8_t)(v2 - v0 + 128u);
        hi[0] = (uint8_t)(v1 - (first ? q2 : q3) + 128u);
        hi[1] = (uint8_t)(v3 - v1 + 128u);
    }
}

/* the predecessor of sample (y, c, x) in its chunk's order; for the chunk's sample 0, its last sample (first = true) */
RRT_FN uint32_t exr_load_pred(const float* hdr, const ExrPlan& p, int y, int c, int x, int y0, int rows, bool& first) {
    first = false;
    if (x > 0) return exr_load(hdr, p, y, c, x - 1);
    if (c > 0) return exr_load(hdr, p, y, c - 1, p.w - 1);
    if (y > y0) return exr_load(hdr, p, y - 1, 2, p.w - 1);
    first = true;
    return exr_load(hdr, p, y0 + rows - 1, 2, p.w - 1);
}

/* One sample, one byte per store: the narrow path and the host conversion */
RRT_FN void exr_put_sample(uint8_t* payload, const float* hdr, const ExrPlan& p, int y, int c, int x) {
    const uint32_t v = exr_load(hdr, p, y, c, x);
    if (p.compression == RRT_EXR_NONE) {
        uint8_t* dst = payload + (((size_t)y * 3u + (size_t)c) * (size_t)p.w + (size_t)x) * (size_t)p.bps;
        for (int b = 0; b < p.bps; ++b) dst[b] = (uint8_t)(v >> (8 * b));
        return;
    }
    int y0, rows;
    size_t offset;
    exr_chunk_of(p, y, y0, rows, offset);
    bool first;
    const uint32_t q = exr_load_pred(hdr, p, y, c, x, y0, rows, first);
    uint8_t lo[2], hi[2];
    exr_filter_sample(p.type, v, q, first, lo, hi);
    const size_t s = ((size_t)(y - y0) * 3u + (size_t)c) * (size_t)p.w + (size_t)x;      /* the sample's number in its chunk */
    const size_t per = (size_t)p.bps / 2u;                                               /* bytes of a sample in each half */
    uint8_t* a = payload + offset + s * per;
    uint8_t* b = a + (size_t)rows * (size_t)p.w * 3u * per;                             /* + n / 2 */
    a[0] = lo[0];
    b[0] = hi[0];
    if (per == 2) { a[1] = lo[1]; b[1] = hi[1]; }
}

/* ---- host only: the format's checks, the plan, the frame in host memory, the filter's inverse, the file header ---- */

static thread_local char g_exr_err[256] = "";

static inline int exr_refuse(const char* what) {
    snprintf(g_exr_err, sizeof(g_exr_err), "%s", what);
    return RRT_ERR_INVALID_ARGUMENT;
}

/* the value of a finite half's bits */
static inline float exr_half_value(uint32_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 1023u;
    float v = e == 0 ? (float)m * 5.9604644775390625e-8f /* 2^-24 */ : (float)(1024u + m) * 5.9604644775390625e-8f;
    for (uint32_t k = 1; k < e; ++k) v *= 2.0f;
    return (h & 0x8000u) ? -v : v;
}

static inline int exr_plan(const rrt_exr_format* f, int w, int h, ExrPlan& p) {
    g_exr_err[0] = 0;
    if (!f) return exr_refuse("fmt is NULL");
    if (f->struct_size != sizeof(rrt_exr_format)) return exr_refuse("fmt->struct_size is not sizeof(rrt_exr_format)");
    if (f->type != RRT_EXR_HALF && f->type != RRT_EXR_FLOAT) return exr_refuse("fmt->type: RRT_EXR_HALF (1) | RRT_EXR_FLOAT (2)");
    if (f->compression != RRT_EXR_NONE && f->compression != RRT_EXR_ZIPS && f->compression != RRT_EXR_ZIP)
        return exr_refuse("fmt->compression: RRT_EXR_NONE (0) | RRT_EXR_ZIPS (2) | RRT_EXR_ZIP (3)");
    const uint32_t mb = exr_float_bits(f->half_max);
    if (!(f->half_max > 0.0f) || mb >= 0x7f800000u) return exr_refuse("fmt->half_max: a finite positive half");
    const uint32_t mh = exr_half_bits(mb, 0x7bffu);
    if (mh == 0u || exr_half_value(mh) != f->half_max) return exr_refuse("fmt->half_max: a finite positive half");
    if (w < 1 || h < 1) return exr_refuse("width and height >= 1");
    p.w = w;
    p.h = h;
    p.type = f->type;
    p.compression = f->compression;
    p.lines = f->compression == RRT_EXR_ZIP ? 16 : 1;
    p.bps = f->type == RRT_EXR_HALF ? 2 : 4;
    p.max_half = mh;
    const uint64_t rows = (uint64_t)(h < p.lines ? h : p.lines);
    if (rows * (uint64_t)w * 3u * (uint64_t)p.bps >= ((uint64_t)1 << 31)) return exr_refuse("a chunk of 2^31 bytes or more");
    const int64_t chunks = ((int64_t)h + p.lines - 1) / p.lines;
    p.n_chunks = (int32_t)chunks;
    return RRT_OK;
}

static inline uint64_t exr_bytes(const ExrPlan& p) { return (uint64_t)p.w * (uint64_t)p.h * 3u * (uint64_t)p.bps; }

/* the wide path's rule: whole groups of kExrWidePixels along a row, both buffers on 16 bytes; then every row of every channel
 * starts on 16 bytes in the payload, in both halves of a filtered chunk */
static inline bool exr_wide_ok(const ExrPlan& p, size_t address_bits) { return p.w % kExrWidePixels == 0 && (address_bits & 15u) == 0; }

/* out[8] of rrt_exr_launch_geometry */
static inline void exr_geometry(const ExrPlan& p, size_t address_bits, int32_t out[8]) {
    const bool wide = exr_wide_ok(p, address_bits);
    const int64_t units = wide ? p.w / kExrWidePixels : (int64_t)p.w * 3;
    const int64_t gy = ((int64_t)p.h + kExrBlockY - 1) / kExrBlockY;
    out[0] = kExrBlockX * kExrBlockY;
    out[1] = kExrBlockX;
    out[2] = kExrBlockY;
    out[3] = wide ? kExrWidePixels : 1;
    out[4] = (int32_t)((units + kExrBlockX - 1) / kExrBlockX);
    out[5] = (int32_t)(gy < kExrMaxGridY ? gy : kExrMaxGridY);
    out[6] = wide ? 1 : 0;
    const int64_t per_pass = (int64_t)out[5] * kExrBlockY;
    out[7] = (int32_t)(((int64_t)p.h + per_pass - 1) / per_pass);
}

static inline bool exr_overlap(uintptr_t a, uint64_t a_bytes, uintptr_t b, uint64_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

static inline int exr_host(void* payload, const float* hdr, int w, int h, const rrt_exr_format* fmt) {
    ExrPlan p;
    const int rc = exr_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    if (!payload || !hdr) return exr_refuse("payload or hdr is NULL");
    if (exr_overlap((uintptr_t)payload, exr_bytes(p), (uintptr_t)hdr, (uint64_t)w * (uint64_t)h * 16u)) return exr_refuse("the payload overlaps the HDR plane");
    for (int y = 0; y < h; ++y)
        for (int c = 0; c < 3; ++c)
            for (int x = 0; x < w; ++x) exr_put_sample(static_cast<uint8_t*>(payload), hdr, p, y, c, x);
    return RRT_OK;
}

static inline int exr_unfilter(void* raw, const void* filtered, size_t n) {
    g_exr_err[0] = 0;
    if (!raw || !filtered) return exr_refuse("raw or filtered is NULL");
    if (n < 2 || (n & 1u) != 0 || n >= ((size_t)1 << 31)) return exr_refuse("n: even, 2 <= n < 2^31");
    if (exr_overlap((uintptr_t)raw, n, (uintptr_t)filtered, n)) return exr_refuse("raw overlaps filtered");
    const uint8_t* in = static_cast<const uint8_t*>(filtered);
    uint8_t* out = static_cast<uint8_t*>(raw);
    const size_t half = n / 2;
    uint32_t t = in[0];
    out[0] = (uint8_t)t;
    for (size_t j = 1; j < n; ++j) {
        t = (t + in[j] - 128u) & 255u;
        out[j < half ? 2 * j : 2 * (j - half) + 1] = (uint8_t)t;
    }
    return RRT_OK;
}

/* the header's bytes, appended to a buffer of `cap` bytes; `at` runs past cap when they do not fit (nothing is written beyond cap) */
struct ExrWriter {
    uint8_t* buf;
    size_t cap, at;
    void bytes(const void* src, size_t n) {
        if (at + n <= cap) memcpy(buf + at, src, n);
        at += n;
    }
    void u8(uint8_t v) { bytes(&v, 1); }
    void i32(int32_t v) { const uint32_t u = (uint32_t)v; const uint8_t b[4] = {(uint8_t)u, (uint8_t)(u >> 8), (uint8_t)(u >> 16), (uint8_t)(u >> 24)}; bytes(b, 4); }
    void f32(float v) { i32((int32_t)exr_float_bits(v)); }
    void text(const char* s) { bytes(s, strlen(s) + 1); }          /* with its NUL */
    void attribute(const char* name, const char* type, int32_t size) { text(name); text(type); i32(size); }
};

static const char kExrSoftware[] = "relativisticraytracer_amd";

static inline int exr_header(const rrt_exr_format* fmt, int w, int h, int fps_num, int fps_den, void* buf, size_t cap, size_t* len) {
    ExrPlan p;
    const int rc = exr_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    if (!buf || !len) return exr_refuse("buf or len is NULL");
    if (fps_num <= 0 || fps_den <= 0) return exr_refuse("fps_num and fps_den > 0");
    uint8_t tmp[1024];
    ExrWriter o = {tmp, sizeof(tmp), 0};
    const uint8_t magic[4] = {0x76, 0x2f, 0x31, 0x01};
    o.bytes(magic, 4);
    o.i32(2);                                           /* version 2, no flag bits: single part, scanlines, short names */
    o.attribute("channels", "chlist", 3 * 18 + 1);
    for (const char* name : {"B", "G", "R"}) {
        o.text(name);
        o.i32(p.type);                                  /* 1 HALF | 2 FLOAT */
        o.u8(0); o.u8(0); o.u8(0); o.u8(0);             /* pLinear, reserved */
        o.i32(1); o.i32(1);                             /* xSampling, ySampling */
    }
    o.u8(0);
    o.attribute("compression", "compression", 1);
    o.u8((uint8_t)p.compression);
    for (const char* name : {"dataWindow", "displayWindow"}) {
        o.attribute(name, "box2i", 16);
        o.i32(0); o.i32(0); o.i32(w - 1); o.i32(h - 1);
    }
    o.attribute("lineOrder", "lineOrder", 1);
    o.u8(0);                                            /* INCREASING_Y */
    o.attribute("pixelAspectRatio", "float", 4);
    o.f32(1.0f);
    o.attribute("screenWindowCenter", "v2f", 8);
    o.f32(0.0f); o.f32(0.0f);
    o.attribute("screenWindowWidth", "float", 4);
    o.f32(1.0f);
    o.attribute("chromaticities", "chromaticities", 32);
    for (float v : {0.64f, 0.33f, 0.30f, 0.60f, 0.15f, 0.06f, 0.3127f, 0.3290f}) o.f32(v);      /* BT.709 R, G, B; D65 */
    o.attribute("framesPerSecond", "rational", 8);
    o.i32(fps_num); o.i32(fps_den);
    o.attribute("software", "string", (int32_t)(sizeof(kExrSoftware) - 1));
    o.bytes(kExrSoftware, sizeof(kExrSoftware) - 1);
    o.u8(0);                                            /* end of the header */
    if (o.at > sizeof(tmp) || o.at > cap) return exr_refuse("cap is smaller than the header");
    memcpy(buf, tmp, o.at);
    *len = o.at;
    return RRT_OK;
}

#endif /* RRT_EXR_CORE_H */
