/*
 * rrt_exr_core.h -- the definition of include/rrt_exr.h as functions the host and the device share (RRT_FN, as rrt_yuv_core.h):
 * plain C++ that g++ can include.  rrt_exr.hip's kernels and its *_host entry points, and tests/exr/exr_exerciser.cpp, run this
 * very source.
 *
 * A chunk's samples are numbered s = (row_in_chunk * 3 + channel) * width + x, channel 0 = B, 1 = G, 2 = R: the order of its raw
 * bytes.  exr_put_sample packs ONE sample -- the narrow path, at any size and alignment; the wide kernel of rrt_exr.hip calls the
 * same exr_sample / exr_filter_sample with vector loads and stores.
 *
 * The second half of the file is the same for data layers (any channel list over any sources: exr_layer_*, exr_layers_*), and
 * tests/exr/exr_layers_exerciser.cpp runs it.  The B, G, R functions above are not expressed through it: the identity between the
 * two is a test (tests/test_exr_layers_host.py), and the dedicated kernels keep their constants.
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

/* ==== data layers (include/rrt_exr.h, the second block comment): any channel list over any sources ========================== */

/* What a layers launch needs, checked and computed once on the host (exr_layers_plan) and passed by value.  Channel c's samples lie
 * ch_pre[c] * w bytes into each raw scanline: ch_pre is the sum of the sample sizes of the channels in front of it. */
struct ExrLayersPlan {
    int32_t w, h;
    int32_t compression, lines, n_chunks;
    int32_t n_src, n_ch;
    int32_t sum_bps;                                  /* bytes of one pixel over all channels: even */
    int32_t store8;                                   /* the wide path stores filtered 4-byte channels 8 bytes at a time (rrt_exr_layers_launch_geometry) */
    uint32_t max_half;
    const uint32_t* src[RRT_EXR_MAX_SOURCES];
    int32_t src_words[RRT_EXR_MAX_SOURCES], src_kind[RRT_EXR_MAX_SOURCES], src_bottom_up[RRT_EXR_MAX_SOURCES];
    int32_t ch_type[RRT_EXR_MAX_CHANNELS], ch_src[RRT_EXR_MAX_CHANNELS], ch_word[RRT_EXR_MAX_CHANNELS], ch_pre[RRT_EXR_MAX_CHANNELS];
};

RRT_FN int exr_layer_bps(int type) { return type == RRT_EXR_HALF ? 2 : 4; }

/* Step 1': the stored bits of one source word u.  F32 -> UINT never arrives here: exr_layers_plan refuses it. */
RRT_FN uint32_t exr_layer_sample(int kind, int type, uint32_t u, uint32_t max_half) {
    if (kind == RRT_EXR_SRC_I32) {
        const int32_t v = (int32_t)u;
        if (type == RRT_EXR_UINT) return v < 0 ? 0u : u;
        u = exr_float_bits((float)v);                 /* round to nearest even */
    }
    return type == RRT_EXR_HALF ? exr_half_bits(u, max_half) : u;
}

/* the last two bytes of a stored sample: what step 3 subtracts from the sample behind it, whatever either's type */
RRT_FN uint32_t exr_layer_tail(int type, uint32_t v) { return type == RRT_EXR_HALF ? v & 0xffffu : v >> 16; }

/* the source word behind channel c of the pixel at EXR row y, column x */
RRT_FN uint32_t exr_layer_word(const ExrLayersPlan& p, int y, int c, int x) {
    const int s = p.ch_src[c];
    const size_t row = (size_t)(p.src_bottom_up[s] ? p.h - 1 - y : y);
    return p.src[s][(row * (size_t)p.w + (size_t)x) * (size_t)p.src_words[s] + (size_t)p.ch_word[c]];
}

/* ... and its stored sample */
RRT_FN uint32_t exr_layer_load(const ExrLayersPlan& p, int y, int c, int x) {
    return exr_layer_sample(p.src_kind[p.ch_src[c]], p.ch_type[c], exr_layer_word(p, y, c, x), p.max_half);
}

/* the chunk that holds row y, as exr_chunk_of */
RRT_FN void exr_layer_chunk_of(const ExrLayersPlan& p, int y, int& y0, int& rows, size_t& offset) {
    y0 = y - y % p.lines;
    rows = p.h - y0 < p.lines ? p.h - y0 : p.lines;
    offset = (size_t)y0 * (size_t)p.w * (size_t)p.sum_bps;
}

/* exr_filter_sample for any pair of types: v is a sample of `bps` bytes, t the TAIL of its predecessor (t & 255 the last byte at
 * an even offset, t >> 8 the last at an odd one).  `first`: v is the chunk's sample 0 and t the tail of its LAST sample.  lo: the
 * sample's bytes in the chunk's first half, one (2-byte samples) or two, the earlier in bits 0-7; hi: those in the second half. */
RRT_FN void exr_layer_filter_sample(int bps, uint32_t v, uint32_t t, bool first, uint32_t& lo, uint32_t& hi) {
    const uint32_t v0 = v & 255u, v1 = (v >> 8) & 255u, te = t & 255u, to = (t >> 8) & 255u;
    lo = (first ? v0 : v0 - te + 128u) & 255u;
    hi = (v1 - (first ? te : to) + 128u) & 255u;
    if (bps == 4) {
        const uint32_t v2 = (v >> 16) & 255u, v3 = v >> 24;
        lo |= ((v2 - v0 + 128u) & 255u) << 8;
        hi |= ((v3 - v1 + 128u) & 255u) << 8;
    }
}

/* exr_load_pred for any channel list -- where the predecessor of sample (y, c, x) in its chunk's order lies: the sample to the
 * left; at a row's start the previous channel's last sample; for channel 0 the last channel's of the row above; for the chunk's
 * sample 0, its last sample (first = true) */
RRT_FN void exr_layer_pred_of(const ExrLayersPlan& p, int y, int c, int x, int y0, int rows, int& py, int& pc, int& px, bool& first) {
    first = false;
    py = y;
    pc = c;
    px = x - 1;
    if (x == 0) {
        px = p.w - 1;
        pc = c - 1;
        if (c == 0) {
            pc = p.n_ch - 1;
            py = y - 1;
            if (y == y0) { first = true; py = y0 + rows - 1; }
        }
    }
}

RRT_FN uint32_t exr_layer_pred_tail(const ExrLayersPlan& p, int y, int c, int x, int y0, int rows, bool& first) {
    int py, pc, px;
    exr_layer_pred_of(p, y, c, x, y0, rows, py, pc, px, first);
    return exr_layer_tail(p.ch_type[pc], exr_layer_load(p, py, pc, px));
}

/* One sample, one byte per store: the narrow path and the host conversion */
RRT_FN void exr_layer_put_sample(uint8_t* payload, const ExrLayersPlan& p, int y, int c, int x) {
    const uint32_t v = exr_layer_load(p, y, c, x);
    const int bps = exr_layer_bps(p.ch_type[c]);
    if (p.compression == RRT_EXR_NONE) {
        uint8_t* dst = payload + ((size_t)y * (size_t)p.sum_bps + (size_t)p.ch_pre[c]) * (size_t)p.w + (size_t)x * (size_t)bps;
        for (int b = 0; b < bps; ++b) dst[b] = (uint8_t)(v >> (8 * b));
        return;
    }
    int y0, rows;
    size_t offset;
    exr_layer_chunk_of(p, y, y0, rows, offset);
    bool first;
    const uint32_t t = exr_layer_pred_tail(p, y, c, x, y0, rows, first);
    uint32_t lo, hi;
    exr_layer_filter_sample(bps, v, t, first, lo, hi);
    const size_t per = (size_t)bps / 2u;                                      /* bytes of the sample in each half */
    uint8_t* a = payload + offset + ((size_t)(y - y0) * (size_t)p.sum_bps + (size_t)p.ch_pre[c]) / 2u * (size_t)p.w + (size_t)x * per;
    uint8_t* b = a + (size_t)rows * (size_t)p.w * (size_t)p.sum_bps / 2u;     /* + n / 2 */
    a[0] = (uint8_t)lo;
    b[0] = (uint8_t)hi;
    if (per == 2) { a[1] = (uint8_t)(lo >> 8); b[1] = (uint8_t)(hi >> 8); }
}

/* ---- host only ---- */

static inline bool exr_layer_name_ok(const char* name) {
    size_t n = 0;
    while (n < 32 && name[n]) ++n;
    if (n < 1 || n > 31 || name[0] == '.' || name[n - 1] == '.') return false;
    for (size_t i = 0; i < n; ++i) {
        const char ch = name[i];
        if (!((ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z') || (ch >= '0' && ch <= '9') || ch == '_' || ch == '.')) return false;
    }
    return true;
}

/* the checks every layers function makes (the sources' addresses apart) and the plan */
static inline int exr_layers_plan(const rrt_exr_layers* L, int w, int h, ExrLayersPlan& p) {
    g_exr_err[0] = 0;
    if (!L) return exr_refuse("layers is NULL");
    if (L->struct_size != sizeof(rrt_exr_layers)) return exr_refuse("layers->struct_size is not sizeof(rrt_exr_layers)");
    rrt_exr_format f = {(uint32_t)sizeof(rrt_exr_format), RRT_EXR_FLOAT, L->compression, L->half_max};
    ExrPlan q;
    const int rc = exr_plan(&f, 1, 1, q);             /* the compression and half_max rules, in exr_plan's words */
    if (rc != RRT_OK) return rc;
    if (w < 1 || h < 1) return exr_refuse("width and height >= 1");
    if (L->n_sources < 1 || L->n_sources > RRT_EXR_MAX_SOURCES) return exr_refuse("layers->n_sources: 1 ... 8");
    if (L->n_channels < 1 || L->n_channels > RRT_EXR_MAX_CHANNELS) return exr_refuse("layers->n_channels: 1 ... 16");
    p = ExrLayersPlan();
    p.w = w;
    p.h = h;
    p.compression = L->compression;
    p.lines = q.lines;
    p.max_half = q.max_half;
    p.n_src = L->n_sources;
    p.n_ch = L->n_channels;
    for (int s = 0; s < p.n_src; ++s) {
        const rrt_exr_source& src = L->sources[s];
        if (src.words != 1 && src.words != 3 && src.words != 4) return exr_refuse("a source's words: 1 | 3 | 4");
        if (src.kind != RRT_EXR_SRC_F32 && src.kind != RRT_EXR_SRC_I32) return exr_refuse("a source's kind: RRT_EXR_SRC_F32 (0) | RRT_EXR_SRC_I32 (1)");
        p.src[s] = static_cast<const uint32_t*>(src.d_data);
        p.src_words[s] = src.words;
        p.src_kind[s] = src.kind;
        p.src_bottom_up[s] = src.bottom_up != 0;
    }
    int halves = 0, fours = 0;
    for (int c = 0; c < p.n_ch; ++c) {
        const rrt_exr_channel& ch = L->channels[c];
        if (!exr_layer_name_ok(ch.name)) return exr_refuse("a channel's name: 1 ... 31 bytes of [A-Za-z0-9_.], no '.' at either end");
        if (c > 0 && strcmp(L->channels[c - 1].name, ch.name) >= 0) {      /* the names are ASCII: strcmp's order is the unsigned bytes' */
            snprintf(g_exr_err, sizeof(g_exr_err), "channel names must ascend strictly: \"%s\" is followed by \"%s\"", L->channels[c - 1].name, ch.name);
            return RRT_ERR_INVALID_ARGUMENT;
        }
        if (ch.type != RRT_EXR_UINT && ch.type != RRT_EXR_HALF && ch.type != RRT_EXR_FLOAT)
            return exr_refuse("a channel's type: RRT_EXR_UINT (0) | RRT_EXR_HALF (1) | RRT_EXR_FLOAT (2)");
        if (ch.source < 0 || ch.source >= p.n_src) return exr_refuse("a channel's source: an index in [0, n_sources)");
        if (ch.word < 0 || ch.word >= p.src_words[ch.source]) return exr_refuse("a channel's word: in [0, words) of its source");
        if (ch.type == RRT_EXR_UINT && p.src_kind[ch.source] == RRT_EXR_SRC_F32) return exr_refuse("an F32 source is not stored as UINT");
        p.ch_type[c] = ch.type;
        p.ch_src[c] = ch.source;
        p.ch_word[c] = ch.word;
        p.ch_pre[c] = p.sum_bps;
        p.sum_bps += exr_layer_bps(ch.type);
        ++(ch.type == RRT_EXR_HALF ? halves : fours);
    }
    const uint64_t rows = (uint64_t)(h < p.lines ? h : p.lines);
    if (rows * (uint64_t)w * (uint64_t)p.sum_bps >= ((uint64_t)1 << 31)) return exr_refuse("a chunk of 2^31 bytes or more");
    p.n_chunks = (int32_t)(((int64_t)h + p.lines - 1) / p.lines);
    p.store8 = p.compression != RRT_EXR_NONE && halves > 0 && fours > 0 && w % 16 == 8;
    return RRT_OK;
}

static inline uint64_t exr_layers_bytes(const ExrLayersPlan& p) { return (uint64_t)p.w * (uint64_t)p.h * (uint64_t)p.sum_bps; }

/* out[8] of rrt_exr_layers_launch_geometry */
static inline void exr_layers_geometry(const ExrLayersPlan& p, size_t address_bits, int32_t out[8]) {
    const bool wide = p.w % kExrWidePixels == 0 && (address_bits & 15u) == 0;
    const int64_t units = wide ? p.w / kExrWidePixels : (int64_t)p.w * p.n_ch;
    const int64_t gy = ((int64_t)p.h + kExrBlockY - 1) / kExrBlockY;
    out[0] = kExrBlockX * kExrBlockY;
    out[1] = kExrBlockX;
    out[2] = kExrBlockY;
    out[3] = wide ? kExrWidePixels : 1;
    out[4] = (int32_t)((units + kExrBlockX - 1) / kExrBlockX);
    out[5] = (int32_t)(gy < kExrMaxGridY ? gy : kExrMaxGridY);
    out[6] = !wide ? 0 : p.store8 ? 2 : 1;
    const int64_t per_pass = (int64_t)out[5] * kExrBlockY;
    out[7] = (int32_t)(((int64_t)p.h + per_pass - 1) / per_pass);
}

/* NULL, alignment and overlap of the payload and every source: what the launch and the host conversion check alike */
static inline int exr_layers_buffers(const void* payload, const ExrLayersPlan& p, size_t& address_bits) {
    if (!payload) return exr_refuse("payload is NULL");
    address_bits = (size_t)(uintptr_t)payload;
    for (int s = 0; s < p.n_src; ++s) {
        const uintptr_t in = (uintptr_t)p.src[s];
        if (!in) return exr_refuse("a source's d_data is NULL");
        if ((in & 3u) != 0) return exr_refuse("a source's d_data is not 4-byte aligned");
        if (exr_overlap((uintptr_t)payload, exr_layers_bytes(p), in, (uint64_t)p.w * (uint64_t)p.h * 4u * (uint64_t)p.src_words[s]))
            return exr_refuse("the payload overlaps a source");
        address_bits |= (size_t)in;
    }
    return RRT_OK;
}

static inline int exr_layers_host(void* payload, const rrt_exr_layers* L, int w, int h) {
    ExrLayersPlan p;
    int rc = exr_layers_plan(L, w, h, p);
    if (rc != RRT_OK) return rc;
    size_t bits;
    rc = exr_layers_buffers(payload, p, bits);
    if (rc != RRT_OK) return rc;
    for (int y = 0; y < h; ++y)
        for (int c = 0; c < p.n_ch; ++c)
            for (int x = 0; x < w; ++x) exr_layer_put_sample(static_cast<uint8_t*>(payload), p, y, c, x);
    return RRT_OK;
}

/* exr_header's attributes, in its order, around the layers' channel list */
static inline int exr_layers_header(const rrt_exr_layers* L, int w, int h, int fps_num, int fps_den, void* buf, size_t cap, size_t* len) {
    ExrLayersPlan p;
    const int rc = exr_layers_plan(L, w, h, p);
    if (rc != RRT_OK) return rc;
    if (!buf || !len) return exr_refuse("buf or len is NULL");
    if (fps_num <= 0 || fps_den <= 0) return exr_refuse("fps_num and fps_den > 0");
    uint8_t tmp[2048];
    ExrWriter o = {tmp, sizeof(tmp), 0};
    const uint8_t magic[4] = {0x76, 0x2f, 0x31, 0x01};
    o.bytes(magic, 4);
    o.i32(2);
    int32_t list = 1;
    for (int c = 0; c < p.n_ch; ++c) list += (int32_t)strlen(L->channels[c].name) + 1 + 16;
    o.attribute("channels", "chlist", list);
    for (int c = 0; c < p.n_ch; ++c) {
        o.text(L->channels[c].name);
        o.i32(p.ch_type[c]);
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
    o.u8(0);
    o.attribute("pixelAspectRatio", "float", 4);
    o.f32(1.0f);
    o.attribute("screenWindowCenter", "v2f", 8);
    o.f32(0.0f); o.f32(0.0f);
    o.attribute("screenWindowWidth", "float", 4);
    o.f32(1.0f);
    o.attribute("chromaticities", "chromaticities", 32);
    for (float v : {0.64f, 0.33f, 0.30f, 0.60f, 0.15f, 0.06f, 0.3127f, 0.3290f}) o.f32(v);
    o.attribute("framesPerSecond", "rational", 8);
    o.i32(fps_num); o.i32(fps_den);
    o.attribute("software", "string", (int32_t)(sizeof(kExrSoftware) - 1));
    o.bytes(kExrSoftware, sizeof(kExrSoftware) - 1);
    o.u8(0);
    if (o.at > sizeof(tmp) || o.at > cap) return exr_refuse("cap is smaller than the header");
    memcpy(buf, tmp, o.at);
    *len = o.at;
    return RRT_OK;
}

#endif /* RRT_EXR_CORE_H */
