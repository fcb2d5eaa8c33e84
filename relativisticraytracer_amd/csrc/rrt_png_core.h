/*
 * rrt_png_core.h -- the definition of include/rrt_png.h as functions the host and the device share (RRT_FN, as rrt_yuv_core.h and
 * rrt_exr_core.h): plain C++ that g++ can include.  rrt_png.hip's narrow kernel and its *_host entry points, and
 * tests/png/png_exerciser.cpp, run this very source.
 *
 * png_row filters ONE row: it walks the row's pixels once per pass with the pixel to the left carried along, scores the five
 * candidates in a plain loop when the filter is adaptive, then emits the row one byte per store and sums it.  The wide kernel of
 * rrt_png.hip calls the same png_pixel / png_filtered / png_cost on bytes it staged in LDS.
 */
#ifndef RRT_PNG_CORE_H
#define RRT_PNG_CORE_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rrt_png.h"
#include "rrt_yuv_core.h"     /* yuv_q_from_hdr: the 16-bit samples are Y4M output's q_c, not a second definition; RRT_FN */

constexpr uint32_t kPngAdler = 65521u;
constexpr int kPngWideThreads = 256;                 /* the wide path's workgroup: four wavefronts over one band of rows */
constexpr int kPngNarrowThreads = 64;                /* the narrow path: a thread filters a row */
constexpr int kPngHaloPixels = 8;                    /* zero pixels staged to the left of a row: 24 | 48 bytes >= 15 + 1 + bpp */
constexpr int kPngBufSlack = 160;                    /* bytes of an LDS row buffer beyond its chunks: the halo, one pixel, the last 28-byte read */

/* What a launch needs of the format and the size, checked and computed once on the host (png_plan) and passed by value */
struct PngPlan {
    int32_t w, h;
    int32_t depth, bpp;       /* 8 | 16, 3 | 6 */
    int32_t filter;           /* 0 ... 4 | RRT_PNG_ADAPTIVE */
    uint32_t n;               /* raw bytes of a row: w * bpp */
    uint32_t stride;          /* 1 + n */
    int32_t chunks;           /* the most 16-byte chunks a row's span touches: ceil((15 + stride) / 16) */
    int32_t seg_chunks;       /* chunks staged at a time: min(chunks, RRT_PNG_SEGMENT_CHUNKS) */
};

/* the raw bytes of the pixel at PNG row r, column x: buffer row h - 1 - r */
template <bool HDR>
RRT_FN void png_pixel(const void* src, const PngPlan& p, int r, int x, uint8_t out[6]) {
    const size_t i = ((size_t)(p.h - 1 - r) * (size_t)p.w + (size_t)x) * 4u;
    if (HDR) {
        const float* f = static_cast<const float*>(src) + i;
        for (int c = 0; c < 3; ++c) {
            const int q = yuv_q_from_hdr(f[c]);
            out[2 * c] = (uint8_t)(q >> 8);
            out[2 * c + 1] = (uint8_t)(q & 255);
        }
    } else {
        const uint8_t* b = static_cast<const uint8_t*>(src) + i;
        out[0] = b[0]; out[1] = b[1]; out[2] = b[2];
        out[3] = out[4] = out[5] = 0;
    }
}

/* step 2: filter `type` of x with a (left), b (above), c (above-left), mod 256 */
RRT_FN uint32_t png_filtered(int type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
    uint32_t pred = 0u;
    if (type == RRT_PNG_SUB) pred = a;
    else if (type == RRT_PNG_UP) pred = b;
    else if (type == RRT_PNG_AVERAGE) pred = (a + b) >> 1;
    else if (type == RRT_PNG_PAETH) {
        const int pa = (int)b - (int)c, pb = (int)a - (int)c, pc = pa + pb;      /* p - a, p - b, p - c with p = a + b - c */
        const int da = pa < 0 ? -pa : pa, db = pb < 0 ? -pb : pb, dc = pc < 0 ? -pc : pc;
        pred = (da <= db && da <= dc) ? a : (db <= dc ? b : c);
    }
    return (x - pred) & 255u;
}

/* step 3: what a filtered byte adds to its candidate's score */
RRT_FN uint32_t png_cost(uint32_t v) { return v < 128u ? v : 256u - v; }

/* the smallest score, ties to the lowest type */
RRT_FN int png_choose(const uint64_t score[5]) {
    int best = 0;
    for (int t = 1; t < 5; ++t)
        if (score[t] < score[best]) best = t;
    return best;
}

/* Steps 2-5 for row r: `stride` bytes at payload + r * stride, two sums at sums + 2 r.  The narrow path and the host. */
template <bool HDR>
RRT_FN void png_row(uint8_t* payload, uint32_t* sums, const void* src, const PngPlan& p, int r) {
    int type = p.filter;
    uint8_t* dst = payload + (size_t)r * (size_t)p.stride;
    uint64_t s1 = 0, s2 = 0;
    for (int pass = type == RRT_PNG_ADAPTIVE ? 0 : 1; pass < 2; ++pass) {
        uint64_t score[5] = {0, 0, 0, 0, 0};
        uint8_t left[6] = {0, 0, 0, 0, 0, 0}, up_left[6] = {0, 0, 0, 0, 0, 0};
        for (int x = 0; x < p.w; ++x) {
            uint8_t cur[6], up[6] = {0, 0, 0, 0, 0, 0};
            png_pixel<HDR>(src, p, r, x, cur);
            if (r > 0) png_pixel<HDR>(src, p, r - 1, x, up);
            for (int j = 0; j < p.bpp; ++j) {
                if (pass == 0) {
                    for (int t = 0; t < 5; ++t) score[t] += png_cost(png_filtered(t, cur[j], left[j], up[j], up_left[j]));
                } else {
                    const uint32_t i = 1u + (uint32_t)x * (uint32_t)p.bpp + (uint32_t)j;        /* the byte's place in the row */
                    const uint32_t d = png_filtered(type, cur[j], left[j], up[j], up_left[j]);
                    dst[i] = (uint8_t)d;
                    s1 += d;
                    s2 += (uint64_t)((p.stride - i) % kPngAdler) * d;
                }
                left[j] = cur[j];
                up_left[j] = up[j];
            }
        }
        if (pass == 0) type = png_choose(score);
    }
    dst[0] = (uint8_t)type;
    s1 += (uint32_t)type;
    s2 += (uint64_t)(p.stride % kPngAdler) * (uint32_t)type;
    sums[2 * (size_t)r] = (uint32_t)(s1 % kPngAdler);
    sums[2 * (size_t)r + 1] = (uint32_t)(s2 % kPngAdler);
}

/* ---- host only: the format's checks, the plan, the frame in host memory, the inverse, the Adler fold, the file header ---- */

static thread_local char g_png_err[256] = "";

static inline int png_refuse(const char* what) {
    snprintf(g_png_err, sizeof(g_png_err), "%s", what);
    return RRT_ERR_INVALID_ARGUMENT;
}

static inline int png_plan(const rrt_png_format* f, int w, int h, PngPlan& p) {
    g_png_err[0] = 0;
    if (!f) return png_refuse("fmt is NULL");
    if (f->struct_size != sizeof(rrt_png_format)) return png_refuse("fmt->struct_size is not sizeof(rrt_png_format)");
    if (f->depth != 8 && f->depth != 16) return png_refuse("fmt->depth: 8 | 16");
    if (f->filter < RRT_PNG_NONE || f->filter > RRT_PNG_ADAPTIVE) return png_refuse("fmt->filter: RRT_PNG_NONE (0) ... RRT_PNG_PAETH (4) | RRT_PNG_ADAPTIVE (5)");
    if (w < 1 || h < 1) return png_refuse("width and height >= 1");
    if ((uint64_t)w * (uint64_t)h >= ((uint64_t)1 << 31)) return png_refuse("width * height is 2^31 or more");
    p.w = w;
    p.h = h;
    p.depth = f->depth;
    p.bpp = f->depth == 8 ? 3 : 6;
    p.filter = f->filter;
    const uint64_t stride = 1u + (uint64_t)w * (uint64_t)p.bpp;
    if (stride * (uint64_t)h >= ((uint64_t)1 << 32)) return png_refuse("a payload of 2^32 bytes or more");
    p.n = (uint32_t)(stride - 1u);
    p.stride = (uint32_t)stride;
    p.chunks = (int32_t)((stride + 15u + 15u) / 16u);
    p.seg_chunks = p.chunks < RRT_PNG_SEGMENT_CHUNKS ? p.chunks : RRT_PNG_SEGMENT_CHUNKS;
    return RRT_OK;
}

static inline uint64_t png_bytes(const PngPlan& p) { return (uint64_t)p.stride * (uint64_t)p.h; }
static inline uint64_t png_input_bytes(const PngPlan& p) { return (uint64_t)p.w * (uint64_t)p.h * (p.depth == 8 ? 4u : 16u); }

/* bytes of one LDS row buffer, and of the launch's dynamic LDS: two of them */
static inline uint32_t png_buf_bytes(const PngPlan& p) { return 16u * (uint32_t)p.seg_chunks + (uint32_t)kPngBufSlack; }

static inline bool png_wide_ok(size_t address_bits) { return (address_bits & 15u) == 0; }

/* step 6's cut */
static inline void png_slices(const PngPlan& p, int32_t& rows, int32_t& n) {
    const uint64_t r = ((uint64_t)RRT_PNG_SLICE_BYTES + p.stride - 1u) / p.stride;
    rows = (int32_t)(r < (uint64_t)p.h ? r : (uint64_t)p.h);
    n = (int32_t)(((int64_t)p.h + rows - 1) / rows);
}

/* out[8] of rrt_png_launch_geometry */
static inline void png_geometry(const PngPlan& p, size_t address_bits, int32_t out[8]) {
    const bool wide = png_wide_ok(address_bits);
    const int per = wide ? RRT_PNG_BAND_ROWS : kPngNarrowThreads;
    out[0] = wide ? kPngWideThreads : kPngNarrowThreads;
    out[1] = per;
    out[2] = (int32_t)(((int64_t)p.h + per - 1) / per);
    out[3] = p.chunks;
    out[4] = (p.chunks + p.seg_chunks - 1) / p.seg_chunks;
    out[5] = wide ? (int32_t)(2u * png_buf_bytes(p)) : 0;
    out[6] = wide ? 1 : 0;
    out[7] = p.seg_chunks;
}

static inline bool png_overlap(uintptr_t a, uint64_t a_bytes, uintptr_t b, uint64_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

/* what every conversion refuses of its buffers, host or device; `depth`: the entry point's */
static inline int png_buffers(const void* payload, const uint32_t* sums, const void* src, const PngPlan& p, int depth) {
    if (!payload || !sums || !src) return png_refuse("payload, row_sums or the input is NULL");
    if (p.depth != depth) return png_refuse(depth == 8 ? "fmt->depth: 8 from an RGBA8 frame" : "fmt->depth: 16 from the HDR plane");
    const uintptr_t out = (uintptr_t)payload, tab = (uintptr_t)sums, in = (uintptr_t)src;
    if ((tab & 3u) != 0) return png_refuse("row_sums is not 4-byte aligned");
    if (depth == 16 && (in & 3u) != 0) return png_refuse("the HDR plane is not 4-byte aligned");
    if (png_overlap(out, png_bytes(p), in, png_input_bytes(p))) return png_refuse("the payload overlaps the input");
    if (png_overlap(tab, 8u * (uint64_t)p.h, in, png_input_bytes(p))) return png_refuse("row_sums overlaps the input");
    if (png_overlap(tab, 8u * (uint64_t)p.h, out, png_bytes(p))) return png_refuse("row_sums overlaps the payload");
    return RRT_OK;
}

template <bool HDR>
static inline int png_host(void* payload, uint32_t* sums, const void* src, int w, int h, const rrt_png_format* fmt) {
    PngPlan p;
    int rc = png_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    rc = png_buffers(payload, sums, src, p, HDR ? 16 : 8);
    if (rc != RRT_OK) return rc;
    for (int r = 0; r < h; ++r) png_row<HDR>(static_cast<uint8_t*>(payload), sums, src, p, r);
    return RRT_OK;
}

static inline int png_unfilter(void* raw, const void* payload, int w, int h, const rrt_png_format* fmt) {
    PngPlan p;
    const int rc = png_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    if (!raw || !payload) return png_refuse("raw or payload is NULL");
    if (png_overlap((uintptr_t)raw, (uint64_t)p.n * (uint64_t)h, (uintptr_t)payload, png_bytes(p))) return png_refuse("raw overlaps the payload");
    const uint8_t* in = static_cast<const uint8_t*>(payload);
    uint8_t* out = static_cast<uint8_t*>(raw);
    for (int r = 0; r < h; ++r)
        if (in[(size_t)r * p.stride] > RRT_PNG_PAETH) return png_refuse("a row's filter type is above 4");
    const uint32_t bpp = (uint32_t)p.bpp;
    for (int r = 0; r < h; ++r) {
        const uint8_t* row = in + (size_t)r * p.stride;
        uint8_t* cur = out + (size_t)r * p.n;
        const uint8_t* up = r > 0 ? cur - p.n : nullptr;
        for (uint32_t i = 0; i < p.n; ++i) {
            const uint32_t a = i >= bpp ? cur[i - bpp] : 0u, b = up ? up[i] : 0u, c = (up && i >= bpp) ? up[i - bpp] : 0u;
            cur[i] = (uint8_t)((uint32_t)row[1 + i] - png_filtered(row[0], 0u, a, b, c));        /* x = v + pred */
        }
    }
    return RRT_OK;
}

static inline int png_adler32(const uint32_t* sums, int w, int h, const rrt_png_format* fmt, uint32_t* adler) {
    PngPlan p;
    const int rc = png_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    if (!sums || !adler) return png_refuse("row_sums or adler is NULL");
    uint64_t A = 1, B = 0;
    for (int r = 0; r < h; ++r) {
        B = (B + sums[2 * (size_t)r + 1] % kPngAdler + (uint64_t)(p.stride % kPngAdler) * A) % kPngAdler;
        A = (A + sums[2 * (size_t)r] % kPngAdler) % kPngAdler;
    }
    *adler = (uint32_t)(B << 16 | A);
    return RRT_OK;
}

/* CRC-32 of the chunks (the PNG specification's, polynomial 0xedb88320), bit by bit: the header is a hundred bytes */
static inline uint32_t png_crc(const uint8_t* data, size_t n) {
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= data[i];
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return c ^ 0xffffffffu;
}

/* chunks appended to a buffer of `cap` bytes; `at` runs past cap when they do not fit (nothing is written beyond cap) */
struct PngWriter {
    uint8_t* buf;
    size_t cap, at;
    void bytes(const void* src, size_t n) {
        if (at + n <= cap) memcpy(buf + at, src, n);
        at += n;
    }
    void u32(uint32_t v) { const uint8_t b[4] = {(uint8_t)(v >> 24), (uint8_t)(v >> 16), (uint8_t)(v >> 8), (uint8_t)v}; bytes(b, 4); }
    void chunk(const char* type, const uint8_t* data, uint32_t n) {
        uint8_t tmp[128];
        memcpy(tmp, type, 4);
        memcpy(tmp + 4, data, n);
        u32(n);
        bytes(tmp, 4u + n);
        u32(png_crc(tmp, 4u + n));
    }
};

static const char kPngSoftware[] = "relativisticraytracer_amd";

static inline int png_header(const rrt_png_format* fmt, int w, int h, void* buf, size_t cap, size_t* len) {
    PngPlan p;
    const int rc = png_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    if (!buf || !len) return png_refuse("buf or len is NULL");
    uint8_t tmp[256];
    PngWriter o = {tmp, sizeof(tmp), 0};
    const uint8_t signature[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    o.bytes(signature, 8);
    const uint32_t uw = (uint32_t)w, uh = (uint32_t)h;
    const uint8_t ihdr[13] = {(uint8_t)(uw >> 24), (uint8_t)(uw >> 16), (uint8_t)(uw >> 8), (uint8_t)uw,
                              (uint8_t)(uh >> 24), (uint8_t)(uh >> 16), (uint8_t)(uh >> 8), (uint8_t)uh,
                              (uint8_t)p.depth, 2, 0, 0, 0};        /* colour type 2; deflate, adaptive filtering, no interlace */
    o.chunk("IHDR", ihdr, 13);
    const uint8_t intent[1] = {0};                      /* perceptual */
    o.chunk("sRGB", intent, 1);
    uint8_t text[64];
    memcpy(text, "Software", 9);                        /* the keyword and its NUL */
    memcpy(text + 9, kPngSoftware, sizeof(kPngSoftware) - 1);
    o.chunk("tEXt", text, (uint32_t)(9 + sizeof(kPngSoftware) - 1));
    if (o.at > sizeof(tmp) || o.at > cap) return png_refuse("cap is smaller than the header");
    memcpy(buf, tmp, o.at);
    *len = o.at;
    return RRT_OK;
}

#endif
