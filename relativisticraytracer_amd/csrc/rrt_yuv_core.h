/*
 * rrt_yuv_core.h -- the definition of include/rrt_yuv.h as functions the host and the device share (RRT_FN, like rrt_exposure.h's
 * first part): plain C++ that g++ can include.  rrt_yuv.hip's kernels and its *_host entry points, and
 * tests/yuv/yuv_exerciser.cpp, run this very source.
 *
 * A frame is cut into strips of kYuvStripW x kYuvStripH pixels (display coordinates), numbered row-major.  A strip produces its
 * own chroma from the pixels it loaded: no second pass.  yuv_strip_narrow converts one strip with one sample per load and store
 * and works at any size and alignment; the wide kernel of rrt_yuv.hip calls the same yuv_q_* / yuv_code with vector accesses.
 */
#ifndef RRT_YUV_CORE_H
#define RRT_YUV_CORE_H

#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/rrt_yuv.h"
#include "rrt_math.h"

/* RRT_FN for a member function (RRT_FN itself says `static`) */
#if defined(__HIPCC__)
#define RRT_YUV_MEMBER __host__ __device__ __forceinline__
#else
#define RRT_YUV_MEMBER inline __attribute__((always_inline))
#endif

constexpr int kYuvStripW = 8, kYuvStripH = 2;
constexpr float kYuvExposure = 0.8f;          /* == kExposure, csrc/rrt_device.h:98 */

/* What a conversion needs of the format and the size, computed once on the host (yuv_plan below) and passed to the kernels by value */
struct YuvPlan {
    int64_t coef[9];          /* rows Y, Cb, Cr; columns R, G, B */
    int32_t off[3];
    int32_t bits, chroma;     /* 8 | 10, 420 | 444 */
    int32_t w, h, cw, ch;     /* the frame, the chroma planes */
    int32_t strips_x, strips_y;
    uint64_t plane[3];        /* byte offsets of Y, Cb, Cr */
};

RRT_FN int yuv_q_from_byte(uint32_t b) { return (int)(b * 257u); }

/* tone_map of csrc/rrt_kernels.h:243, one channel: 1.0f - rrt_expf(-H * kExposure) */
RRT_FN float yuv_tone(float hdr) { return 1.0f - rrt_expf(-hdr * kYuvExposure); }

/* NaN compares false: 0.  t <= 1, so the product is at most 65535.0f and the cast is defined. */
RRT_FN int yuv_q_from_hdr(float hdr) {
    const float t = yuv_tone(hdr);
    if (!(t > 0.0f)) return 0;
    const int q = (int)(t * 65535.0f);
    return q < 65535 ? q : 65535;
}

/* row `row` (0: Y, 1: Cb, 2: Cr) of a sum of 2^n pixels' q */
RRT_FN int yuv_code(const YuvPlan& p, int row, int n, int64_t sr, int64_t sg, int64_t sb) {
    const int64_t* c = p.coef + 3 * row;
    const int64_t v = (c[0] * sr + c[1] * sg + c[2] * sb + ((int64_t)p.off[row] << (30 + n)) + ((int64_t)1 << (29 + n))) >> (30 + n);
    const int64_t top = ((int64_t)1 << p.bits) - 1;
    return (int)(v < 0 ? 0 : (v > top ? top : v));
}

/* q of the pixel at display (col, row): buffer row h - 1 - row */
template <bool HDR>
RRT_FN void yuv_load_q(const void* src, int w, int h, int col, int row, int q[3]) {
    const size_t i = (size_t)(h - 1 - row) * (size_t)w + (size_t)col;
    if (HDR) {
        const float* f = static_cast<const float*>(src) + 4 * i;
        q[0] = yuv_q_from_hdr(f[0]); q[1] = yuv_q_from_hdr(f[1]); q[2] = yuv_q_from_hdr(f[2]);
    } else {
        const uint8_t* b = static_cast<const uint8_t*>(src) + 4 * i;
        q[0] = yuv_q_from_byte(b[0]); q[1] = yuv_q_from_byte(b[1]); q[2] = yuv_q_from_byte(b[2]);
    }
}

/* sample `i` of the plane at `base`: one byte, or two little-endian */
RRT_FN void yuv_put(uint8_t* base, size_t i, int bits, int code) {
    if (bits == 8) {
        base[i] = (uint8_t)code;
    } else {
        base[2 * i] = (uint8_t)(code & 255);
        base[2 * i + 1] = (uint8_t)(code >> 8);
    }
}

/* Strip (sx, sy), one sample per store.  Columns and rows past the frame's edge are the edge's: a 4:2:0 sum at an odd edge counts
 * the last column or row twice, as the definition says; nothing past the edge is stored.  `load(col, row, real, q)` gives a
 * pixel's sixteen-bit components: the SDR inputs through YuvNarrowLoad below, the HDR10 leg through rrt_hdr10_core.h's. */
template <class LOAD>
RRT_FN void yuv_strip_narrow_with(uint8_t* yuv, const YuvPlan& p, int sx, int sy, const LOAD& load) {
    const int x0 = sx * kYuvStripW, r0 = sy * kYuvStripH;
    int q[kYuvStripH][kYuvStripW][3];
    for (int j = 0; j < kYuvStripH; ++j)
        for (int i = 0; i < kYuvStripW; ++i) {
            const bool real = x0 + i < p.w && r0 + j < p.h;       /* false: the edge's pixel again, for a 4:2:0 sum */
            const int col = x0 + i < p.w ? x0 + i : p.w - 1, row = r0 + j < p.h ? r0 + j : p.h - 1;
            load(col, row, real, q[j][i]);
        }
    for (int j = 0; j < kYuvStripH && r0 + j < p.h; ++j)
        for (int i = 0; i < kYuvStripW && x0 + i < p.w; ++i) {
            const size_t at = (size_t)(r0 + j) * (size_t)p.w + (size_t)(x0 + i);
            yuv_put(yuv + p.plane[0], at, p.bits, yuv_code(p, 0, 0, q[j][i][0], q[j][i][1], q[j][i][2]));
            if (p.chroma == 444) {
                yuv_put(yuv + p.plane[1], at, p.bits, yuv_code(p, 1, 0, q[j][i][0], q[j][i][1], q[j][i][2]));
                yuv_put(yuv + p.plane[2], at, p.bits, yuv_code(p, 2, 0, q[j][i][0], q[j][i][1], q[j][i][2]));
            }
        }
    if (p.chroma == 420) {
        const int cx0 = sx * (kYuvStripW / 2);
        for (int i = 0; i < kYuvStripW / 2 && cx0 + i < p.cw; ++i) {
            int64_t s[3];
            for (int c = 0; c < 3; ++c)
                s[c] = (int64_t)q[0][2 * i][c] + q[0][2 * i + 1][c] + q[1][2 * i][c] + q[1][2 * i + 1][c];
            const size_t at = (size_t)sy * (size_t)p.cw + (size_t)(cx0 + i);
            yuv_put(yuv + p.plane[1], at, p.bits, yuv_code(p, 1, 2, s[0], s[1], s[2]));
            yuv_put(yuv + p.plane[2], at, p.bits, yuv_code(p, 2, 2, s[0], s[1], s[2]));
        }
    }
}

template <bool HDR>
struct YuvNarrowLoad {
    const void* src;
    int w, h;
    RRT_YUV_MEMBER void operator()(int col, int row, bool, int q[3]) const { yuv_load_q<HDR>(src, w, h, col, row, q); }
};

template <bool HDR>
RRT_FN void yuv_strip_narrow(uint8_t* yuv, const void* src, const YuvPlan& p, int sx, int sy) {
    const YuvNarrowLoad<HDR> load = {src, p.w, p.h};
    yuv_strip_narrow_with(yuv, p, sx, sy, load);
}
static_assert(kYuvStripH == 2 && kYuvStripW % 2 == 0, "a strip holds whole 2 x 2 chroma blocks");

/* ---- host only: the format's checks, the plan, the conversion of a frame in host memory (rrt_yuv.hip's C ABI calls these) ---- */

static inline int yuv_check_format(const rrt_yuv_format* f) {
    if (!f) return RRT_ERR_INVALID_ARGUMENT;
    if (f->struct_size != sizeof(rrt_yuv_format)) return RRT_ERR_ABI_MISMATCH;
    if ((f->chroma != 420 && f->chroma != 444) || (f->range != 0 && f->range != 1) || (f->bits != 8 && f->bits != 10))
        return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}

/* BT.709's Kr and Kb unless told otherwise (rrt_hdr10_core.h passes BT.2020's) */
static inline void yuv_coefficients(const rrt_yuv_format& f, int64_t coef[9], int32_t off[3], double Kr = 0.2126, double Kb = 0.0722) {
    const double Kg = 1.0 - Kr - Kb;
    const double K[9] = {Kr, Kg, Kb,
                         -Kr / (2.0 * (1.0 - Kb)), -Kg / (2.0 * (1.0 - Kb)), 0.5,
                         0.5, -Kg / (2.0 * (1.0 - Kr)), -Kb / (2.0 * (1.0 - Kr))};
    const int k = 1 << (f.bits - 8), top = (1 << f.bits) - 1;
    for (int r = 0; r < 3; ++r) {
        const double A = f.range ? (double)top : (r == 0 ? 219.0 * k : 224.0 * k);
        for (int c = 0; c < 3; ++c) coef[3 * r + c] = (int64_t)std::llround(K[3 * r + c] * A * 1073741824.0 / 65535.0);
    }
    off[0] = f.range ? 0 : 16 * k;
    off[1] = off[2] = 1 << (f.bits - 1);
}

static inline int yuv_plan(const rrt_yuv_format* f, int w, int h, YuvPlan& p) {
    const int rc = yuv_check_format(f);
    if (rc != RRT_OK) return rc;
    if (w <= 0 || h <= 0 || (int64_t)w * h >= ((int64_t)1 << 31)) return RRT_ERR_INVALID_ARGUMENT;
    yuv_coefficients(*f, p.coef, p.off);
    p.bits = f->bits;
    p.chroma = f->chroma;
    p.w = w;
    p.h = h;
    p.cw = f->chroma == 420 ? (w + 1) >> 1 : w;
    p.ch = f->chroma == 420 ? (h + 1) >> 1 : h;
    p.strips_x = (w + kYuvStripW - 1) / kYuvStripW;
    p.strips_y = (h + kYuvStripH - 1) / kYuvStripH;
    const uint64_t bps = f->bits == 8 ? 1 : 2;
    p.plane[0] = 0;
    p.plane[1] = (uint64_t)w * h * bps;
    p.plane[2] = p.plane[1] + (uint64_t)p.cw * p.ch * bps;
    return RRT_OK;
}

static inline uint64_t yuv_bytes(const YuvPlan& p) { return p.plane[2] + (p.plane[2] - p.plane[1]); }

/* the wide kernel's stores: kYuvStripW samples per luma (and 4:4:4 chroma) row, half as many per 4:2:0 chroma row.  d_yuv itself is
 * 16-byte aligned (a launch refuses another), so offsets decide. */
static inline bool yuv_wide_ok(const YuvPlan& p) {
    const uint64_t bps = p.bits == 8 ? 1 : 2;
    const uint64_t ystore = kYuvStripW * bps, cstore = (p.chroma == 420 ? kYuvStripW / 2 : kYuvStripW) * bps;
    if (p.w % kYuvStripW != 0) return false;                            /* whole strips; an RGBA8 row then starts on 16 bytes too */
    if (((uint64_t)p.w * bps) % ystore != 0) return false;
    if (p.plane[1] % cstore != 0 || p.plane[2] % cstore != 0 || ((uint64_t)p.cw * bps) % cstore != 0) return false;
    return true;
}

template <bool HDR>
static inline int yuv_host(void* yuv, const void* src, int w, int h, const rrt_yuv_format* fmt) {
    if (!yuv || !src) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    const int rc = yuv_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    const uintptr_t out = (uintptr_t)yuv, in = (uintptr_t)src;
    if (out < in + (uint64_t)w * h * (HDR ? 16 : 4) && in < out + yuv_bytes(p)) return RRT_ERR_INVALID_ARGUMENT;
    for (int sy = 0; sy < p.strips_y; ++sy)
        for (int sx = 0; sx < p.strips_x; ++sx) yuv_strip_narrow<HDR>(static_cast<uint8_t*>(yuv), src, p, sx, sy);
    return RRT_OK;
}

#endif /* RRT_YUV_CORE_H */
