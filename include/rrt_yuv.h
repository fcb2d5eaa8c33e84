/*
 * rrt_yuv.h -- C ABI of librrt_yuv.so: a finished frame packed as planar BT.709 Y'CbCr, 8 or 10 bits, 4:2:0 or 4:4:4, limited or
 * full range, in the byte layout of a YUV4MPEG2 (.y4m) frame.  A library of its own: it needs nothing of the ray marcher (no
 * handles, no rrt_params) and include/rrt.h is unchanged by it; only rrt.h's status values are shared.
 *
 * Conventions (rrt.h's): every function returns an rrt_status; `d_*` pointers are DEVICE pointers owned by the caller; `stream`
 * is a hipStream_t passed as void* (NULL = the null stream).  A launch is ONE kernel on the caller's stream: no allocation, no
 * memset, no synchronisation, the coefficients travel as kernel arguments -- it can be captured into a hipGraph.
 *
 * THE DEFINITION ("Y4M output", has it with its derivation)
 *
 *   The frame is width x height with buffer rows bottom-up (what every launch of rrt.h writes); the planes are top-down: display
 *   row r (0 = top) is buffer row height - 1 - r.
 *
 *   1. Sixteen-bit components q = (qR, qG, qB) per pixel.
 *        from RGBA8:  q_c = byte_c * 257 (alpha ignored);
 *        from linear HDR (the float4 frame an `hdr=` launch or rrt_launch_exposure writes):
 *                     t_c = 1.0f - rrt_expf(-H_c * 0.8f)          -- the march's tone map, uncontracted
 *                     q_c = t_c > 0.0f ? min((int)(t_c * 65535.0f), 65535) : 0     -- binary32 product, truncated
 *                     (NaN and negative HDR give 0, +inf gives 65535).
 *   2. Coefficients, on the host, in binary64: llround(K * A * 1073741824.0 / 65535.0) with Kr = 0.2126, Kb = 0.0722,
 *      Kg = 1.0 - Kr - Kb and the rows
 *        Y  ( Kr,              Kg,               Kb            )
 *        Cb (-Kr/(2(1-Kb)),   -Kg/(2(1-Kb)),     0.5           )
 *        Cr ( 0.5,            -Kg/(2(1-Kr)),    -Kb/(2(1-Kr))  )
 *      With k = 2^(bits-8): limited range A = 219k (Y), 224k (Cb, Cr), offsets 16k, 2^(bits-1), 2^(bits-1);
 *      full range A = 2^bits - 1 for all three, offsets 0, 2^(bits-1), 2^(bits-1).
 *   3. A code from a sum S of 2^n pixels' q, in int64 with an arithmetic shift:
 *        code = clamp((cR*S_R + cG*S_G + cB*S_B + (off << (30+n)) + (1 << (29+n))) >> (30+n), 0, 2^bits - 1)
 *      Luma, and chroma in 4:4:4: one pixel, n = 0.  Chroma in 4:2:0: sample (i, j) of the cw x ch plane, cw = (width+1)>>1,
 *      ch = (height+1)>>1, sums the four pixels at display columns 2i, min(2i+1, width-1) and display rows 2j, min(2j+1, height-1),
 *      n = 2: at an odd edge the last column or row counts twice (centre siting, Y4M's C420jpeg).
 *   4. Frame bytes: the Y plane (height rows of width), then Cb, then Cr (ch x cw, or height x width in 4:4:4), tightly packed, no
 *      padding anywhere; samples are 1 byte at 8 bits, 2 bytes little-endian at 10 bits.
 *   5. Stream: "YUV4MPEG2 W<w> H<h> F<num>:<den> Ip A1:1 C<tag> XCOLORRANGE=<LIMITED|FULL>\n" with <tag> one of 420jpeg, 444,
 *      420p10, 444p10; then per frame "FRAME\n" and the bytes of 4.  Y4M carries no matrix tag: the data is BT.709.
 */
#ifndef RRT_YUV_H
#define RRT_YUV_H

#include <stddef.h>
#include <stdint.h>

#include "rrt.h"     /* rrt_status */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rrt_yuv_format {
    uint32_t struct_size;    /* sizeof(rrt_yuv_format): rrt_yuv_format_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    int32_t chroma;          /* 420 | 444 */
    int32_t range;           /* 0 limited | 1 full */
    int32_t bits;            /* 8 | 10 */
} rrt_yuv_format;

/* 4:2:0, limited range, 8 bits */
int rrt_yuv_format_default(rrt_yuv_format* fmt);

/* Step 2's nine coefficients (rows Y, Cb, Cr; columns R, G, B) and three offsets.  Host only.  RRT_ERR_INVALID_ARGUMENT: NULL
 * pointers, a chroma, range or bits outside the lists (every function below refuses a format the same way). */
int rrt_yuv_coefficients(const rrt_yuv_format* fmt, int64_t coef[9], int32_t off[3]);

/* Step 4's byte count and the byte offsets of the Y, Cb and Cr planes.  Host only; plane_offset may be NULL.
 * RRT_ERR_INVALID_ARGUMENT: NULL bytes, width or height <= 0, width*height >= 2^31. */
int rrt_yuv_frame_bytes(const rrt_yuv_format* fmt, int width, int height, size_t* bytes, size_t plane_offset[3]);

/* Step 5's header line (with its newline, without a terminating NUL) into buf[0 .. cap); *len is its length.  Host only.
 * RRT_ERR_INVALID_ARGUMENT: NULL buf or len, a size rrt_yuv_frame_bytes refuses, fps_num or fps_den <= 0, a cap too small
 * (nothing is written then). */
int rrt_y4m_header(const rrt_yuv_format* fmt, int width, int height, int fps_num, int fps_den, char* buf, size_t cap, size_t* len);

/* How a launch of this size is laid out, for tests and tools: out[0] threads per workgroup, out[1] and out[2] the pixels one
 * thread converts along x and y (its strip), out[3] 1 if this size takes the wide path (vector loads and stores; every row of
 * every plane starts on a multiple of the store's width), 0 if it takes the narrow one (one sample per store).  Strips are
 * numbered row-major over the frame and a workgroup takes out[0] consecutive strips.  Both paths write the same bytes.  (An RGBA8
 * input that is not itself 16-byte aligned takes the narrow path at any size: its rows cannot be loaded 16 bytes at a time.)
 * Host only. */
int rrt_yuv_launch_geometry(const rrt_yuv_format* fmt, int width, int height, int32_t out[4]);

/* The conversions on the device: d_yuv receives rrt_yuv_frame_bytes bytes.  RRT_ERR_INVALID_ARGUMENT, before any device call:
 * NULL pointers, a size or format refused above, d_yuv or d_hdr not 16-byte aligned, d_rgba8 not 4-byte aligned, an output that
 * overlaps the input. */
int rrt_launch_yuv_from_rgba8(void* d_yuv, const void* d_rgba8, int width, int height, const rrt_yuv_format* fmt, void* stream);
int rrt_launch_yuv_from_hdr(void* d_yuv, const float* d_hdr, int width, int height, const rrt_yuv_format* fmt, void* stream);

/* The same conversions on HOST memory, from the source the kernels run (no device is touched); same refusals, without the
 * alignment rules. */
int rrt_yuv_from_rgba8_host(void* yuv, const void* rgba8, int width, int height, const rrt_yuv_format* fmt);
int rrt_yuv_from_hdr_host(void* yuv, const float* hdr, int width, int height, const rrt_yuv_format* fmt);

/* The message of the HIP runtime call that made a launch above or below return RRT_ERR_HIP ("" if none did) */
const char* rrt_yuv_last_error(void);

/*
 * HDR10 OUTPUT ("HDR10 output"): the linear HDR frame as 10-bit BT.2020 non-constant-luminance Y'CbCr behind
 * the SMPTE ST 2084 (PQ) transfer, with the two light levels an HDR10 encoder asks for (MaxCLL, MaxFALL: CTA-861.3) reduced on the
 * device.  Everything is binary32 and uncontracted, one rounding per written operation in the written order.  Per pixel, from
 * H = (H_R, H_G, H_B) (alpha ignored), with white = white_nits, peak = peak_nits and, derived once on the host,
 * K = knee * peak, span = peak - K, inv = 1.0f / span (unused when knee == 1):
 *
 *   A. Light.    a_c = (H_c > 0.0f) ? H_c * white : 0.0f       -- NaN and negative values give 0, +inf stays +inf
 *   B. Gamut (BT.2087, linear light).
 *                b_R = (0.6274f*a_R + 0.3293f*a_G) + 0.0433f*a_B
 *                b_G = (0.0691f*a_R + 0.9195f*a_G) + 0.0114f*a_B
 *                b_B = (0.0164f*a_R + 0.0880f*a_G) + 0.8956f*a_B      -- all terms >= 0: an infinite channel gives +inf, never NaN
 *   C. Shoulder, per channel: the renderer's own exponential curve moved to the top of the range.
 *                b <= K: c = b;  else knee == 1: c = peak;  else c = K + span * (1.0f - rrt_expf(-((b - K) * inv)));
 *                then c = min(c, peak).  Continuous with slope 1 at K, asymptote peak; +inf gives peak.
 *   D. PQ.       y = c * 1.0e-4f;  p = rrt_powf(y, 0.1593017578125f);
 *                e = rrt_powf((0.8359375f + 18.8515625f*p) / (1.0f + 18.6875f*p), 78.84375f)       -- the IEEE quotient
 *                q = min((int)(e * 65535.0f + 0.5f), 65535)
 *   E. Codes.    Steps 2-4 above, unchanged, with Kr = 0.2627, Kb = 0.0593, Kg = 1 - Kr - Kb.  10 bits only; both ranges, both
 *                chroma layouts.
 *   F. Light levels.  Per real pixel m = max(c_R, c_G, c_B) -- step C's nits, the light the file encodes -- and
 *                fx = (uint32_t)(m * 64.0f), truncated, at most 640000.  Each pixel counts once: the edge columns and rows 4:2:0
 *                reads twice are not metered twice.  The state is 32 bytes, 16-byte aligned, owned by the caller:
 *                  { uint64 frame_sum; uint64 max_frame_sum; uint32 frame_max; uint32 max_cll; uint32 frames; uint32 reserved; }
 *                The pack kernel adds every fx into frame_sum and maxes it into frame_max (integer atomics: exact in any order); a
 *                one-thread fold kernel behind it does max_frame_sum = max(max_frame_sum, frame_sum), max_cll = max(max_cll,
 *                frame_max), frames += 1, frame_sum = frame_max = 0.  The host resolves, in integers,
 *                MaxCLL = ceil(max_cll / 64), MaxFALL = ceil(max_frame_sum / (64 * w * h)).
 *   G. Stream.   Step 5's header, unchanged (C420p10 / C444p10): Y4M has no tag for primaries or transfer, so the drivers write
 *                <path>.hdr10.json next to the file when it closes (rrt_y4m_hdr10_sidecar's bytes).
 */
typedef struct rrt_yuv_hdr10 {
    uint32_t struct_size;    /* sizeof(rrt_yuv_hdr10): rrt_yuv_hdr10_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    float white_nits;        /* the luminance of H = 1: 203 (BT.2408's reference white) */
    float peak_nits;         /* the shoulder's asymptote and the mastering display's maximum: 1000 */
    float knee;              /* the shoulder starts at knee * peak_nits: 0.5; 1 is a hard clip, 0 the curve from black */
} rrt_yuv_hdr10;

int rrt_yuv_hdr10_default(rrt_yuv_hdr10* hdr10);

/* Step E's coefficients and offsets.  Host only.  Refuses what rrt_yuv_coefficients refuses, and bits != 10. */
int rrt_yuv_hdr10_coefficients(const rrt_yuv_format* fmt, int64_t coef[9], int32_t off[3]);

/* The size of step F's state: 32 */
int rrt_yuv_hdr10_light_bytes(size_t* bytes);

/* Steps A-F on the device.  d_light NULL: no metering, ONE kernel; otherwise the pack kernel and the fold kernel, a linear chain on
 * the caller's stream.  No allocation, no synchronisation.  Strips and the wide / narrow rule are rrt_yuv_launch_geometry's.
 * Refuses what rrt_launch_yuv_from_hdr refuses, and: fmt->bits != 10; hdr10 NULL; white_nits or peak_nits not finite, <= 0 or
 * > 10000; knee outside [0, 1] (all RRT_ERR_INVALID_ARGUMENT; a wrong hdr10->struct_size is RRT_ERR_ABI_MISMATCH); a d_light that
 * is not 16-byte aligned or overlaps d_yuv or d_hdr. */
int rrt_launch_yuv_hdr10_from_hdr(void* d_yuv, const float* d_hdr, int width, int height, const rrt_yuv_format* fmt,
                                  const rrt_yuv_hdr10* hdr10, void* d_light, void* stream);

/* Zeroes the state (one one-thread kernel): once per film.  RRT_ERR_INVALID_ARGUMENT: NULL or not 16-byte aligned. */
int rrt_launch_yuv_hdr10_light_reset(void* d_light, void* stream);

/* The same on HOST memory, from the source the kernels run; `light` is a host state (pack and fold) or NULL.  Same refusals without
 * the alignment rules. */
int rrt_yuv_hdr10_from_hdr_host(void* yuv, const float* hdr, int width, int height, const rrt_yuv_format* fmt,
                                const rrt_yuv_hdr10* hdr10, void* light);

/* out[0] MaxCLL, out[1] MaxFALL, out[2] the frames folded, from a HOST copy of the state.  Host only. */
int rrt_yuv_hdr10_light_levels(const void* state_copy, int width, int height, uint32_t out[3]);

/* Step G's sidecar into buf[0 .. cap) (no terminating NUL); *len is its length.  Host only.  `levels` is
 * rrt_yuv_hdr10_light_levels' out.  RRT_ERR_INVALID_ARGUMENT: NULL pointers, settings refused above, a cap too small. */
int rrt_y4m_hdr10_sidecar(const rrt_yuv_hdr10* hdr10, const uint32_t levels[3], char* buf, size_t cap, size_t* len);

#ifdef __cplusplus
}
#endif
#endif /* RRT_YUV_H */
