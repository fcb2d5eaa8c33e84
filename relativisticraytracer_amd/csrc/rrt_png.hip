/*
 * rrt_png.hip -- librrt_png.so (include/rrt_png.h): a finished frame as the filtered scanlines of a PNG file on the device.
 *
 * A row's stride is 1 + 3 w or 1 + 6 w bytes, so rows start at every byte alignment of the payload.  Two kernels write the same bytes:
 *
 *   png_wide<HDR>     a workgroup of kPngWideThreads owns a band of RRT_PNG_BAND_ROWS consecutive rows.  It stages a row's RAW bytes
 *                     in LDS -- 16-byte loads of the input; at depth 16 every pixel is tone-mapped once per band plus once for the
 *                     row above the band, not once per use --, keeps the row above in a second buffer, and walks the row in CHUNKS:
 *                     the 16-byte words of the PAYLOAD that the row's span touches.  A thread reads a chunk's 16 + bpp raw bytes of
 *                     both rows from LDS once (seven aligned words each, shifted into place) and scores all five candidates from
 *                     them; the scores are reduced with __shfl_xor and LDS; then the chunks are walked again with the winning
 *                     filter, each written with ONE aligned 16-byte store, and summed for the row's s1 and s2.  Only the first and
 *                     the last chunk of a row are partial: their bytes are stored one by one, so every payload byte is written
 *                     once, by one thread, and no word that two rows share is read back.  A row longer than the staging
 *                     (RRT_PNG_SEGMENT_CHUNKS chunks, 2 x 32.5 KB of LDS) is cut into segments, each staged with both rows.
 *   png_narrow<HDR>   png_row of rrt_png_core.h, the definition: a thread filters a row, one byte per store, plain loops.  Any
 *                     alignment.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include "../../include/rrt_png.h"
#include "rrt_png_core.h"

/* ---- device ---------------------------------------------------------------------------------------------------------------- */

/* `count` pixels of PNG row `row` from column p_lo on as raw bytes at buf; a column left of 0 and the row above row 0 are zeros */
template <bool HDR>
__device__ __forceinline__ void png_stage(uint8_t* buf, const void* __restrict__ src, const PngPlan& p, int row, int p_lo, int count) {
    const int tid = (int)threadIdx.x;
    if constexpr (HDR) {
        const float4* line = static_cast<const float4*>(src) + (size_t)(p.h - 1 - row) * (size_t)p.w;
        for (int q = tid; q < count; q += kPngWideThreads) {
            const int x = p_lo + q;
            uint32_t s[3] = {0u, 0u, 0u};
            if (row >= 0 && x >= 0) {
                const float4 v = line[x];
                s[0] = (uint32_t)yuv_q_from_hdr(v.x);
                s[1] = (uint32_t)yuv_q_from_hdr(v.y);
                s[2] = (uint32_t)yuv_q_from_hdr(v.z);
            }
            uint16_t* dst = reinterpret_cast<uint16_t*>(buf + (size_t)q * 6u);      /* most significant byte first */
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = (uint16_t)((s[c] >> 8) | ((s[c] & 255u) << 8));
        }
    } else {
        if (row < 0) {
            for (int t = tid; t < count * 3; t += kPngWideThreads) buf[t] = 0;
            return;
        }
        for (int t = tid; t < -p_lo * 3; t += kPngWideThreads) buf[t] = 0;
        /* the row's pixels by their number in the frame, in the aligned groups of four that 16-byte loads fetch */
        const uint32_t total = (uint32_t)p.w * (uint32_t)p.h, first = (uint32_t)(p.h - 1 - row) * (uint32_t)p.w;
        const uint32_t l0 = first + (uint32_t)(p_lo > 0 ? p_lo : 0), l1 = first + (uint32_t)(p_lo + count - 1);
        const uint32_t* px = static_cast<const uint32_t*>(src);
        for (uint32_t g = (l0 >> 2) + (uint32_t)tid; g <= (l1 >> 2); g += kPngWideThreads) {
            uint32_t v[4] = {0u, 0u, 0u, 0u};
            if (4u * g + 3u < total) {
                const uint4 t = reinterpret_cast<const uint4*>(px)[g];
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (4u * g + (uint32_t)j < total) v[j] = px[4u * g + (uint32_t)j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t l = 4u * g + (uint32_t)j;
                if (l < l0 || l > l1) continue;
                uint8_t* dst = buf + (size_t)((int)(l - first) - p_lo) * 3u;
                dst[0] = (uint8_t)v[j];
                dst[1] = (uint8_t)(v[j] >> 8);
                dst[2] = (uint8_t)(v[j] >> 16);
            }
        }
    }
}

/* the 24 bytes buf[lo ...) as six words, byte 0 of w[0] = buf[lo]: seven aligned LDS words, shifted into place */
__device__ __forceinline__ void png_window(const uint8_t* buf, int lo, uint32_t w[6]) {
    const uint32_t* d = reinterpret_cast<const uint32_t*>(buf + (lo & ~3));
    const uint32_t sh = (uint32_t)(lo & 3) * 8u;
    uint32_t t[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) t[k] = d[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = (uint32_t)(((((uint64_t)t[k + 1]) << 32) | t[k]) >> sh);
}

#define PNG_BYTE(w, k) (((w)[(k) >> 2] >> (((k) & 3) * 8)) & 255u)

/* sums over the workgroup, left in every thread; `red` is free again once every thread has passed the next barrier */
template <int N>
__device__ __forceinline__ void png_reduce(uint64_t v[N], uint64_t (*red)[5]) {
#pragma unroll
    for (int n = 0; n < N; ++n) {
        uint32_t lo = (uint32_t)v[n], hi = (uint32_t)(v[n] >> 32);
        uint64_t acc = v[n];
        for (int off = 32; off >= 1; off >>= 1) {
            const uint32_t ol = (uint32_t)__shfl_xor((int)lo, off), oh = (uint32_t)__shfl_xor((int)hi, off);
            acc += ((uint64_t)oh << 32) | ol;
            lo = (uint32_t)acc;
            hi = (uint32_t)(acc >> 32);
        }
        v[n] = acc;
    }
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int n = 0; n < N; ++n) red[wave][n] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = red[0][n] + red[1][n] + red[2][n] + red[3][n];
}

template <bool HDR>
__global__ __launch_bounds__(kPngWideThreads) void png_wide(uint8_t* __restrict__ payload, uint32_t* __restrict__ sums, const void* __restrict__ src, PngPlan p) {
    constexpr int BPP = HDR ? 6 : 3;
    extern __shared__ uint4 png_lds[];
    __shared__ uint64_t red[kPngWideThreads / 64][5];
    const uint32_t buf_bytes = 16u * (uint32_t)p.seg_chunks + (uint32_t)kPngBufSlack;
    uint8_t* cur = reinterpret_cast<uint8_t*>(png_lds);
    uint8_t* prev = cur + buf_bytes;
    const int tid = (int)threadIdx.x;
    const bool one = p.chunks <= p.seg_chunks;          /* every row is one segment: a staged row serves as the next row's row above */
    const int r0 = (int)blockIdx.x * RRT_PNG_BAND_ROWS;
    const int r1 = r0 + RRT_PNG_BAND_ROWS < p.h ? r0 + RRT_PNG_BAND_ROWS : p.h;
    int64_t base_cur = 0, base_prev = 0;                /* the raw byte index of each buffer's byte 0 */
    for (int r = r0; r < r1; ++r) {
        const uint64_t s = (uint64_t)r * p.stride;      /* the row's span starts here; the payload is 16-byte aligned */
        const int64_t A = (int64_t)(s & 15u);           /* chunk c holds the row's bytes 16 c - A ... 16 c - A + 15 */
        const int nc = (int)(((uint64_t)A + p.stride + 15u) / 16u);
        int type = p.filter;
        const bool adaptive = type == RRT_PNG_ADAPTIVE;
        uint32_t score[5] = {0u, 0u, 0u, 0u, 0u};
        uint64_t s1 = 0, pos = 0, neg = 0;
        for (int pass = adaptive ? 0 : 1; pass < 2; ++pass) {
            for (int c0 = 0; c0 < nc; c0 += p.seg_chunks) {
                const int c1 = c0 + p.seg_chunks < nc ? c0 + p.seg_chunks : nc;
                if (!(one && adaptive && pass == 1)) {
                    __syncthreads();                    /* the buffers' last readers are done */
                    const int p_lo = c0 == 0 ? -kPngHaloPixels : (int)((16 * (int64_t)c0 - A - 1 - BPP) / BPP);
                    const int64_t last = (16 * (int64_t)(c1 - 1) - A + 14) / BPP;
                    const int p_hi = last < (int64_t)(p.w - 1) ? (int)last : p.w - 1;
                    const int count = p_hi - p_lo + 1;
                    if (one && r > r0) {
                        uint8_t* t = cur; cur = prev; prev = t;
                        base_prev = base_cur;
                    } else {
                        png_stage<HDR>(prev, src, p, r - 1, p_lo, count);
                        base_prev = (int64_t)p_lo * BPP;
                    }
                    png_stage<HDR>(cur, src, p, r, p_lo, count);
                    base_cur = (int64_t)p_lo * BPP;
                    __syncthreads();
                }
                for (int c = c0 + tid; c < c1; c += kPngWideThreads) {
                    const int64_t i0 = 16 * (int64_t)c - A;
                    uint32_t cw[6], pw[6];
                    png_window(cur, (int)(i0 - 1 - BPP - base_cur), cw);
                    png_window(prev, (int)(i0 - 1 - BPP - base_prev), pw);
                    if (pass == 0) {
#pragma unroll
                        for (int k = 0; k < 16; ++k) {
                            const bool valid = (uint64_t)(i0 + k - 1) < (uint64_t)p.n;
                            const uint32_t x = PNG_BYTE(cw, BPP + k), a = PNG_BYTE(cw, k), b = PNG_BYTE(pw, BPP + k), cc = PNG_BYTE(pw, k);
#pragma unroll
                            for (int t = 0; t < 5; ++t) {
                                const uint32_t cost = png_cost(png_filtered(t, x, a, b, cc));
                                score[t] += valid ? cost : 0u;
                            }
                        }
                    } else {
                        uint32_t out[4] = {0u, 0u, 0u, 0u}, S = 0u, T = 0u;
#pragma unroll
                        for (int k = 0; k < 16; ++k) {
                            const bool valid = (uint64_t)(i0 + k - 1) < (uint64_t)p.n;
                            const uint32_t x = PNG_BYTE(cw, BPP + k), a = PNG_BYTE(cw, k), b = PNG_BYTE(pw, BPP + k), cc = PNG_BYTE(pw, k);
                            const uint32_t d = valid ? png_filtered(type, x, a, b, cc) : (i0 + k == 0 ? (uint32_t)type : 0u);
                            out[k >> 2] |= d << ((k & 3) * 8);
                            S += d;
                            T += (uint32_t)k * d;
                        }
                        uint8_t* dst = payload + s + i0;        /* with i0 < 0 only bytes at or behind payload + s are touched */
                        if (i0 >= 0 && i0 + 16 <= (int64_t)p.stride) {
                            *reinterpret_cast<uint4*>(dst) = make_uint4(out[0], out[1], out[2], out[3]);
                        } else {
#pragma unroll
                            for (int k = 0; k < 16; ++k)
                                if (i0 + k >= 0 && i0 + k < (int64_t)p.stride) dst[k] = (uint8_t)(out[k >> 2] >> ((k & 3) * 8));
                        }
                        /* byte k weighs stride - i0 - k: (stride - i0) S - T, with the first factor reduced so that nothing overflows */
                        const uint64_t W = (uint64_t)((int64_t)p.stride - i0);
                        const uint32_t Wm = W <= 0xffffffffull ? (uint32_t)W % kPngAdler : (uint32_t)(W % kPngAdler);
                        s1 += S;
                        pos += (uint64_t)Wm * S;
                        neg += T;
                    }
                }
            }
            if (pass == 0) {
                uint64_t total[5];
#pragma unroll
                for (int t = 0; t < 5; ++t) total[t] = score[t];
                png_reduce<5>(total, red);
                type = png_choose(total);
            }
        }
        uint64_t v[3] = {s1, pos, neg};
        png_reduce<3>(v, red);
        if (tid == 0) {
            sums[2 * (size_t)r] = (uint32_t)(v[0] % kPngAdler);
            sums[2 * (size_t)r + 1] = (uint32_t)((v[1] % kPngAdler + kPngAdler - v[2] % kPngAdler) % kPngAdler);
        }
    }
}

template <bool HDR>
__global__ __launch_bounds__(kPngNarrowThreads) void png_narrow(uint8_t* payload, uint32_t* sums, const void* src, PngPlan p) {
    const uint32_t r = blockIdx.x * (uint32_t)kPngNarrowThreads + threadIdx.x;
    if (r < (uint32_t)p.h) png_row<HDR>(payload, sums, src, p, (int)r);
}

/* ---- C ABI ----------------------------------------------------------------------------------------------------------------- */

#define RRT_PNG_EXPORT extern "C" __attribute__((visibility("default")))

RRT_PNG_EXPORT int rrt_png_format_default(rrt_png_format* fmt) {
    g_png_err[0] = 0;
    if (!fmt) return png_refuse("fmt is NULL");
    fmt->struct_size = sizeof(rrt_png_format);
    fmt->depth = 8;
    fmt->filter = RRT_PNG_ADAPTIVE;
    return RRT_OK;
}

RRT_PNG_EXPORT int rrt_png_frame_bytes(const rrt_png_format* fmt, int width, int height, size_t* payload_bytes, size_t* stride, size_t* row_sum_bytes) {
    PngPlan p;
    const int rc = png_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!payload_bytes) return png_refuse("payload_bytes is NULL");
    *payload_bytes = (size_t)png_bytes(p);
    if (stride) *stride = p.stride;
    if (row_sum_bytes) *row_sum_bytes = 8u * (size_t)p.h;
    return RRT_OK;
}

RRT_PNG_EXPORT int rrt_png_slices(const rrt_png_format* fmt, int width, int height, int32_t* rows_per_slice, int32_t* n_slices) {
    PngPlan p;
    const int rc = png_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!rows_per_slice || !n_slices) return png_refuse("rows_per_slice or n_slices is NULL");
    png_slices(p, *rows_per_slice, *n_slices);
    return RRT_OK;
}

RRT_PNG_EXPORT int rrt_png_launch_geometry(const rrt_png_format* fmt, int width, int height, size_t address_bits, int32_t out[8]) {
    PngPlan p;
    const int rc = png_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!out) return png_refuse("out is NULL");
    png_geometry(p, address_bits, out);
    return RRT_OK;
}

template <bool HDR>
static int png_launch(void* d_payload, uint32_t* d_row_sums, const void* d_src, int width, int height, const rrt_png_format* fmt, void* stream) {
    PngPlan p;
    int rc = png_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    rc = png_buffers(d_payload, d_row_sums, d_src, p, HDR ? 16 : 8);
    if (rc != RRT_OK) return rc;
    int32_t g[8];
    png_geometry(p, (size_t)((uintptr_t)d_payload | (uintptr_t)d_src), g);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* dst = static_cast<uint8_t*>(d_payload);
    if (g[6]) hipLaunchKernelGGL((png_wide<HDR>), dim3((uint32_t)g[2]), dim3(kPngWideThreads), (size_t)g[5], st, dst, d_row_sums, d_src, p);
    else hipLaunchKernelGGL((png_narrow<HDR>), dim3((uint32_t)g[2]), dim3(kPngNarrowThreads), 0, st, dst, d_row_sums, d_src, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_png_err, sizeof(g_png_err), "%s: %s", HDR ? "png_from_hdr" : "png_from_rgba8", hipGetErrorString(e));
        return RRT_ERR_HIP;
    }
    return RRT_OK;
}

RRT_PNG_EXPORT int rrt_launch_png_from_rgba8(void* d_payload, uint32_t* d_row_sums, const void* d_rgba8, int width, int height, const rrt_png_format* fmt, void* stream) {
    return png_launch<false>(d_payload, d_row_sums, d_rgba8, width, height, fmt, stream);
}

RRT_PNG_EXPORT int rrt_launch_png_from_hdr(void* d_payload, uint32_t* d_row_sums, const float* d_hdr, int width, int height, const rrt_png_format* fmt, void* stream) {
    return png_launch<true>(d_payload, d_row_sums, d_hdr, width, height, fmt, stream);
}

RRT_PNG_EXPORT int rrt_png_from_rgba8_host(void* payload, uint32_t* row_sums, const void* rgba8, int width, int height, const rrt_png_format* fmt) {
    return png_host<false>(payload, row_sums, rgba8, width, height, fmt);
}

RRT_PNG_EXPORT int rrt_png_from_hdr_host(void* payload, uint32_t* row_sums, const float* hdr, int width, int height, const rrt_png_format* fmt) {
    return png_host<true>(payload, row_sums, hdr, width, height, fmt);
}

RRT_PNG_EXPORT int rrt_png_unfilter_host(void* raw, const void* payload, int width, int height, const rrt_png_format* fmt) {
    return png_unfilter(raw, payload, width, height, fmt);
}

RRT_PNG_EXPORT int rrt_png_adler32(const uint32_t* row_sums, int width, int height, const rrt_png_format* fmt, uint32_t* adler) {
    return png_adler32(row_sums, width, height, fmt, adler);
}

RRT_PNG_EXPORT int rrt_png_header(const rrt_png_format* fmt, int width, int height, void* buf, size_t cap, size_t* len) {
    return png_header(fmt, width, height, buf, cap, len);
}

RRT_PNG_EXPORT const char* rrt_png_last_error(void) { return g_png_err; }
