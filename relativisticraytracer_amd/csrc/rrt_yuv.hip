/*
 * rrt_yuv.hip -- librrt_yuv.so (include/rrt_yuv.h): a frame packed as planar BT.709 Y'CbCr on the device.
 *
 * The pass is memory-bound: a thread converts one strip of kYuvStripW x kYuvStripH pixels (rrt_yuv_core.h), consecutive lanes take
 * consecutive strips of a row pair, and a 4:2:0 thread averages its chroma from the pixels it already holds -- one kernel, no LDS,
 * no second pass.  Two kernels write the same codes:
 *
 *   yuv_pack_wide     16-byte loads (two per row from RGBA8, one per pixel from HDR) and one store per plane and row of
 *                     kYuvStripW samples (8 or 16 bytes), kYuvStripW / 2 samples (4 or 8 bytes) for 4:2:0 chroma.  The planes are
 *                     tightly packed, so their bases and row starts are aligned only by accident: this kernel is launched only when
 *                     every row start of every plane is a multiple of its store's width (yuv_wide_ok), and then a frame has no
 *                     partial strip either.
 *   yuv_pack_narrow   yuv_strip_narrow: one sample per load and store, any size.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include "../../include/rrt_yuv.h"
#include "rrt_yuv_core.h"

constexpr int kYuvThreads = 256;
constexpr unsigned kYuvMaxGroups = 1u << 20;     /* beyond it the strips are taken in rounds (grid-stride) */

static thread_local char g_yuv_err[256] = "";

/* ---- device ---------------------------------------------------------------------------------------------------------------- */

/* N codes as one store: 8 x 8 bits = 8 bytes, 4 x 8 bits = 4, 8 x 10 bits = 16, 4 x 10 bits = 8 */
template <int BITS, int N>
__device__ __forceinline__ void yuv_store(uint8_t* dst, const int* c) {
    if constexpr (BITS == 8) {
        const uint32_t a = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
        if constexpr (N == 4) {
            *reinterpret_cast<uint32_t*>(dst) = a;
        } else {
            const uint32_t b = (uint32_t)c[4] | ((uint32_t)c[5] << 8) | ((uint32_t)c[6] << 16) | ((uint32_t)c[7] << 24);
            *reinterpret_cast<uint2*>(dst) = make_uint2(a, b);
        }
    } else {
        const uint32_t a = (uint32_t)c[0] | ((uint32_t)c[1] << 16), b = (uint32_t)c[2] | ((uint32_t)c[3] << 16);
        if constexpr (N == 4) {
            *reinterpret_cast<uint2*>(dst) = make_uint2(a, b);
        } else {
            const uint32_t d = (uint32_t)c[4] | ((uint32_t)c[5] << 16), e = (uint32_t)c[6] | ((uint32_t)c[7] << 16);
            *reinterpret_cast<uint4*>(dst) = make_uint4(a, b, d, e);
        }
    }
}

/* Launched only where yuv_wide_ok holds: width is a multiple of kYuvStripW, so every strip is whole along x; an odd height leaves
 * the last strip row one display row high (its second row reads the first again and is not stored). */
template <bool HDR, int BITS, int CHROMA>
__global__ __launch_bounds__(kYuvThreads) void yuv_pack_wide(uint8_t* __restrict__ yuv, const void* __restrict__ src, YuvPlan p) {
    constexpr int W = kYuvStripW, BPS = BITS == 8 ? 1 : 2;
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    for (uint32_t s = blockIdx.x * kYuvThreads + threadIdx.x; s < strips; s += gridDim.x * kYuvThreads) {
        const int sy = (int)(s / (uint32_t)p.strips_x), sx = (int)(s - (uint32_t)sy * (uint32_t)p.strips_x);
        const int x0 = sx * W, r0 = sy * kYuvStripH;
        const bool two = r0 + 1 < p.h;
        int q[kYuvStripH][W][3];
#pragma unroll
        for (int j = 0; j < kYuvStripH; ++j) {
            const int row = (j == 1 && two) ? r0 + 1 : r0;
            const size_t first = (size_t)(p.h - 1 - row) * (size_t)p.w + (size_t)x0;
            if constexpr (HDR) {
                const float4* f = static_cast<const float4*>(src) + first;
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float4 v = f[i];
                    q[j][i][0] = yuv_q_from_hdr(v.x); q[j][i][1] = yuv_q_from_hdr(v.y); q[j][i][2] = yuv_q_from_hdr(v.z);
                }
            } else {
                const uint4* u = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(src) + 4 * first);
                const uint4 a = u[0], b = u[1];
                const uint32_t px[W] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    q[j][i][0] = yuv_q_from_byte(px[i] & 255u);
                    q[j][i][1] = yuv_q_from_byte((px[i] >> 8) & 255u);
                    q[j][i][2] = yuv_q_from_byte((px[i] >> 16) & 255u);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kYuvStripH; ++j) {
            if (j == 1 && !two) break;
            const size_t at = ((size_t)(r0 + j) * (size_t)p.w + (size_t)x0) * BPS;
            int code[W];
#pragma unroll
            for (int i = 0; i < W; ++i) code[i] = yuv_code(p, 0, 0, q[j][i][0], q[j][i][1], q[j][i][2]);
            yuv_store<BITS, W>(yuv + p.plane[0] + at, code);
            if constexpr (CHROMA == 444) {
#pragma unroll
                for (int c = 1; c < 3; ++c) {
#pragma unroll
                    for (int i = 0; i < W; ++i) code[i] = yuv_code(p, c, 0, q[j][i][0], q[j][i][1], q[j][i][2]);
                    yuv_store<BITS, W>(yuv + p.plane[c] + at, code);
                }
            }
        }
        if constexpr (CHROMA == 420) {
            const size_t at = ((size_t)sy * (size_t)p.cw + (size_t)(sx * (W / 2))) * BPS;
            int64_t sum[W / 2][3];
#pragma unroll
            for (int i = 0; i < W / 2; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    sum[i][c] = (int64_t)q[0][2 * i][c] + q[0][2 * i + 1][c] + q[1][2 * i][c] + q[1][2 * i + 1][c];
#pragma unroll
            for (int c = 1; c < 3; ++c) {
                int code[W / 2];
#pragma unroll
                for (int i = 0; i < W / 2; ++i) code[i] = yuv_code(p, c, 2, sum[i][0], sum[i][1], sum[i][2]);
                yuv_store<BITS, W / 2>(yuv + p.plane[c] + at, code);
            }
        }
    }
}

template <bool HDR>
__global__ __launch_bounds__(kYuvThreads) void yuv_pack_narrow(uint8_t* yuv, const void* src, YuvPlan p) {
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    for (uint32_t s = blockIdx.x * kYuvThreads + threadIdx.x; s < strips; s += gridDim.x * kYuvThreads) {
        const int sy = (int)(s / (uint32_t)p.strips_x);
        yuv_strip_narrow<HDR>(yuv, src, p, (int)(s - (uint32_t)sy * (uint32_t)p.strips_x), sy);
    }
}

/* ---- launches -------------------------------------------------------------------------------------------------------------- */

template <bool HDR>
static int yuv_launch(void* d_yuv, const void* d_src, int w, int h, const rrt_yuv_format* fmt, void* stream) {
    if (!d_yuv || !d_src) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    const int rc = yuv_plan(fmt, w, h, p);
    if (rc != RRT_OK) return rc;
    const uintptr_t out = (uintptr_t)d_yuv, in = (uintptr_t)d_src;
    if ((out & 15u) != 0 || (in & (HDR ? 15u : 3u)) != 0) return RRT_ERR_INVALID_ARGUMENT;
    const uint64_t out_bytes = yuv_bytes(p), in_bytes = (uint64_t)w * h * (HDR ? 16 : 4);
    if (out < in + in_bytes && in < out + out_bytes) return RRT_ERR_INVALID_ARGUMENT;
    /* strips <= width * height < 2^31 */
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    const uint32_t want = (strips + kYuvThreads - 1) / kYuvThreads;
    const dim3 grid(want < kYuvMaxGroups ? want : kYuvMaxGroups), block(kYuvThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* y = static_cast<uint8_t*>(d_yuv);
    const bool wide = yuv_wide_ok(p) && (HDR || (in & 15u) == 0);      /* RGBA8 rows start on 16 bytes only if the frame does */
    if (!wide)
        hipLaunchKernelGGL(yuv_pack_narrow<HDR>, grid, block, 0, st, y, d_src, p);
    else if (p.bits == 8 && p.chroma == 420)
        hipLaunchKernelGGL((yuv_pack_wide<HDR, 8, 420>), grid, block, 0, st, y, d_src, p);
    else if (p.bits == 8)
        hipLaunchKernelGGL((yuv_pack_wide<HDR, 8, 444>), grid, block, 0, st, y, d_src, p);
    else if (p.chroma == 420)
        hipLaunchKernelGGL((yuv_pack_wide<HDR, 10, 420>), grid, block, 0, st, y, d_src, p);
    else
        hipLaunchKernelGGL((yuv_pack_wide<HDR, 10, 444>), grid, block, 0, st, y, d_src, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_yuv_err, sizeof(g_yuv_err), "%s: %s", HDR ? "yuv_from_hdr" : "yuv_from_rgba8", hipGetErrorString(e));
        return RRT_ERR_HIP;
    }
    return RRT_OK;
}

/* ---- C ABI ----------------------------------------------------------------------------------------------------------------- */

#define RRT_YUV_EXPORT extern "C" __attribute__((visibility("default")))

RRT_YUV_EXPORT int rrt_yuv_format_default(rrt_yuv_format* fmt) {
    if (!fmt) return RRT_ERR_INVALID_ARGUMENT;
    fmt->struct_size = sizeof(rrt_yuv_format);
    fmt->chroma = 420;
    fmt->range = 0;
    fmt->bits = 8;
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_yuv_coefficients(const rrt_yuv_format* fmt, int64_t coef[9], int32_t off[3]) {
    if (!coef || !off) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = yuv_check_format(fmt);
    if (rc != RRT_OK) return rc;
    yuv_coefficients(*fmt, coef, off);
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_yuv_frame_bytes(const rrt_yuv_format* fmt, int width, int height, size_t* bytes, size_t plane_offset[3]) {
    if (!bytes) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    const int rc = yuv_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    *bytes = (size_t)yuv_bytes(p);
    if (plane_offset)
        for (int i = 0; i < 3; ++i) plane_offset[i] = (size_t)p.plane[i];
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_y4m_header(const rrt_yuv_format* fmt, int width, int height, int fps_num, int fps_den, char* buf, size_t cap,
                                  size_t* len) {
    if (!buf || !len) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    const int rc = yuv_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (fps_num <= 0 || fps_den <= 0) return RRT_ERR_INVALID_ARGUMENT;
    const char* tag = fmt->bits == 8 ? (fmt->chroma == 420 ? "420jpeg" : "444") : (fmt->chroma == 420 ? "420p10" : "444p10");
    char line[160];
    const int n = snprintf(line, sizeof(line), "YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s XCOLORRANGE=%s\n", width, height, fps_num, fps_den,
                           tag, fmt->range ? "FULL" : "LIMITED");
    if (n <= 0 || (size_t)n >= sizeof(line) || (size_t)n > cap) return RRT_ERR_INVALID_ARGUMENT;
    memcpy(buf, line, (size_t)n);
    *len = (size_t)n;
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_yuv_launch_geometry(const rrt_yuv_format* fmt, int width, int height, int32_t out[4]) {
    if (!out) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    const int rc = yuv_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    out[0] = kYuvThreads;
    out[1] = kYuvStripW;
    out[2] = kYuvStripH;
    out[3] = yuv_wide_ok(p) ? 1 : 0;
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_launch_yuv_from_rgba8(void* d_yuv, const void* d_rgba8, int width, int height, const rrt_yuv_format* fmt,
                                             void* stream) {
    return yuv_launch<false>(d_yuv, d_rgba8, width, height, fmt, stream);
}

RRT_YUV_EXPORT int rrt_launch_yuv_from_hdr(void* d_yuv, const float* d_hdr, int width, int height, const rrt_yuv_format* fmt,
                                           void* stream) {
    return yuv_launch<true>(d_yuv, d_hdr, width, height, fmt, stream);
}

RRT_YUV_EXPORT int rrt_yuv_from_rgba8_host(void* yuv, const void* rgba8, int width, int height, const rrt_yuv_format* fmt) {
    return yuv_host<false>(yuv, rgba8, width, height, fmt);
}

RRT_YUV_EXPORT int rrt_yuv_from_hdr_host(void* yuv, const float* hdr, int width, int height, const rrt_yuv_format* fmt) {
    return yuv_host<true>(yuv, hdr, width, height, fmt);
}

RRT_YUV_EXPORT const char* rrt_yuv_last_error(void) { return g_yuv_err; }
