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
 *
 * The HDR10 leg (rrt_hdr10_core.h) runs the same strips through yuv_hdr10_pack_wide / yuv_hdr10_pack_narrow -- only the loader that
 * turns a pixel into sixteen-bit components differs -- and, when it meters, reduces the light levels per workgroup and folds them per
 * frame in yuv_hdr10_fold.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include "../../include/rrt_yuv.h"
#include "rrt_yuv_core.h"
#include "rrt_hdr10_core.h"

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

/* One strip of the wide path, shared by every wide kernel: `load(first, real, q)` gives the sixteen-bit components of the W pixels
 * that start at pixel index `first` of the input (real: false where an odd height makes the strip's second row read its first
 * again).  Used only where yuv_wide_ok holds: width is a multiple of kYuvStripW, so every strip is whole along x; an odd height
 * leaves the last strip row one display row high (its second row is not stored). */
template <int BITS, int CHROMA, class LOAD>
__device__ __forceinline__ void yuv_wide_strip(uint8_t* __restrict__ yuv, const YuvPlan& p, uint32_t s, const LOAD& load) {
    constexpr int W = kYuvStripW, BPS = BITS == 8 ? 1 : 2;
    const int sy = (int)(s / (uint32_t)p.strips_x), sx = (int)(s - (uint32_t)sy * (uint32_t)p.strips_x);
    const int x0 = sx * W, r0 = sy * kYuvStripH;
    const bool two = r0 + 1 < p.h;
    int q[kYuvStripH][W][3];
#pragma unroll
    for (int j = 0; j < kYuvStripH; ++j) {
        const int row = (j == 1 && two) ? r0 + 1 : r0;
        load((size_t)(p.h - 1 - row) * (size_t)p.w + (size_t)x0, j == 0 || two, q[j]);
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

/* the SDR inputs' rows: 16-byte loads, two per row from RGBA8, one per pixel from HDR */
template <bool HDR>
struct YuvWideLoad {
    const void* __restrict__ src;
    __device__ __forceinline__ void operator()(size_t first, bool, int (&q)[kYuvStripW][3]) const {
        constexpr int W = kYuvStripW;
        if constexpr (HDR) {
            const float4* f = static_cast<const float4*>(src) + first;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float4 v = f[i];
                q[i][0] = yuv_q_from_hdr(v.x); q[i][1] = yuv_q_from_hdr(v.y); q[i][2] = yuv_q_from_hdr(v.z);
            }
        } else {
            const uint4* u = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(src) + 4 * first);
            const uint4 a = u[0], b = u[1];
            const uint32_t px[W] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < W; ++i) {
                q[i][0] = yuv_q_from_byte(px[i] & 255u);
                q[i][1] = yuv_q_from_byte((px[i] >> 8) & 255u);
                q[i][2] = yuv_q_from_byte((px[i] >> 16) & 255u);
            }
        }
    }
};

template <bool HDR, int BITS, int CHROMA>
__global__ __launch_bounds__(kYuvThreads) void yuv_pack_wide(uint8_t* __restrict__ yuv, const void* __restrict__ src, YuvPlan p) {
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    const YuvWideLoad<HDR> load = {src};
    for (uint32_t s = blockIdx.x * kYuvThreads + threadIdx.x; s < strips; s += gridDim.x * kYuvThreads)
        yuv_wide_strip<BITS, CHROMA>(yuv, p, s, load);
}

template <bool HDR>
__global__ __launch_bounds__(kYuvThreads) void yuv_pack_narrow(uint8_t* yuv, const void* src, YuvPlan p) {
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    for (uint32_t s = blockIdx.x * kYuvThreads + threadIdx.x; s < strips; s += gridDim.x * kYuvThreads) {
        const int sy = (int)(s / (uint32_t)p.strips_x);
        yuv_strip_narrow<HDR>(yuv, src, p, (int)(s - (uint32_t)sy * (uint32_t)p.strips_x), sy);
    }
}

/* ---- HDR10 (rrt_hdr10_core.h): the same strips, loads and stores around a heavier pixel -- six rrt_pow_pos against three rrt_expf -- */

/* a row of the wide path: one 16-byte load per pixel; a thread meters what it converts into its own sum and max */
template <bool METER>
struct Hdr10WideLoad {
    const float4* __restrict__ hdr;
    const Hdr10Plan& t;
    Hdr10Meter& m;
    __device__ __forceinline__ void operator()(size_t first, bool real, int (&q)[kYuvStripW][3]) const {
        const float4* f = hdr + first;
#pragma unroll
        for (int i = 0; i < kYuvStripW; ++i) {
            const float4 v = f[i];
            uint32_t fx;
            hdr10_pixel(v.x, v.y, v.z, t, q[i], fx);
            if (METER && real) {
                m.sum += fx;
                m.max = fx > m.max ? fx : m.max;
            }
        }
    }
};

/* F: the threads' sums and maxima across the wavefront with __shfl_xor, across the workgroup's wavefronts through LDS, then one
 * 64-bit atomicAdd and one 32-bit atomicMax per workgroup (vector atomics; integers, so exact in any order).  Every thread of the
 * workgroup calls this: a thread whose strips were all out of range brings zeros. */
__device__ __forceinline__ void hdr10_reduce(const Hdr10Meter& m, Hdr10Light* light) {
    constexpr int kWaves = kYuvThreads / 64;
    __shared__ unsigned long long s_sum[kWaves];
    __shared__ uint32_t s_max[kWaves];
    unsigned long long sum = m.sum;
    uint32_t top = m.max;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        const uint32_t other = __shfl_xor(top, d, 64);
        top = other > top ? other : top;
    }
    if ((threadIdx.x & 63u) == 0) {
        s_sum[threadIdx.x >> 6] = sum;
        s_max[threadIdx.x >> 6] = top;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kWaves; ++k) {
            sum += s_sum[k];
            top = s_max[k] > top ? s_max[k] : top;
        }
        atomicAdd(reinterpret_cast<unsigned long long*>(&light->frame_sum), sum);
        atomicMax(&light->frame_max, top);
    }
}
static_assert(kYuvThreads % 64 == 0, "whole wavefronts");

template <int CHROMA, bool METER>
__global__ __launch_bounds__(kYuvThreads) void yuv_hdr10_pack_wide(uint8_t* __restrict__ yuv, const float4* __restrict__ hdr, YuvPlan p,
                                                                   Hdr10Plan t, Hdr10Light* __restrict__ light) {
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    Hdr10Meter m = {0, 0};
    const Hdr10WideLoad<METER> load = {hdr, t, m};
    for (uint32_t s = blockIdx.x * kYuvThreads + threadIdx.x; s < strips; s += gridDim.x * kYuvThreads)
        yuv_wide_strip<10, CHROMA>(yuv, p, s, load);
    if constexpr (METER) hdr10_reduce(m, light);
}

template <bool METER>
__global__ __launch_bounds__(kYuvThreads) void yuv_hdr10_pack_narrow(uint8_t* yuv, const float* hdr, YuvPlan p, Hdr10Plan t,
                                                                     Hdr10Light* light) {
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    Hdr10Meter m = {0, 0};
    const Hdr10NarrowLoad load = {hdr, &t, METER ? &m : nullptr, p.w, p.h};
    for (uint32_t s = blockIdx.x * kYuvThreads + threadIdx.x; s < strips; s += gridDim.x * kYuvThreads) {
        const int sy = (int)(s / (uint32_t)p.strips_x);
        yuv_strip_narrow_with(yuv, p, (int)(s - (uint32_t)sy * (uint32_t)p.strips_x), sy, load);
    }
    if constexpr (METER) hdr10_reduce(m, light);
}

/* one thread, behind the pack kernel on the same stream (static: the library exports its C ABI only, no host stubs) */
static __global__ void yuv_hdr10_fold(Hdr10Light* light) { hdr10_fold(light); }

static __global__ void yuv_hdr10_reset(Hdr10Light* light) { *light = Hdr10Light{0, 0, 0, 0, 0, 0}; }

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

static bool yuv_overlap(uintptr_t a, uint64_t a_bytes, uintptr_t b, uint64_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

static int hdr10_hip_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return RRT_OK;
    snprintf(g_yuv_err, sizeof(g_yuv_err), "%s: %s", what, hipGetErrorString(e));
    return RRT_ERR_HIP;
}

/* the pack kernel and, with d_light, the fold kernel behind it: a linear chain on `stream` */
static int hdr10_launch(void* d_yuv, const float* d_hdr, int w, int h, const rrt_yuv_format* fmt, const rrt_yuv_hdr10* hdr10, void* d_light,
                        void* stream) {
    if (!d_yuv || !d_hdr) return RRT_ERR_INVALID_ARGUMENT;
    YuvPlan p;
    Hdr10Plan t;
    const int rc = hdr10_plan(fmt, hdr10, w, h, p, t);
    if (rc != RRT_OK) return rc;
    const uintptr_t out = (uintptr_t)d_yuv, in = (uintptr_t)d_hdr, lt = (uintptr_t)d_light;
    if ((out & 15u) != 0 || (in & 15u) != 0 || (lt & 15u) != 0) return RRT_ERR_INVALID_ARGUMENT;
    const uint64_t out_bytes = yuv_bytes(p), in_bytes = (uint64_t)w * h * 16;
    if (yuv_overlap(out, out_bytes, in, in_bytes)) return RRT_ERR_INVALID_ARGUMENT;
    if (d_light && (yuv_overlap(lt, sizeof(Hdr10Light), in, in_bytes) || yuv_overlap(lt, sizeof(Hdr10Light), out, out_bytes)))
        return RRT_ERR_INVALID_ARGUMENT;
    const uint32_t strips = (uint32_t)p.strips_x * (uint32_t)p.strips_y;
    const uint32_t want = (strips + kYuvThreads - 1) / kYuvThreads;
    const dim3 grid(want < kYuvMaxGroups ? want : kYuvMaxGroups), block(kYuvThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* y = static_cast<uint8_t*>(d_yuv);
    const float4* f4 = reinterpret_cast<const float4*>(d_hdr);
    Hdr10Light* light = static_cast<Hdr10Light*>(d_light);
    if (!yuv_wide_ok(p)) {
        if (light) hipLaunchKernelGGL(yuv_hdr10_pack_narrow<true>, grid, block, 0, st, y, d_hdr, p, t, light);
        else hipLaunchKernelGGL(yuv_hdr10_pack_narrow<false>, grid, block, 0, st, y, d_hdr, p, t, light);
    } else if (p.chroma == 420) {
        if (light) hipLaunchKernelGGL((yuv_hdr10_pack_wide<420, true>), grid, block, 0, st, y, f4, p, t, light);
        else hipLaunchKernelGGL((yuv_hdr10_pack_wide<420, false>), grid, block, 0, st, y, f4, p, t, light);
    } else {
        if (light) hipLaunchKernelGGL((yuv_hdr10_pack_wide<444, true>), grid, block, 0, st, y, f4, p, t, light);
        else hipLaunchKernelGGL((yuv_hdr10_pack_wide<444, false>), grid, block, 0, st, y, f4, p, t, light);
    }
    int status = hdr10_hip_status("yuv_hdr10_from_hdr");
    if (status == RRT_OK && light) {
        hipLaunchKernelGGL(yuv_hdr10_fold, dim3(1), dim3(1), 0, st, light);
        status = hdr10_hip_status("yuv_hdr10_fold");
    }
    return status;
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

RRT_YUV_EXPORT int rrt_yuv_hdr10_default(rrt_yuv_hdr10* hdr10) {
    if (!hdr10) return RRT_ERR_INVALID_ARGUMENT;
    hdr10->struct_size = sizeof(rrt_yuv_hdr10);
    hdr10->white_nits = 203.0f;
    hdr10->peak_nits = 1000.0f;
    hdr10->knee = 0.5f;
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_yuv_hdr10_coefficients(const rrt_yuv_format* fmt, int64_t coef[9], int32_t off[3]) {
    if (!coef || !off) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = yuv_check_format(fmt);
    if (rc != RRT_OK) return rc;
    if (fmt->bits != 10) return RRT_ERR_INVALID_ARGUMENT;
    yuv_coefficients(*fmt, coef, off, kHdr10Kr, kHdr10Kb);
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_yuv_hdr10_light_bytes(size_t* bytes) {
    if (!bytes) return RRT_ERR_INVALID_ARGUMENT;
    *bytes = sizeof(Hdr10Light);
    return RRT_OK;
}

RRT_YUV_EXPORT int rrt_launch_yuv_hdr10_from_hdr(void* d_yuv, const float* d_hdr, int width, int height, const rrt_yuv_format* fmt,
                                                 const rrt_yuv_hdr10* hdr10, void* d_light, void* stream) {
    return hdr10_launch(d_yuv, d_hdr, width, height, fmt, hdr10, d_light, stream);
}

RRT_YUV_EXPORT int rrt_launch_yuv_hdr10_light_reset(void* d_light, void* stream) {
    if (!d_light || ((uintptr_t)d_light & 15u) != 0) return RRT_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(yuv_hdr10_reset, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), static_cast<Hdr10Light*>(d_light));
    return hdr10_hip_status("yuv_hdr10_light_reset");
}

RRT_YUV_EXPORT int rrt_yuv_hdr10_from_hdr_host(void* yuv, const float* hdr, int width, int height, const rrt_yuv_format* fmt,
                                               const rrt_yuv_hdr10* hdr10, void* light) {
    return hdr10_host(yuv, hdr, width, height, fmt, hdr10, static_cast<Hdr10Light*>(light));
}

RRT_YUV_EXPORT int rrt_yuv_hdr10_light_levels(const void* state_copy, int width, int height, uint32_t out[3]) {
    return hdr10_levels(static_cast<const Hdr10Light*>(state_copy), width, height, out);
}

RRT_YUV_EXPORT int rrt_y4m_hdr10_sidecar(const rrt_yuv_hdr10* hdr10, const uint32_t levels[3], char* buf, size_t cap, size_t* len) {
    return hdr10_sidecar(hdr10, levels, buf, cap, len);
}
