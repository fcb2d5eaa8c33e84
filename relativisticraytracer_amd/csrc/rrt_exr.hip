/*
 * rrt_exr.hip -- librrt_exr.so (include/rrt_exr.h): the frame's linear HDR packed as OpenEXR scanline chunks on the device.
 *
 * The pass is memory-bound: 16 bytes read per pixel, 6 or 12 written.  A workgroup is kExrBlockX x kExrBlockY threads: a wavefront
 * along a row, four rows; the grid's y dimension stops at kExrMaxGridY and the workgroups take taller frames in passes.  Two
 * kernels write the same bytes:
 *
 *   exr_pack_wide<TYPE, FILTER>   a thread packs kExrWidePixels = 8 pixels of a row: eight 16-byte loads, then per channel one
 *                                 16-byte store (HALF, NONE), two (FLOAT), or -- filtered -- one store into each half of the chunk:
 *                                 16 bytes each for FLOAT, 8 bytes each for HALF (eight samples have only eight low and eight high
 *                                 bytes).  The filter's predecessor of a thread's first sample is its left neighbour's last: ONE
 *                                 more 16-byte load of the pixel to the left, which the neighbour reads anyway (two loads for the
 *                                 thread at a row's start: the row's last pixel and the previous row's).  No LDS, no second pass.
 *                                 Launched only where exr_wide_ok holds.
 *   exr_pack_narrow               exr_put_sample: one sample per thread, one byte per store, any size and alignment.
 *
 * The wide kernel converts to half with the hardware instruction (exr_convert); the narrow kernel and the host run exr_half_bits'
 * integer arithmetic, the definition.
 *
 * Data layers (rrt_launch_exr_layers) are a second pair, exr_layers_wide<FILTER> and exr_layers_narrow, further down: the same
 * workgroup and grid, any channel list over any sources.  The kernels above are not routed through them.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <stdio.h>
#include <string.h>

#include "../../include/rrt_exr.h"
#include "rrt_exr_core.h"

/* ---- device ---------------------------------------------------------------------------------------------------------------- */

/* The wide kernel's conversion.  HALF: the hardware convert (v_cvt_f16_f32: round to nearest even, subnormal halves kept), then
 * exr_half_bits' NaN and clamp rules on the half's bits -- inf is 0x7c00, above every max_half.  Equal to exr_half_bits on every
 * input of tests/exr_ref.py's conversion_inputs (tests/test_gpu_exr.py).  With the integer form the 3840x2160 half launches took
 * 0.151 and 0.165 ms where they take 0.041 and 0.049 ms ("EXR output"). */
template <int TYPE>
__device__ __forceinline__ uint32_t exr_convert(float f, uint32_t max_half) {
    if constexpr (TYPE == RRT_EXR_HALF) {
        const uint32_t h = __half_as_ushort(__float2half_rn(f)), a = h & 0x7fffu;
        return a > 0x7c00u ? 0u : ((h & 0x8000u) | (a < max_half ? a : max_half));
    } else {
        return __float_as_uint(f);
    }
}

template <int TYPE, bool FILTER>
__global__ __launch_bounds__(kExrBlockX * kExrBlockY) void exr_pack_wide(uint8_t* __restrict__ payload, const float4* __restrict__ hdr, ExrPlan p) {
    constexpr int W = kExrWidePixels;
    constexpr size_t BPS = TYPE == RRT_EXR_HALF ? 2 : 4;
    const uint32_t sx = blockIdx.x * kExrBlockX + threadIdx.x;
    if (sx >= (uint32_t)(p.w / W)) return;
    const int x0 = (int)sx * W;
    const size_t w = (size_t)p.w;
    for (uint32_t yy = blockIdx.y * kExrBlockY + threadIdx.y; yy < (uint32_t)p.h; yy += gridDim.y * kExrBlockY) {
        const int y = (int)yy;
        const float4* row = hdr + (size_t)(p.h - 1 - y) * w;
        uint32_t v[3][W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float4 f = row[x0 + i];
            v[0][i] = exr_convert<TYPE>(f.z, p.max_half);
            v[1][i] = exr_convert<TYPE>(f.y, p.max_half);
            v[2][i] = exr_convert<TYPE>(f.x, p.max_half);
        }
        if constexpr (!FILTER) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                uint8_t* dst = payload + (((size_t)y * 3u + (size_t)c) * w + (size_t)x0) * BPS;
                if constexpr (TYPE == RRT_EXR_HALF) {
                    *reinterpret_cast<uint4*>(dst) = make_uint4(v[c][0] | (v[c][1] << 16), v[c][2] | (v[c][3] << 16), v[c][4] | (v[c][5] << 16),
                                                                v[c][6] | (v[c][7] << 16));
                } else {
                    reinterpret_cast<uint4*>(dst)[0] = make_uint4(v[c][0], v[c][1], v[c][2], v[c][3]);
                    reinterpret_cast<uint4*>(dst)[1] = make_uint4(v[c][4], v[c][5], v[c][6], v[c][7]);
                }
            }
        } else {
            int y0, rows;
            size_t offset;
            exr_chunk_of(p, y, y0, rows, offset);
            /* the predecessors of v[c][0]: the pixel to the left; at a row's start the row's last pixel (G follows B, R follows G) and,
             * for B, the R of the row before -- or, for the chunk's sample 0, of the chunk's last row */
            uint32_t q[3];
            bool first = false;
            if (x0 > 0) {
                const float4 f = row[x0 - 1];
                q[0] = exr_convert<TYPE>(f.z, p.max_half);
                q[1] = exr_convert<TYPE>(f.y, p.max_half);
                q[2] = exr_convert<TYPE>(f.x, p.max_half);
            } else {
                first = y == y0;
                const int yp = first ? y0 + rows - 1 : y - 1;
                const float4 a = row[p.w - 1], b = hdr[(size_t)(p.h - 1 - yp) * w + (w - 1)];
                q[0] = exr_convert<TYPE>(b.x, p.max_half);
                q[1] = exr_convert<TYPE>(a.z, p.max_half);
                q[2] = exr_convert<TYPE>(a.y, p.max_half);
            }
            const size_t half_bytes = (size_t)rows * w * 3u * (BPS / 2);       /* n / 2 */
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const size_t s = ((size_t)(y - y0) * 3u + (size_t)c) * w + (size_t)x0;
                uint8_t* lo_dst = payload + offset + s * (BPS / 2);
                uint8_t* hi_dst = lo_dst + half_bytes;
                uint32_t lo[W], hi[W];          /* a sample's bytes in each half: one (HALF) or two (FLOAT), in the low bits */
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    uint8_t l[2], h[2];
                    exr_filter_sample(TYPE, v[c][i], i == 0 ? q[c] : v[c][i - 1], i == 0 && c == 0 && first, l, h);
                    lo[i] = (uint32_t)l[0] | ((uint32_t)l[1] << 8);
                    hi[i] = (uint32_t)h[0] | ((uint32_t)h[1] << 8);
                }
                if constexpr (TYPE == RRT_EXR_HALF) {
                    *reinterpret_cast<uint2*>(lo_dst) = make_uint2(lo[0] | (lo[1] << 8) | (lo[2] << 16) | (lo[3] << 24),
                                                                   lo[4] | (lo[5] << 8) | (lo[6] << 16) | (lo[7] << 24));
                    *reinterpret_cast<uint2*>(hi_dst) = make_uint2(hi[0] | (hi[1] << 8) | (hi[2] << 16) | (hi[3] << 24),
                                                                   hi[4] | (hi[5] << 8) | (hi[6] << 16) | (hi[7] << 24));
                } else {
                    *reinterpret_cast<uint4*>(lo_dst) = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
                    *reinterpret_cast<uint4*>(hi_dst) = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
                }
            }
        }
    }
}

/* static: the library exports its C ABI only, no host stubs */
static __global__ __launch_bounds__(kExrBlockX * kExrBlockY) void exr_pack_narrow(uint8_t* payload, const float* hdr, ExrPlan p) {
    const uint32_t u = blockIdx.x * kExrBlockX + threadIdx.x;         /* 3 width < 2^31: a row of samples is less than a chunk */
    if (u >= 3u * (uint32_t)p.w) return;
    const int c = (int)(u / (uint32_t)p.w), x = (int)(u - (uint32_t)c * (uint32_t)p.w);
    for (uint32_t y = blockIdx.y * kExrBlockY + threadIdx.y; y < (uint32_t)p.h; y += gridDim.y * kExrBlockY)
        exr_put_sample(payload, hdr, p, (int)y, c, x);
}

/* ---- data layers: any channel list over any sources (include/rrt_exr.h, the second block comment) --------------------------- */

/* exr_layer_sample with the hardware converts: v_cvt_f32_i32 rounds to nearest even as the host's (float)v does */
__device__ __forceinline__ uint32_t exr_layer_convert(int kind, int type, uint32_t u, uint32_t max_half) {
    if (kind == RRT_EXR_SRC_I32) {
        const int32_t v = (int32_t)u;
        if (type == RRT_EXR_UINT) return v < 0 ? 0u : u;
        u = __float_as_uint((float)v);
    }
    return type == RRT_EXR_HALF ? exr_convert<RRT_EXR_HALF>(__uint_as_float(u), max_half) : u;
}

/* A thread packs kExrWidePixels pixels of a row.  Source by source (a wave-uniform loop): 2 * words 16-byte loads, ONCE, then every
 * channel that reads the source -- word, kind and type are wave-uniform, the registers are indexed by constants only -- converted,
 * filtered and stored at the channel's own place in the scanline.  The filter's predecessor of a thread's first sample is one
 * more 4-byte load per channel (exr_layer_pred_of): a word the left neighbour's 16-byte loads fetch anyway.  Launched only where
 * the geometry says wide; p.store8 is its out[6] == 2. */
template <bool FILTER>
__global__ __launch_bounds__(kExrBlockX * kExrBlockY) void exr_layers_wide(uint8_t* __restrict__ payload, ExrLayersPlan p) {
    constexpr int W = kExrWidePixels;
    const uint32_t sx = blockIdx.x * kExrBlockX + threadIdx.x;
    if (sx >= (uint32_t)(p.w / W)) return;
    const int x0 = (int)sx * W;
    const size_t w = (size_t)p.w;
    for (uint32_t yy = blockIdx.y * kExrBlockY + threadIdx.y; yy < (uint32_t)p.h; yy += gridDim.y * kExrBlockY) {
        const int y = (int)yy;
        int y0 = 0, rows = 0;
        size_t offset = 0;
        if constexpr (FILTER) exr_layer_chunk_of(p, y, y0, rows, offset);
        for (int s = 0; s < p.n_src; ++s) {
            const int words = p.src_words[s], kind = p.src_kind[s];
            const size_t row = (size_t)(p.src_bottom_up[s] ? p.h - 1 - y : y);
            const uint4* ptr = reinterpret_cast<const uint4*>(p.src[s] + (row * w + (size_t)x0) * (size_t)words);
            uint32_t r[4 * W];          /* the 8 pixels' words, as they lie */
#pragma unroll
            for (int j = 0; j < W; ++j) {
                uint4 t = make_uint4(0u, 0u, 0u, 0u);
                if (j < 2 * words) t = ptr[j];
                r[4 * j] = t.x; r[4 * j + 1] = t.y; r[4 * j + 2] = t.z; r[4 * j + 3] = t.w;
            }
            for (int c = 0; c < p.n_ch; ++c) {
                if (p.ch_src[c] != s) continue;
                const int k = p.ch_word[c], type = p.ch_type[c];
                uint32_t v[W];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    uint32_t u;
                    if (words == 4) u = k == 0 ? r[4 * i] : k == 1 ? r[4 * i + 1] : k == 2 ? r[4 * i + 2] : r[4 * i + 3];
                    else if (words == 3) u = k == 0 ? r[3 * i] : k == 1 ? r[3 * i + 1] : r[3 * i + 2];
                    else u = r[i];
                    v[i] = exr_layer_convert(kind, type, u, p.max_half);
                }
                if constexpr (!FILTER) {
                    uint8_t* dst = payload + ((size_t)y * (size_t)p.sum_bps + (size_t)p.ch_pre[c]) * w + (size_t)x0 * (size_t)exr_layer_bps(type);
                    if (type == RRT_EXR_HALF) {
                        *reinterpret_cast<uint4*>(dst) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
                    } else {
                        reinterpret_cast<uint4*>(dst)[0] = make_uint4(v[0], v[1], v[2], v[3]);
                        reinterpret_cast<uint4*>(dst)[1] = make_uint4(v[4], v[5], v[6], v[7]);
                    }
                } else {
                    int py, pc, px;
                    bool first;
                    exr_layer_pred_of(p, y, c, x0, y0, rows, py, pc, px, first);
                    const uint32_t t = exr_layer_tail(p.ch_type[pc], exr_layer_convert(p.src_kind[p.ch_src[pc]], p.ch_type[pc], exr_layer_word(p, py, pc, px), p.max_half));
                    const int bps = exr_layer_bps(type);
                    uint32_t lo[W], hi[W];      /* a sample's bytes in each half: one (HALF) or two, in the low bits */
#pragma unroll
                    for (int i = 0; i < W; ++i)
                        exr_layer_filter_sample(bps, v[i], i == 0 ? t : exr_layer_tail(type, v[i - 1]), i == 0 && first, lo[i], hi[i]);
                    uint8_t* lo_dst = payload + offset + ((size_t)(y - y0) * (size_t)p.sum_bps + (size_t)p.ch_pre[c]) / 2u * w + (size_t)x0 * (size_t)(bps / 2);
                    uint8_t* hi_dst = lo_dst + (size_t)rows * w * (size_t)p.sum_bps / 2u;      /* + n / 2 */
                    if (type == RRT_EXR_HALF) {
                        *reinterpret_cast<uint2*>(lo_dst) = make_uint2(lo[0] | (lo[1] << 8) | (lo[2] << 16) | (lo[3] << 24),
                                                                       lo[4] | (lo[5] << 8) | (lo[6] << 16) | (lo[7] << 24));
                        *reinterpret_cast<uint2*>(hi_dst) = make_uint2(hi[0] | (hi[1] << 8) | (hi[2] << 16) | (hi[3] << 24),
                                                                       hi[4] | (hi[5] << 8) | (hi[6] << 16) | (hi[7] << 24));
                    } else {
                        const uint4 a = make_uint4(lo[0] | (lo[1] << 16), lo[2] | (lo[3] << 16), lo[4] | (lo[5] << 16), lo[6] | (lo[7] << 16));
                        const uint4 b = make_uint4(hi[0] | (hi[1] << 16), hi[2] | (hi[3] << 16), hi[4] | (hi[5] << 16), hi[6] | (hi[7] << 16));
                        if (p.store8) {         /* this channel's place in a half may be 8 past a multiple of 16 */
                            reinterpret_cast<uint2*>(lo_dst)[0] = make_uint2(a.x, a.y);
                            reinterpret_cast<uint2*>(lo_dst)[1] = make_uint2(a.z, a.w);
                            reinterpret_cast<uint2*>(hi_dst)[0] = make_uint2(b.x, b.y);
                            reinterpret_cast<uint2*>(hi_dst)[1] = make_uint2(b.z, b.w);
                        } else {
                            *reinterpret_cast<uint4*>(lo_dst) = a;
                            *reinterpret_cast<uint4*>(hi_dst) = b;
                        }
                    }
                }
            }
        }
    }
}

static __global__ __launch_bounds__(kExrBlockX * kExrBlockY) void exr_layers_narrow(uint8_t* payload, ExrLayersPlan p) {
    const uint32_t u = blockIdx.x * kExrBlockX + threadIdx.x;         /* width * n_channels < 2^31: a row of samples is less than a chunk */
    if (u >= (uint32_t)p.n_ch * (uint32_t)p.w) return;
    const int c = (int)(u / (uint32_t)p.w), x = (int)(u - (uint32_t)c * (uint32_t)p.w);
    for (uint32_t y = blockIdx.y * kExrBlockY + threadIdx.y; y < (uint32_t)p.h; y += gridDim.y * kExrBlockY)
        exr_layer_put_sample(payload, p, (int)y, c, x);
}

/* ---- C ABI ----------------------------------------------------------------------------------------------------------------- */

#define RRT_EXR_EXPORT extern "C" __attribute__((visibility("default")))

RRT_EXR_EXPORT int rrt_exr_format_default(rrt_exr_format* fmt) {
    g_exr_err[0] = 0;
    if (!fmt) return exr_refuse("fmt is NULL");
    fmt->struct_size = sizeof(rrt_exr_format);
    fmt->type = RRT_EXR_HALF;
    fmt->compression = RRT_EXR_ZIP;
    fmt->half_max = 65504.0f;
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_frame_bytes(const rrt_exr_format* fmt, int width, int height, size_t* payload_bytes, int32_t* n_chunks) {
    ExrPlan p;
    const int rc = exr_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!payload_bytes) return exr_refuse("payload_bytes is NULL");
    *payload_bytes = (size_t)exr_bytes(p);
    if (n_chunks) *n_chunks = p.n_chunks;
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_chunk(const rrt_exr_format* fmt, int width, int height, int i, int32_t* y, size_t* offset, size_t* bytes) {
    ExrPlan p;
    const int rc = exr_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!y || !offset || !bytes) return exr_refuse("y, offset or bytes is NULL");
    if (i < 0 || i >= p.n_chunks) return exr_refuse("i: a chunk in [0, n_chunks)");
    int y0, rows;
    exr_chunk_of(p, i * p.lines, y0, rows, *offset);
    *y = y0;
    *bytes = (size_t)rows * (size_t)p.w * 3u * (size_t)p.bps;
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_launch_geometry(const rrt_exr_format* fmt, int width, int height, size_t address_bits, int32_t out[8]) {
    ExrPlan p;
    const int rc = exr_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!out) return exr_refuse("out is NULL");
    exr_geometry(p, address_bits, out);
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_launch_exr_from_hdr(void* d_payload, const float* d_hdr, int width, int height, const rrt_exr_format* fmt, void* stream) {
    ExrPlan p;
    const int rc = exr_plan(fmt, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!d_payload || !d_hdr) return exr_refuse("d_payload or d_hdr is NULL");
    const uintptr_t out = (uintptr_t)d_payload, in = (uintptr_t)d_hdr;
    if ((in & 3u) != 0) return exr_refuse("d_hdr is not 4-byte aligned");
    if (exr_overlap(out, exr_bytes(p), in, (uint64_t)width * (uint64_t)height * 16u)) return exr_refuse("d_payload overlaps d_hdr");
    int32_t g[8];
    exr_geometry(p, (size_t)(out | in), g);
    const dim3 grid((uint32_t)g[4], (uint32_t)g[5]), block(kExrBlockX, kExrBlockY);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* dst = static_cast<uint8_t*>(d_payload);
    const float4* f4 = reinterpret_cast<const float4*>(d_hdr);
    const bool filter = p.compression != RRT_EXR_NONE;
    if (!g[6]) hipLaunchKernelGGL(exr_pack_narrow, grid, block, 0, st, dst, d_hdr, p);
    else if (p.type == RRT_EXR_HALF && !filter) hipLaunchKernelGGL((exr_pack_wide<RRT_EXR_HALF, false>), grid, block, 0, st, dst, f4, p);
    else if (p.type == RRT_EXR_HALF) hipLaunchKernelGGL((exr_pack_wide<RRT_EXR_HALF, true>), grid, block, 0, st, dst, f4, p);
    else if (!filter) hipLaunchKernelGGL((exr_pack_wide<RRT_EXR_FLOAT, false>), grid, block, 0, st, dst, f4, p);
    else hipLaunchKernelGGL((exr_pack_wide<RRT_EXR_FLOAT, true>), grid, block, 0, st, dst, f4, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_exr_err, sizeof(g_exr_err), "exr_from_hdr: %s", hipGetErrorString(e));
        return RRT_ERR_HIP;
    }
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_from_hdr_host(void* payload, const float* hdr, int width, int height, const rrt_exr_format* fmt) {
    return exr_host(payload, hdr, width, height, fmt);
}

RRT_EXR_EXPORT int rrt_exr_unfilter_host(void* raw, const void* filtered, size_t n) { return exr_unfilter(raw, filtered, n); }

RRT_EXR_EXPORT int rrt_exr_header(const rrt_exr_format* fmt, int width, int height, int fps_num, int fps_den, void* buf, size_t cap, size_t* len) {
    return exr_header(fmt, width, height, fps_num, fps_den, buf, cap, len);
}

RRT_EXR_EXPORT int rrt_exr_layers_default(rrt_exr_layers* layers) {
    g_exr_err[0] = 0;
    if (!layers) return exr_refuse("layers is NULL");
    memset(layers, 0, sizeof(*layers));
    layers->struct_size = sizeof(rrt_exr_layers);
    layers->compression = RRT_EXR_ZIP;
    layers->half_max = 65504.0f;
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_layers_frame_bytes(const rrt_exr_layers* layers, int width, int height, size_t* payload_bytes, int32_t* n_chunks) {
    ExrLayersPlan p;
    const int rc = exr_layers_plan(layers, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!payload_bytes) return exr_refuse("payload_bytes is NULL");
    *payload_bytes = (size_t)exr_layers_bytes(p);
    if (n_chunks) *n_chunks = p.n_chunks;
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_layers_chunk(const rrt_exr_layers* layers, int width, int height, int i, int32_t* y, size_t* offset, size_t* bytes) {
    ExrLayersPlan p;
    const int rc = exr_layers_plan(layers, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!y || !offset || !bytes) return exr_refuse("y, offset or bytes is NULL");
    if (i < 0 || i >= p.n_chunks) return exr_refuse("i: a chunk in [0, n_chunks)");
    int y0, rows;
    exr_layer_chunk_of(p, i * p.lines, y0, rows, *offset);
    *y = y0;
    *bytes = (size_t)rows * (size_t)p.w * (size_t)p.sum_bps;
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_layers_launch_geometry(const rrt_exr_layers* layers, int width, int height, size_t address_bits, int32_t out[8]) {
    ExrLayersPlan p;
    const int rc = exr_layers_plan(layers, width, height, p);
    if (rc != RRT_OK) return rc;
    if (!out) return exr_refuse("out is NULL");
    exr_layers_geometry(p, address_bits, out);
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_launch_exr_layers(void* d_payload, const rrt_exr_layers* layers, int width, int height, void* stream) {
    ExrLayersPlan p;
    int rc = exr_layers_plan(layers, width, height, p);
    if (rc != RRT_OK) return rc;
    size_t bits;
    rc = exr_layers_buffers(d_payload, p, bits);
    if (rc != RRT_OK) return rc;
    int32_t g[8];
    exr_layers_geometry(p, bits, g);
    const dim3 grid((uint32_t)g[4], (uint32_t)g[5]), block(kExrBlockX, kExrBlockY);
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* dst = static_cast<uint8_t*>(d_payload);
    if (!g[6]) hipLaunchKernelGGL(exr_layers_narrow, grid, block, 0, st, dst, p);
    else if (p.compression == RRT_EXR_NONE) hipLaunchKernelGGL((exr_layers_wide<false>), grid, block, 0, st, dst, p);
    else hipLaunchKernelGGL((exr_layers_wide<true>), grid, block, 0, st, dst, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_exr_err, sizeof(g_exr_err), "exr_layers: %s", hipGetErrorString(e));
        return RRT_ERR_HIP;
    }
    return RRT_OK;
}

RRT_EXR_EXPORT int rrt_exr_layers_host(void* payload, const rrt_exr_layers* layers, int width, int height) {
    return exr_layers_host(payload, layers, width, height);
}

RRT_EXR_EXPORT int rrt_exr_layers_header(const rrt_exr_layers* layers, int width, int height, int fps_num, int fps_den, void* buf, size_t cap, size_t* len) {
    return exr_layers_header(layers, width, height, fps_num, fps_den, buf, cap, len);
}

RRT_EXR_EXPORT const char* rrt_exr_last_error(void) { return g_exr_err; }
