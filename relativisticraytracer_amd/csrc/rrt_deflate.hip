/*
 * rrt_deflate.hip -- librrt_deflate.so (include/rrt_deflate.h): raw deflate streams on the device.  Three kernels, one after the other
 * on the caller's stream:
 *
 *   deflate_segments   a workgroup of RRT_DEFLATE_THREADS per segment runs dfl_fragment of rrt_deflate_core.h, the definition, over a
 *                      DeflateWork in LDS (79 KB: two workgroups per CU): the segment staged from 16-byte loads, the run scans, the
 *                      histogram (LDS atomics), the ranking of the used symbols by every thread, the two-queue merge on one lane,
 *                      the codes, the header's size, a prefix sum of the chunks' bit counts, the stored-or-dynamic decision, and the
 *                      bits -- whole words stored, shared words OR-ed.  The fragment leaves LDS in aligned 16-byte stores for its
 *                      slot in the scratch; its length goes into the scratch's length table.
 *   deflate_offsets    one workgroup: the exclusive prefix sum of the lengths, and the streams' sizes.
 *   deflate_gather     a workgroup per segment copies the fragment to its place in d_out, byte-exactly: aligned 16-byte stores built
 *                      from two aligned 16-byte loads of the slot, single bytes only in the destination words the fragment's ends cut.
 */
#include <hip/hip_runtime.h>

#include <stdio.h>
#include <string.h>

#include "../../include/rrt_deflate.h"
#include "rrt_deflate_core.h"

/* ---- device ------------------------------------------------------------------------------------------------------------------- */

struct DflDeviceThreads {
    template <class F>
    __device__ __forceinline__ void run(F f) {
        f((int)threadIdx.x);
        __syncthreads();
    }
};

static __global__ __launch_bounds__(kDflThreads) void deflate_segments(uint8_t* __restrict__ scratch, const void* __restrict__ src, DeflatePlan p) {
    __shared__ DeflateWork w;
    const uint64_t g = blockIdx.x;
    const DeflateSeg s = dfl_segment(p, src, g);
    DflDeviceThreads x;
    dfl_fragment(x, w, s);
    const uint32_t len = w.frag_len;
    DflQuad* slot = reinterpret_cast<DflQuad*>(scratch + dfl_slot_offset(p, g, s.off));
    const DflQuad* from = reinterpret_cast<const DflQuad*>(w.bits);
    for (uint32_t q = threadIdx.x; q < (len + 15u) / 16u; q += (uint32_t)kDflThreads) slot[q] = from[q];
    if (threadIdx.x == 0) reinterpret_cast<uint32_t*>(scratch)[g] = len;
}

static __global__ __launch_bounds__(kDflThreads) void deflate_offsets(uint32_t* __restrict__ sizes, uint8_t* __restrict__ scratch, DeflatePlan p) {
    __shared__ uint32_t part[kDflThreads];
    const uint32_t* lens = reinterpret_cast<const uint32_t*>(scratch);
    uint32_t* offs = reinterpret_cast<uint32_t*>(scratch) + p.n_segments;
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0u;
    for (uint64_t g0 = 0; g0 < p.n_segments; g0 += (uint64_t)kDflThreads) {
        const uint64_t g = g0 + tid;
        const uint32_t mine = g < p.n_segments ? lens[g] : 0u;
        uint32_t v = mine;
        part[tid] = v;
        __syncthreads();
        for (uint32_t off = 1u; off < (uint32_t)kDflThreads; off <<= 1) {
            const uint32_t add = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            v += add;
            part[tid] = v;
            __syncthreads();
        }
        if (g < p.n_segments) offs[g] = carry + v - mine;
        carry += part[kDflThreads - 1];
        __syncthreads();
    }
    /* the offsets were written by this workgroup: visible to it behind the barrier */
    for (uint64_t j = tid; j < p.n_streams; j += (uint64_t)kDflThreads) {
        const uint32_t a = offs[j * p.per_stream];
        const uint32_t b = j + 1u < p.n_streams ? offs[(j + 1u) * p.per_stream] : carry;
        sizes[j] = b - a;
    }
}

__device__ __forceinline__ uint32_t dfl_pick(uint32_t k, uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return k == 0u ? a : k == 1u ? b : k == 2u ? c : d; }

static __global__ __launch_bounds__(kDflThreads) void deflate_gather(uint8_t* __restrict__ out, const uint8_t* __restrict__ scratch, DeflatePlan p) {
    const uint64_t g = blockIdx.x;
    const DeflateSeg s = dfl_segment(p, nullptr, g);
    const uint32_t* table = reinterpret_cast<const uint32_t*>(scratch);
    const uint32_t len = table[g];
    uint8_t* dst = out + table[p.n_segments + g];
    const uint8_t* slot = scratch + dfl_slot_offset(p, g, s.off);
    const uint32_t A = (uint32_t)((uintptr_t)dst & 15u);         /* destination word q holds the fragment's bytes 16 q - A ... 16 q - A + 15 */
    const uint32_t sh = (16u - A) & 15u, ws = sh >> 2, bs = (sh & 3u) * 8u;
    const uint32_t nq = (A + len + 15u) / 16u;
    for (uint32_t q = threadIdx.x; q < nq; q += (uint32_t)kDflThreads) {
        const int64_t i0 = 16 * (int64_t)q - (int64_t)A;
        /* the two aligned words of the slot around byte i0; with A > 0 the first one of q = 0 lies in front of the slot, inside the
         * scratch (the tables are there at the least), and none of its bytes is used */
        const int64_t f = i0 >= 0 ? (i0 & ~(int64_t)15) : -16;
        const DflQuad lo = *reinterpret_cast<const DflQuad*>(slot + f), hi = *reinterpret_cast<const DflQuad*>(slot + f + 16);
        uint32_t a[5], v[4];
        a[0] = dfl_pick(ws, lo.x, lo.y, lo.z, lo.w);
        a[1] = dfl_pick(ws, lo.y, lo.z, lo.w, hi.x);
        a[2] = dfl_pick(ws, lo.z, lo.w, hi.x, hi.y);
        a[3] = dfl_pick(ws, lo.w, hi.x, hi.y, hi.z);
        a[4] = dfl_pick(ws, hi.x, hi.y, hi.z, hi.w);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = bs ? (a[k] >> bs) | (a[k + 1] << (32u - bs)) : a[k];
        uint8_t* d = dst + i0;
        if (i0 >= 0 && i0 + 16 <= (int64_t)len) {
            DflQuad t = {v[0], v[1], v[2], v[3]};
            *reinterpret_cast<DflQuad*>(d) = t;
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (i0 + k >= 0 && i0 + k < (int64_t)len) d[k] = (uint8_t)(v[k >> 2] >> ((k & 3) * 8));
        }
    }
}

/* ---- C ABI ----------------------------------------------------------------------------------------------------------------------- */

#define RRT_DEFLATE_EXPORT extern "C" __attribute__((visibility("default")))

RRT_DEFLATE_EXPORT int rrt_deflate_plan(size_t n, size_t stream_bytes, size_t* n_streams, size_t* n_segments, size_t* out_bound, size_t* scratch_bytes) {
    DeflatePlan p;
    const int rc = dfl_plan(n, stream_bytes, 0, p);
    if (rc != RRT_OK) return rc;
    if (n_streams) *n_streams = (size_t)p.n_streams;
    if (n_segments) *n_segments = (size_t)p.n_segments;
    if (out_bound) *out_bound = (size_t)dfl_out_bound(p);
    if (scratch_bytes) *scratch_bytes = (size_t)dfl_scratch_bytes(p);
    return RRT_OK;
}

RRT_DEFLATE_EXPORT int rrt_deflate_launch_geometry(size_t n, size_t stream_bytes, size_t address_bits, int32_t out[12]) {
    DeflatePlan p;
    const int rc = dfl_plan(n, stream_bytes, 0, p);
    if (rc != RRT_OK) return rc;
    if (!out) return dfl_refuse("out is NULL");
    dfl_geometry(p, address_bits, out);
    return RRT_OK;
}

RRT_DEFLATE_EXPORT int rrt_deflate_code_lengths_host(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths_out, int32_t* halvings) {
    return dfl_code_lengths(counts, n_symbols, limit, lengths_out, halvings);
}

RRT_DEFLATE_EXPORT int rrt_launch_deflate(void* d_out, uint32_t* d_stream_sizes, void* d_scratch, const void* d_src, size_t n, size_t stream_bytes, int finish, void* stream) {
    DeflatePlan p;
    const int rc = dfl_plan(n, stream_bytes, finish, p);
    if (rc != RRT_OK) return rc;
    if (!d_out || !d_stream_sizes || !d_scratch || (!d_src && n != 0)) return dfl_refuse("d_out, d_stream_sizes, d_scratch or d_src is NULL");
    const uintptr_t out = (uintptr_t)d_out, tab = (uintptr_t)d_stream_sizes, scr = (uintptr_t)d_scratch, in = (uintptr_t)d_src;
    if ((tab & 3u) != 0) return dfl_refuse("d_stream_sizes is not 4-byte aligned");
    if ((scr & 15u) != 0) return dfl_refuse("d_scratch is not 16-byte aligned");
    const uint64_t out_b = dfl_out_bound(p), tab_b = 4u * p.n_streams, scr_b = dfl_scratch_bytes(p);
    if (n != 0 && (dfl_overlap(out, out_b, in, n) || dfl_overlap(tab, tab_b, in, n) || dfl_overlap(scr, scr_b, in, n))) return dfl_refuse("an output overlaps the input");
    if (dfl_overlap(out, out_b, tab, tab_b) || dfl_overlap(out, out_b, scr, scr_b) || dfl_overlap(tab, tab_b, scr, scr_b)) return dfl_refuse("the outputs overlap each other");
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* scratch = static_cast<uint8_t*>(d_scratch);
    const dim3 grid((uint32_t)p.n_segments), block((uint32_t)kDflThreads);
    hipLaunchKernelGGL(deflate_segments, grid, block, 0, st, scratch, d_src, p);
    hipLaunchKernelGGL(deflate_offsets, dim3(1), block, 0, st, d_stream_sizes, scratch, p);
    hipLaunchKernelGGL(deflate_gather, grid, block, 0, st, static_cast<uint8_t*>(d_out), scratch, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        snprintf(g_dfl_err, sizeof(g_dfl_err), "deflate: %s", hipGetErrorString(e));
        return RRT_ERR_HIP;
    }
    return RRT_OK;
}

RRT_DEFLATE_EXPORT int rrt_deflate_host(void* out, uint32_t* stream_sizes, const void* src, size_t n, size_t stream_bytes, int finish, size_t* total) {
    return dfl_host(out, stream_sizes, src, n, stream_bytes, finish, total);
}

RRT_DEFLATE_EXPORT const char* rrt_deflate_last_error(void) { return g_dfl_err; }
