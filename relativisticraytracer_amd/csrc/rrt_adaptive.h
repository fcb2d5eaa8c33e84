/*
 * rrt_adaptive.h -- adaptive supersampling (include/rrt.h: rrt_launch_raymarch_adaptive has the contract): which pixels of a stored
 * RGBA8 frame are REFINED, as ONE __host__ __device__ function -- adaptive_mask runs it on the device, rrt_adaptive_mask
 * (rrt_hip.hip's C ABI) on the host, so the tests can demand that the host query and the device list agree -- and the pass that
 * compacts the refined pixels' frame indices into the caller's scratch.  The rule is integer arithmetic on stored bytes: there is
 * nothing to round.  refine_pixels, the pass that re-renders the listed pixels, is in rrt_kernels.h beside the sampled kernels
 * whose pieces it uses.
 *
 * A SECTION of rrt_hip.hip, included by rrt_kernels.h inside its anonymous namespace.
 */
#ifndef RRT_ADAPTIVE_H
#define RRT_ADAPTIVE_H

/* The caller's scratch: the count of refined pixels (one uint32; the 12 bytes behind it are zeroed with it and otherwise unused),
 * then from kAdaptiveListOffset on the refined pixels' frame indices (uint32, stored row * width + x), at most width*height. */
constexpr size_t kAdaptiveListOffset = 16;
inline size_t adaptive_scratch(int width, int height) {
    return (kAdaptiveListOffset + (size_t)width * (size_t)height * sizeof(uint32_t) + 15) & ~(size_t)15;
}

/* pixel i of a stored RGBA8 frame as one little-endian word (r in the low byte); the device's frames are uchar4 arrays, a host
 * caller's bytes may sit anywhere */
__host__ __device__ __forceinline__ uint32_t adaptive_texel(const uint8_t* frame, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return reinterpret_cast<const uint32_t*>(frame)[i];
#else
    const uint8_t* p = frame + 4 * i;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
#endif
}

/* max over r, g, b of |p - q|; alpha is not looked at */
__host__ __device__ __forceinline__ int adaptive_gap(uint32_t p, uint32_t q) {
    int gap = 0;
    for (int c = 0; c < 24; c += 8) {
        const int d = (int)((p >> c) & 255u) - (int)((q >> c) & 255u);
        const int ad = d < 0 ? -d : d;
        gap = ad > gap ? ad : gap;
    }
    return gap;
}

/* Is pixel (x, row) of the stored width x height frame refined at threshold T: does it differ from its left, right, upper or lower
 * neighbour by more than T in a colour channel.  Coordinates clamp at the frame's edge (a clamped neighbour is the pixel itself:
 * gap 0), no wrap.  Symmetric in the two pixels of a pair, so the stored frame's bottom-up rows need no flip. */
__host__ __device__ __forceinline__ bool adaptive_refined(const uint8_t* frame, int width, int height, int x, int row, int T) {
    const size_t i = (size_t)row * width + x;
    const uint32_t p = adaptive_texel(frame, i);
    const uint32_t l = adaptive_texel(frame, x > 0 ? i - 1 : i), r = adaptive_texel(frame, x + 1 < width ? i + 1 : i);
    const uint32_t u = adaptive_texel(frame, row > 0 ? i - width : i), d = adaptive_texel(frame, row + 1 < height ? i + width : i);
    return adaptive_gap(p, l) > T || adaptive_gap(p, r) > T || adaptive_gap(p, u) > T || adaptive_gap(p, d) > T;
}

/* The mask pass: one lane per pixel of the stored base frame, a wavefront per 8x8 pixel tile, the tiles in scan order (four to a
 * workgroup).  The wave's refined lanes are compacted by ballot and popcount: its first refined lane reserves the wave's range of
 * the list with ONE atomic add on the counter, every refined lane writes its frame index at its prefix.  Which wave reserves first
 * is up to the hardware -- the list's order is not part of the contract -- but a wave's entries are consecutive and come from one
 * tile, so the pixels refine_pixels packs into a wavefront stay neighbours.  The counter was zeroed by zero_words in front of this
 * launch; at most width*height indices are written, which is what the scratch holds. */
constexpr int kMaskTile = 8, kMaskWaves = 4;
__global__ __launch_bounds__(64 * kMaskWaves) void adaptive_mask(const uint8_t* frame, int width, int height, int T,
                                                                unsigned* count, unsigned* list) {
    const int lane = threadIdx.x & 63;
    const unsigned tiles_x = (unsigned)(width + kMaskTile - 1) / kMaskTile, tiles_y = (unsigned)(height + kMaskTile - 1) / kMaskTile;
    const unsigned tile = blockIdx.x * (unsigned)kMaskWaves + (threadIdx.x >> 6);
    const unsigned ty = tile / tiles_x, tx = tile - ty * tiles_x;
    if (ty >= tiles_y) return;                                    /* wave-uniform: the last workgroup's spare waves */
    const int x = (int)tx * kMaskTile + (lane & (kMaskTile - 1)), row = (int)ty * kMaskTile + lane / kMaskTile;
    const bool refined = x < width && row < height && adaptive_refined(frame, width, height, x, row, T);
    const unsigned long long m = __ballot(refined);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    unsigned base = 0u;
    if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(m));
    base = (unsigned)__shfl((int)base, leader);
    if (refined) list[base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = (unsigned)row * (unsigned)width + (unsigned)x;
}

/* what refine_pixels needs beside the virtual frame's FrameArgs: the list the mask pass left and the frame's HDR plane */
struct RefineArgs {
    const unsigned* count;
    const unsigned* list;
    float4* hdr_out;        /* may be NULL */
    int s;
};

#endif /* RRT_ADAPTIVE_H */
