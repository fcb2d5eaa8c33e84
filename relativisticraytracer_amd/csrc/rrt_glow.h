/*
 * rrt_glow.h -- the gfx950 kernels of the HDR glow (rrt_launch_glow, include/rrt.h): a soft-knee bright pass and L separable
 * Gaussian lobes, added back onto the frame's HDR and tone-mapped.  A SECTION of rrt_hip.hip like rrt_kernels.h (included after it:
 * tone_map / store_rgba8 are the march's own).
 *
 *   glow_load_weights   copies a slice of the host-computed taps (by-value kernel argument) into the scratch's weight table
 *   glow_hpass<M>       one workgroup per row segment: stages the segment and its halo in LDS with the bright pass applied on
 *                       load, then runs every lobe's horizontal pass from it into the scratch planes U_l
 *   glow_vpass<M>       lanes along x (one 1 KiB row read per tap), each lane M consecutive rows of a column: every lobe's
 *                       vertical pass, the lobe sum, the composite onto H, the tone map and the RGBA8 store
 *
 * Both passes keep a register sliding window: a lane owns M consecutive outputs, visits its M + 2R inputs once in ascending
 * order and adds input jp to output m with tap jp - m.  Every output's terms therefore arrive in ascending k, which is the
 * order the contract fixes, and the tap index is the same in every lane, so the weights are wave-uniform (scalar loads).
 */
#ifndef RRT_GLOW_H
#define RRT_GLOW_H

constexpr int kGlowMaxLobes = 4;
constexpr int kGlowMaxRadius = 1024;
constexpr int kGlowM = 16;                       /* outputs per lane, both passes */
constexpr int kGlowU = 8;                        /* inputs per chunk of the window's steady middle */
constexpr int kGlowHThreads = 128;               /* glow_hpass: a segment is at most kGlowHThreads * kGlowM outputs of a row */
constexpr int kGlowLdsBytes = 64 * 1024;         /* glow_hpass' staged segment + halo stays within the default dynamic LDS */
constexpr int kGlowVWaves = 4;                   /* glow_vpass: waves per workgroup, each kGlowM rows of the same 64 columns */
constexpr int kGlowWeightChunk = 960;            /* floats per glow_load_weights launch: the argument stays under 4 KiB */

struct GlowArgs {
    const float4* hdr;         /* H, w*h, bottom-up rows (rgb read) */
    float4* planes;            /* U_l = planes + l*w*h: the horizontal passes' results (alpha unused) */
    const float* weights;      /* lobe l's 2 R_l + 1 taps at weights + woff[l] */
    uchar4* out;
    int width, height, lobes, rmax;
    int seg;                   /* glow_hpass' outputs per segment (a multiple of kGlowM): glow_seg(rmax) */
    int radius[kGlowMaxLobes], woff[kGlowMaxLobes];
    float threshold, scale;    /* T; s = intensity / (float)L */
};

struct GlowWeightChunk {
    float w[kGlowWeightChunk];
    int offset, count;
};

__global__ __launch_bounds__(256) void glow_load_weights(float* __restrict__ dst, GlowWeightChunk c) {
    for (int i = threadIdx.x; i < c.count; i += blockDim.x) dst[c.offset + i] = c.w[i];
}

/* the soft-knee bright pass: luma in the reference's dot order, B = rgb * ((luma - T) / luma) above T, else 0 */
__device__ __forceinline__ float4 glow_bright(float4 h, float t) {
    const float luma = (h.x * 0.2126f + h.y * 0.7152f) + h.z * 0.0722f;
    if (!(luma > t)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float f = (luma - t) / luma;
    return make_float4(h.x * f, h.y * f, h.z * f, 0.0f);
}

/* acc[m] = acc[m] + w[jp - m] * x for every m whose window holds input jp (0 <= jp - m <= 2R): the window's two ramps */
template <int M>
__device__ __forceinline__ void glow_tap_edge(float (&ar)[M], float (&ag)[M], float (&ab)[M], const float* __restrict__ w, int jp,
                                              int r2, float4 x) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if (m <= jp && jp - m <= r2) {
            const float wk = w[jp - m];
            ar[m] = ar[m] + wk * x.x;
            ag[m] = ag[m] + wk * x.y;
            ab[m] = ab[m] + wk * x.z;
        }
    }
}

/* One lane's window: inputs jp = 0 ... M + 2R - 1 (load(jp)) into outputs m = 0 ... M - 1, output m's taps in ascending k.
 * In the steady middle (M - 1 <= jp <= 2R) every output takes every input; there the inputs go in chunks of kGlowU, whose
 * M + kGlowU - 1 weights are loaded once (wave-uniform: scalar loads) and whose loads are all issued before the arithmetic. */
template <int M, class Load>
__device__ __forceinline__ void glow_window(float (&ar)[M], float (&ag)[M], float (&ab)[M], const float* __restrict__ w, int r2,
                                            Load load) {
#pragma unroll
    for (int m = 0; m < M; ++m) { ar[m] = 0.0f; ag[m] = 0.0f; ab[m] = 0.0f; }
    const int n = M + r2;
    int jp = 0;
    for (; jp < M - 1; ++jp) glow_tap_edge<M>(ar, ag, ab, w, jp, r2, load(jp));
    for (; jp + kGlowU - 1 <= r2; jp += kGlowU) {
        float wv[M + kGlowU - 1];                  /* wv[t] = w[jp - (M - 1) + t]: input jp + u, output m takes wv[u - m + M - 1] */
#pragma unroll
        for (int t = 0; t < M + kGlowU - 1; ++t) wv[t] = w[jp - (M - 1) + t];
        float4 x[kGlowU];
#pragma unroll
        for (int u = 0; u < kGlowU; ++u) x[u] = load(jp + u);
#pragma unroll
        for (int u = 0; u < kGlowU; ++u) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float wk = wv[u - m + M - 1];
                ar[m] = ar[m] + wk * x[u].x;
                ag[m] = ag[m] + wk * x[u].y;
                ab[m] = ab[m] + wk * x[u].z;
            }
        }
    }
    for (; jp < n; ++jp) glow_tap_edge<M>(ar, ag, ab, w, jp, r2, load(jp));
}

/* LDS slot of staged input e: one float4 of padding after every kGlowM, so that lanes kGlowM inputs apart fall on distinct
 * 16-byte bank slots for ds_read_b128 (stride 17 float4) */
__device__ __forceinline__ int glow_slot(int e) { return e + e / kGlowM; }

/* the LDS a segment of `seg` outputs and its halo take */
__host__ __device__ inline size_t glow_hpass_lds(int seg, int rmax) {
    const int n = seg + 2 * rmax;
    return (size_t)(n + n / kGlowM + 1) * sizeof(float4);
}
/* the widest segment (kGlowHThreads * kGlowM, halved while needed) whose LDS fits kGlowLdsBytes */
inline int glow_seg(int rmax) {
    int seg = kGlowHThreads * kGlowM;
    while (seg > kGlowM && glow_hpass_lds(seg, rmax) > (size_t)kGlowLdsBytes) seg /= 2;
    return seg;
}

/* grid ceil(width / seg) * height (segment fastest), block kGlowHThreads, dynamic LDS glow_hpass_lds(seg, rmax) */
template <int M>
__global__ __launch_bounds__(kGlowHThreads) void glow_hpass(GlowArgs a) {
    extern __shared__ float4 row[];
    const int w = a.width, n_seg = (w + a.seg - 1) / a.seg;
    const int y = blockIdx.x / n_seg;
    const int x0 = (blockIdx.x - y * n_seg) * a.seg;
    const int seg = min(a.seg, w - x0);
    const int n_in = ((seg + M - 1) / M) * M + 2 * a.rmax;
    const float4* src = a.hdr + (size_t)y * w;
    for (int e = threadIdx.x; e < n_in; e += kGlowHThreads) {
        const int x = min(max(x0 - a.rmax + e, 0), w - 1);
        row[glow_slot(e)] = glow_bright(src[x], a.threshold);
    }
    __syncthreads();
    const int base = threadIdx.x * M;
    if (base >= seg) return;
    for (int l = 0; l < a.lobes; ++l) {
        const int r = a.radius[l], r2 = 2 * r;
        const float* __restrict__ wl = a.weights + a.woff[l];
        float ar[M], ag[M], ab[M];
        const int e0 = base + a.rmax - r;
        glow_window<M>(ar, ag, ab, wl, r2, [&](int jp) { return row[glow_slot(e0 + jp)]; });
        float4* dst = a.planes + (size_t)l * w * a.height + (size_t)y * w + x0 + base;
#pragma unroll
        for (int m = 0; m < M; ++m)
            if (base + m < seg) dst[m] = make_float4(ar[m], ag[m], ab[m], 0.0f);
    }
}

/* grid ceil(height / (kGlowVWaves M)) * ceil(width / 64), block (64, kGlowVWaves): consecutive workgroups walk up one
 * 64-column strip, so the rows their windows share are still in the cache */
template <int M>
__global__ __launch_bounds__(64 * kGlowVWaves) void glow_vpass(GlowArgs a) {
    const int w = a.width, h = a.height, n_yb = (h + kGlowVWaves * M - 1) / (kGlowVWaves * M);
    const int strip = blockIdx.x / n_yb;
    const int x = strip * 64 + threadIdx.x;
    const int y0 = ((blockIdx.x - strip * n_yb) * kGlowVWaves + threadIdx.y) * M;
    if (y0 >= h) return;
    const int xc = min(x, w - 1);                /* lanes past the right edge march along and store nothing */
    float gr[M], gg[M], gb[M];
    for (int l = 0; l < a.lobes; ++l) {
        const int r = a.radius[l], r2 = 2 * r;
        const float* __restrict__ wl = a.weights + a.woff[l];
        const float4* __restrict__ u = a.planes + (size_t)l * w * h + xc;
        float ar[M], ag[M], ab[M];
        glow_window<M>(ar, ag, ab, wl, r2, [&](int jp) { return u[(size_t)min(max(y0 - r + jp, 0), h - 1) * w]; });
        if (l == 0) {
#pragma unroll
            for (int m = 0; m < M; ++m) { gr[m] = ar[m]; gg[m] = ag[m]; gb[m] = ab[m]; }
        } else {
#pragma unroll
            for (int m = 0; m < M; ++m) { gr[m] = gr[m] + ar[m]; gg[m] = gg[m] + ag[m]; gb[m] = gb[m] + ab[m]; }
        }
    }
    if (x >= w) return;
    const float s = a.scale;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        if (y0 + m < h) {
            const size_t i = (size_t)(y0 + m) * w + x;
            const float4 hv = a.hdr[i];
            float o_r, o_g, o_b;
            tone_map(mk(hv.x + gr[m] * s, hv.y + gg[m] * s, hv.z + gb[m] * s), o_r, o_g, o_b);
            store_rgba8(a.out, i, o_r, o_g, o_b);
        }
    }
}

#endif
