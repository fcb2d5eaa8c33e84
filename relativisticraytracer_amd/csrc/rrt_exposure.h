/*
 * rrt_exposure.h -- exposure control (include/rrt.h: rrt_launch_exposure has the contract): a frame's linear HDR scaled by
 * 2^ev, with ev given (manual) or metered from the frame's log-luminance histogram and adapted over time (auto), all on the device.
 *
 * Two parts.  The first is plain C++ the host and the device share, like projection_dir: the luma, the bin rule and the resolve
 * walk as RRT_FN functions -- rrt_exposure_meter_host (rrt_hip.hip's C ABI) and tests/exposure/exposure_exerciser.cpp run the very
 * source the kernels run.  The second, compiled by hipcc only, is the kernels: a SECTION of rrt_hip.hip like rrt_glow.h, included
 * after rrt_kernels.h (tone_map / store_rgba8 / zero_words are the march's own).
 *
 *   exposure_reset     zeroes the histogram and the state, loads the host-computed bin centres (by-value kernel argument)
 *   exposure_meter     grid-stride over the float4 pixels: a 256-bin histogram per wave in LDS (integer atomics; a wave whose
 *                      counted lanes share one bin adds its lane count once), summed per workgroup, one global integer atomic per
 *                      non-empty bin and workgroup
 *   exposure_resolve   one lane: the percentile cut, the mean log2 luminance in binary64, the target, the adapted ev, the scale
 *   exposure_apply     one lane per pixel: H.rgb * scale, the tone map, the RGBA8 store and, if asked for, the scaled HDR
 *
 * Only integer atomics: the histogram holds exact counts whatever order the adds arrive in, so every launch is reproducible.
 */
#ifndef RRT_EXPOSURE_H
#define RRT_EXPOSURE_H

constexpr int kExposureBins = 256;
constexpr int kExposureBinBias = 888;            /* (127 - 16) * 8: bin 0 starts at 2^-16 */

/* The caller's scratch (rrt_exposure_scratch_bytes; include/rrt.h documents the layout): the histogram, the state, the bin centres */
constexpr size_t kExposureHistOffset = 0;
constexpr size_t kExposureStateOffset = kExposureBins * sizeof(uint32_t);
struct ExposureState {
    float ev;                  /* the adapted EV, carried from frame to frame */
    uint32_t frames;           /* launches since the reset (saturating) */
    float scale;               /* rrt_expf(ev * ln 2): what exposure_apply multiplies by */
    float target;              /* diagnostics of the last launch: the clamped target (0 if nothing was metered), */
    uint64_t n;                /*   the metered pixels N, */
    double m;                  /*   the retained pixels' mean log2 luminance (0 if nothing was metered) */
    uint32_t reserved[8];
};
static_assert(sizeof(ExposureState) == 64, "the state's layout is part of include/rrt.h's contract");
constexpr size_t kExposureTableOffset = kExposureStateOffset + sizeof(ExposureState);
constexpr size_t kExposureScratchBytes = kExposureTableOffset + kExposureBins * sizeof(double);
static_assert(kExposureStateOffset % 16 == 0 && kExposureTableOffset % 16 == 0 && kExposureScratchBytes % 16 == 0, "16-byte sections");

/* what the resolve walk needs of rrt_exposure, the key already as log2(key) in double (host) */
struct ExposureMeter {
    double log2_key;
    float ev, min_ev, max_ev, adapt_up, adapt_down;
    int32_t low_permille, high_permille;
};

/* the glow's luma, in its association */
RRT_FN float exposure_luma(float r, float g, float b) { return (r * 0.2126f + g * 0.7152f) + b * 0.0722f; }

/* The bin of a luma, or -1 if it is not metered: only positive finite values count (subnormals included; zero, negatives, NaN and
 * infinity do not).  8 exponent bits and 3 mantissa bits of the float: 8 bins per octave, linear inside one, clamped to
 * [2^-16, 2^16).  Integer work on the bits: nothing to round. */
RRT_FN int exposure_bin(float luma) {
    const uint32_t u = rrt_f2u(luma);
    if (!(u > 0u && u < 0x7f800000u)) return -1;
    const int b = (int)(u >> 20) - kExposureBinBias;
    return b < 0 ? 0 : (b > kExposureBins - 1 ? kExposureBins - 1 : b);
}

/* bin b's centre in log2 units, in double (host: rrt_exposure_bin_ev and the table exposure_reset loads) */
static inline double exposure_bin_centre(int b) {
    const int e = (b + kExposureBinBias) >> 3, j = (b + kExposureBinBias) & 7;
    return (double)(e - 127) + std::log2(1.0 + ((double)j + 0.5) / 8.0);
}

RRT_FN float exposure_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

/* One frame's resolve, in the order include/rrt.h writes it: N, the two cuts, the retained counts' mean log2 luminance in binary64
 * (ascending bins from 0.0), the clamped target, the state's step, the scale.  Removing `lo` counts from the lowest bins upwards and
 * `hi` from the highest downwards leaves of bin b, whose counts are the pixels of rank [cum, cum + c_b) in luminance order, the
 * ranks inside [lo, N - hi).  lo + hi < N because the two per-mille values sum to less than 1000: at least one pixel is retained. */
RRT_FN void exposure_resolve_step(const uint32_t* hist, const double* table, const ExposureMeter& s, ExposureState& st) {
    uint64_t n = 0;
    for (int b = 0; b < kExposureBins; ++b) n += hist[b];
    double m = 0.0;
    float target = 0.0f, ev = st.ev;
    if (n == 0) {
        if (st.frames == 0u) ev = exposure_clamp(s.ev, s.min_ev, s.max_ev);
    } else {
        const uint64_t lo = n * (uint64_t)s.low_permille / 1000u, end = n - n * (uint64_t)s.high_permille / 1000u;
        uint64_t cum = 0, kept = 0;
        double sum = 0.0;
        for (int b = 0; b < kExposureBins; ++b) {
            const uint64_t c = hist[b];
            const uint64_t from = cum > lo ? cum : lo, to = cum + c < end ? cum + c : end;
            const uint64_t r = to > from ? to - from : 0u;
            sum = sum + (double)r * table[b];
            kept += r;
            cum += c;
        }
        m = sum / (double)kept;
        target = exposure_clamp((float)(s.log2_key - m) + s.ev, s.min_ev, s.max_ev);
        if (st.frames == 0u) {
            ev = target;
        } else {
            const float alpha = target > ev ? s.adapt_up : s.adapt_down;
            ev = ev + (target - ev) * alpha;
        }
    }
    st.ev = ev;
    if (st.frames != 0xffffffffu) st.frames += 1u;
    st.scale = rrt_expf(ev * 0.693147182f);
    st.target = target;
    st.n = n;
    st.m = m;
}

#if defined(__HIPCC__)

struct ExposureTable {
    double ev[kExposureBins];
};

/* one workgroup of kExposureBins threads */
__global__ __launch_bounds__(256) void exposure_reset(uint8_t* scratch, ExposureTable t) {
    const int i = threadIdx.x;
    reinterpret_cast<uint32_t*>(scratch + kExposureHistOffset)[i] = 0u;
    if (i < (int)(sizeof(ExposureState) / sizeof(uint32_t))) reinterpret_cast<uint32_t*>(scratch + kExposureStateOffset)[i] = 0u;
    reinterpret_cast<double*>(scratch + kExposureTableOffset)[i] = t.ev[i];
}

/* The meter's grid comes from the chip, not from the frame: kMeterGroupsPerCU workgroups for each of gfx950's 256 CUs at most,
 * every wave striding over the frame in runs of kMeterRun * 64 consecutive pixels whose loads are all issued before the first is
 * counted.  A 4K frame is 32 pixels per lane; the workgroups' 256 final atomics each are what a larger grid would multiply. */
constexpr int kMeterWaves = 4, kMeterThreads = 64 * kMeterWaves, kMeterRun = 4;
constexpr int kMeterCUs = 256, kMeterGroupsPerCU = 4;
inline unsigned exposure_meter_groups(size_t n) {
    const size_t per_group = (size_t)kMeterThreads * kMeterRun;
    const size_t want = (n + per_group - 1) / per_group, cap = (size_t)kMeterCUs * kMeterGroupsPerCU;
    return (unsigned)(want < cap ? want : cap);
}

/* one pixel per lane into the wave's LDS histogram; every lane of the wave calls it (ballots) */
__device__ __forceinline__ void exposure_count(unsigned* mine, int lane, float4 h) {
    const int bin = exposure_bin(exposure_luma(h.x, h.y, h.z));
    const unsigned long long m = __ballot(bin >= 0);
    if (m == 0ull) return;
    /* flat regions: every counted lane in one bin -> one add of the lane count instead of up to 64 serialised ones */
    const int leader = __ffsll((long long)m) - 1;
    const int b0 = __shfl(bin, leader);
    if (__ballot(bin >= 0 && bin != b0) == 0ull) {
        if (lane == leader) atomicAdd(&mine[b0], (unsigned)__popcll(m));
    } else if (bin >= 0) {
        atomicAdd(&mine[bin], 1u);
    }
}

__global__ __launch_bounds__(kMeterThreads) void exposure_meter(const float4* __restrict__ hdr, size_t n, unsigned* __restrict__ hist) {
    __shared__ unsigned bins[kMeterWaves][kExposureBins];
    for (int i = threadIdx.x; i < kMeterWaves * kExposureBins; i += kMeterThreads) (&bins[0][0])[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned* mine = bins[wave];
    const size_t stride = (size_t)gridDim.x * kMeterThreads * kMeterRun;
    /* `base` is the wave's first pixel of the round: the trip count is the same in all 64 lanes.  A lane past the frame's end loads
     * the last pixel instead (no branch around a load: the run's loads are in flight together) and counts a luma of 0, which is
     * not metered. */
    for (size_t base = ((size_t)blockIdx.x * kMeterWaves + wave) * (64 * kMeterRun); base < n; base += stride) {
        float4 h[kMeterRun];
#pragma unroll
        for (int u = 0; u < kMeterRun; ++u) {
            const size_t i = base + (size_t)(u * 64 + lane);
            h[u] = hdr[i < n ? i : n - 1];
            if (i >= n) h[u].x = h[u].y = h[u].z = 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kMeterRun; ++u) exposure_count(mine, lane, h[u]);
    }
    __syncthreads();
    const int t = threadIdx.x;                                       /* kMeterThreads == kExposureBins: thread t owns bin t */
    unsigned sum = 0u;
#pragma unroll
    for (int w = 0; w < kMeterWaves; ++w) sum += bins[w][t];
    if (sum != 0u) atomicAdd(&hist[t], sum);
}
static_assert(kMeterThreads == kExposureBins, "exposure_meter's last step gives every bin one thread");

__global__ __launch_bounds__(64) void exposure_resolve(const unsigned* hist, ExposureState* state, const double* table, ExposureMeter s) {
    if (threadIdx.x != 0) return;
    ExposureState st = *state;
    exposure_resolve_step(hist, table, s, st);
    *state = st;
}

/* state != NULL (auto): the scale the resolve left, one wave-uniform load; else the host's scale by value (manual).  hdr_out may be
 * hdr_in: a lane reads its pixel before it writes it, and nobody else touches that pixel. */
__global__ __launch_bounds__(256) void exposure_apply(uchar4* out8, float4* hdr_out, const float4* hdr_in, size_t n,
                                                      const ExposureState* state, float scale_by_value) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float scale = state ? state->scale : scale_by_value;
    const float4 h = hdr_in[i];
    const float4 o = make_float4(h.x * scale, h.y * scale, h.z * scale, h.w);
    if (hdr_out) hdr_out[i] = o;
    if (out8) {
        float o_r, o_g, o_b;
        tone_map(mk(o.x, o.y, o.z), o_r, o_g, o_b);
        store_rgba8(out8, i, o_r, o_g, o_b);
    }
}

#endif /* __HIPCC__ */
#endif /* RRT_EXPOSURE_H */
