/*
 * rrt_device.h -- gfx950 device functions of the geodesic ray-march path.
 *
 * Hand-written for CDNA4; not a translation of the reference's CUDA headers.
 * Every function cites the reference lines whose RESULT it must reproduce.
 * Arithmetic contract (what makes the output bit-identical to the CPU oracle):
 *   - IEEE binary32 only, every source-level operation rounded once, in the
 *     reference's association order; the translation unit is compiled with
 *     -ffp-contract=off, so the only fused operations are the explicit fmaf()
 *     calls inside rrt_math.h (the portable transcendentals);
 *   - `/` and sqrtf are correctly rounded (hipcc default
 *     -fhip-fp32-correctly-rounded-divide-sqrt); where the hot loops replace them by cheaper sequences
 *     (sqrt_rsq, sqrt_seeded, div_seeded, rrt_div_tame) those give the same bits on the operands they are
 *     used for, and each is checked against the IEEE form on the GPU (rrt_selfcheck_*);
 *   - algebraic shortcuts are taken only where they are exact in binary32
 *     (x - 0 == x, 1*x == x, (0,1,0) x p == (p.z, 0, -p.x), fmod(x,1) ==
 *     x - trunc(x) up to the sign of a zero result, which no consumer observes).
 */
#ifndef RRT_DEVICE_H
#define RRT_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

/*
 * Correctly rounded a / b without hipcc's range scaling: v_rcp_f32 (1 ulp), one Newton refinement, then the
 * Markstein residual corrections -- the FMA core of LLVM's own f32 division, which is what `/` compiles to minus
 * v_div_scale / v_div_fmas / v_div_fixup.  Bit-identical to IEEE `/` whenever those would have been no-ops:
 * b normal with 2^-60 <= |b| <= 2^60, and a == 0 or 2^-60 <= |a / b| <= 2^60 ("tame" operands; checked on 2^32
 * random tame pairs, tests/test_gpu_units.py).  10 issue slots instead of ~20.  Used only where the operand
 * ranges are known by construction -- each use says why.
 */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RRT_NO_LEAN)     /* -DRRT_NO_LEAN: A/B builds with hipcc's IEEE forms everywhere */
#ifndef RRT_TAME_DIV_ROUNDS
#define RRT_TAME_DIV_ROUNDS 2       /* the v_rcp seed is only good to 2^-23: keep both corrections here (cheap: the media) */
#endif
__device__ __forceinline__ float rrt_div_core(float a, float b, float seed) {
    float e = __builtin_fmaf(-b, seed, 1.0f);
    float y = __builtin_fmaf(e, seed, seed);
    float q = a * y;
    float r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
#if RRT_TAME_DIV_ROUNDS >= 2
    r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
#endif
    return q;
}
__device__ __forceinline__ float rrt_div_tame(float a, float b) { return rrt_div_core(a, b, __builtin_amdgcn_rcpf(b)); }
#define RRT_MATH_TAME_DIV(a, b) rrt_div_tame((a), (b))
/* y * 2^k, the tail of rrt_expf: one v_ldexp_f32 instead of two multiplies and the integer work that builds their
 * factors -- the same function (rrt_math.h: rrt_scale2), checked bit for bit down into the subnormal results by the
 * math-function unit tests. */
#define RRT_MATH_SCALE2(y, k) __builtin_ldexpf((y), (k))
#else
__host__ __device__ static inline float rrt_div_tame(float a, float b) { return a / b; }   /* host pass: never executed */
#endif

/*
 * a / B for a compile-time constant B (round 3): y = RN(1/B) is folded at compile time and is the CORRECTLY ROUNDED
 * reciprocal, which is exactly Markstein's hypothesis: q = RN(a*y) is a faithful quotient, r = a - B*q is exact in one
 * fma, and RN(q + r*y) is the correctly rounded a / B -- three instructions instead of the ten of rrt_div_tame (whose
 * v_rcp seed alone costs as much as the Newton step behind it).  Valid where nothing under- or overflows: callers pass
 * bounded dividends (each use site says so); rrt_selfcheck_div_const checks EVERY dividend of magnitude 2^[-40, 40) (and
 * +0) against IEEE `/` for every constant the media code divides by.  (A -0 dividend would return +0 for B > 0; the use
 * sites cannot produce one: their dividends are differences with non-zero literals, or radii / temperatures >= 1.)
 */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(RRT_NO_LEAN) && !defined(RRT_NO_CONST_DIV)
/* B must be a literal (or constexpr) at the call site: `1.0f / B` is then folded by the compiler, correctly rounded.
 * (With a run-time B this is still a / B exactly -- the reciprocal would be IEEE-divided at run time -- only slow.) */
__device__ __forceinline__ float rrt_div_const(float a, const float B) {
    const float y = 1.0f / B;
    const float q = a * y;
    const float r = __builtin_fmaf(-B, q, a);
    return __builtin_fmaf(r, y, q);
}
#else
__host__ __device__ static inline float rrt_div_const(float a, const float B) { return a / B; }
#endif

#include "rrt_math.h"

#ifndef RRT_PROBE
#define RRT_PROBE 0
#endif
#define RRT_DEV __device__ __forceinline__

namespace rrt {

/* ---- scene constants, reference include/config.h:18-48 (values verbatim) ---- */
constexpr float kDiskTempRef = 1.5e7f;      /* DISK_TEMP_REF    :18 */
constexpr float kEventHorizon = 2.0f;       /* EVENT_HORIZON    :29 */
constexpr float kIsco = 10.0f;              /* ISCO_RADIUS      :33 */
constexpr float kDiskOut = 25.0f;           /* DISK_OUT_M       :34 */
constexpr float kDiskH = 0.8f;              /* DISK_H_M         :35 */
constexpr float kDiskLum = 6.0f;            /* DISK_LUMINOSITY  :36 */
constexpr float kDiskOpacity = 0.4f;        /* DISK_OPACITY     :37 */
constexpr float kExposure = 0.8f;           /* EXPOSURE         :38 */
constexpr float kCloudH = 0.5f;             /* CLOUD_H_M        :41 */
constexpr float kCloudOut = 25.0f;          /* CLOUD_OUT_M      :42 */
constexpr float kCloudOpacity = 0.3f;       /* CLOUD_OPACITY    :43 */
constexpr float kCloudLum = 0.4f;           /* CLOUD_LUMINOSITY :44 */
constexpr float kStepSize = 0.3f;           /* STEP_SIZE_M      :47 */
constexpr float kPi = 3.1415926535f;        /* PI, math_utils.h:7 */

struct v3 { float x, y, z; };

RRT_DEV v3 mk(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
RRT_DEV float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }          /* math_utils.h:11 */
RRT_DEV v3 cross(v3 a, v3 b) {                                                       /* math_utils.h:15 */
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
RRT_DEV float length(v3 v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z); }      /* :19 */
RRT_DEV v3 normalize(v3 v) {                                                         /* :23-27 */
    float mag = length(v);
    if (mag < 1e-6f) return mk(0.f, 0.f, 0.f);
    return mk(v.x / mag, v.y / mag, v.z / mag);
}
RRT_DEV v3 add(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
RRT_DEV v3 mul(v3 v, float s) { return mk(v.x * s, v.y * s, v.z * s); }
RRT_DEV float lerp(float a, float b, float t) { return a + t * (b - a); }            /* :41 */
RRT_DEV float fmin2(float a, float b) { return __builtin_fminf(a, b); }
RRT_DEV float fmax2(float a, float b) { return __builtin_fmaxf(a, b); }
RRT_DEV float smoothstep(float e0, float e1, float x) {                              /* :45-48 */
    float t = fmin2(fmax2((x - e0) / (e1 - e0), 0.0f), 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

template <bool LEAN> RRT_DEV float smoothstep_t(float e0, float e1, float x);      /* below: needs rrt_div_tame */

/* fmodf(x, 1.0f) for finite x: exact, differs from libm only in the sign of a zero. */
RRT_DEV float fmod1(float x) { return x - __builtin_truncf(x); }

/* hash31, math_utils.h:91-96 -- arithmetic hash, must stay unfused. */
RRT_DEV float hash31(float px, float py, float pz) {
    float x = fmod1(px * 0.1031f), y = fmod1(py * 0.1031f), z = fmod1(pz * 0.1031f);
    float d = x * (y + 33.33f) + y * (z + 33.33f) + z * (x + 33.33f);
    x += d; y += d; z += d;
    return fmod1((x + y) * z);
}

/* noise3D, math_utils.h:98-110.  i + 0 == i and i + 1 are exact (|i| < 2^24). */
RRT_DEV float noise3d(v3 p) {
    float ix = floorf(p.x), iy = floorf(p.y), iz = floorf(p.z);
    float fx = p.x - ix, fy = p.y - iy, fz = p.z - iz;
    float ux = fx * fx * (3.0f - 2.0f * fx);
    float uy = fy * fy * (3.0f - 2.0f * fy);
    float uz = fz * fz * (3.0f - 2.0f * fz);
    /* "+ 0.0f" reproduces add(i, (0,0,0)): it turns a -0 lattice coordinate into +0 */
    float x0 = ix + 0.0f, y0 = iy + 0.0f, z0 = iz + 0.0f;
    float x1 = ix + 1.0f, y1 = iy + 1.0f, z1 = iz + 1.0f;
    float a = lerp(hash31(x0, y0, z0), hash31(x1, y0, z0), ux);
    float b = lerp(hash31(x0, y1, z0), hash31(x1, y1, z0), ux);
    float c = lerp(hash31(x0, y0, z1), hash31(x1, y0, z1), ux);
    float d = lerp(hash31(x0, y1, z1), hash31(x1, y1, z1), ux);
    return lerp(lerp(a, b, uy), lerp(c, d, uy), uz);
}

/* fbm, math_utils.h:112-121 */
template <int OCT>
RRT_DEV float fbm(v3 p) {
    float v = 0.0f, a = 0.5f;
#pragma unroll 1
    for (int i = 0; i < OCT; ++i) {
        v += a * noise3d(p);
        p = mk(p.x * 2.05f + 10.0f, p.y * 2.05f + 10.0f, p.z * 2.05f + 10.0f);
        a *= 0.5f;
    }
    return v;
}

/*
 * Lattice-hash table (rrt_noise_table, include/rrt.h).
 *
 * noise3D spends ~108 of its ~150 VALU instructions hashing the eight corners of the lattice cell, and
 * hash31 of a lattice point is a pure function of three integers.  For the noise calls whose cells are
 * shared by most lanes of a wavefront (the low octaves: a wave covers 8x8 neighbouring pixels, whose
 * sample points lie a few hundredths of a lattice cell apart) the corner values are READ instead, from a
 * dense table over the box of lattice points those calls can reach, built once by the same hash31 code
 * (so the bits are the same): the vector-memory pipe and the L1/L2, which the march leaves idle, take
 * over two thirds of the call's VALU work.  Measured (tools/noise_table_microbench.hip): 2.0-2.4x per
 * call while the wave's cells span a few cache lines, many times SLOWER when every lane has its own --
 * hence the wave-uniform gate (lut_spread / lut_fits) in front of every table call.
 *
 * Record of lattice point (x, y, z), 16 bytes:
 *   { H(x,y,z),  H(x+1,y,z) - H(x,y,z),  H(x,y+1,z),  H(x+1,y+1,z) - H(x,y+1,z) }
 * so that lerp(H(x..), H(x+1..), t) = a + t*(b - a) of math_utils.h:41 keeps its three roundings: the
 * stored difference is the rounded (b - a).  A cell needs the records (x,y,z) and (x,y,z+1).
 * Layout [z][y][x]; `origin` folds the box origin into one constant; `last` clamps the index so that a
 * read can never leave the allocation (the host proves the box covers every reachable cell for the
 * launch's `time`, tests count violations in debug launches).
 */
struct NoiseLut {
    const float4* cells;
    int origin;            /* (z0*ny + y0)*nx + x0 */
    int nx, nxy;
    unsigned last;         /* n_cells - nxy - 1 */
    unsigned families;     /* which call families the box was sized for: ANDed into the callers' `from_table` words */
};

struct LutTap { float4 q0, q1; float ux, uy, uz; };
/* first half of a table lookup: the two 16-byte loads are issued, nothing waits on them */
RRT_DEV LutTap lut_fetch(const NoiseLut& L, v3 p, unsigned* oob) {
    LutTap t;
    float ix = floorf(p.x), iy = floorf(p.y), iz = floorf(p.z);
    float fx = p.x - ix, fy = p.y - iy, fz = p.z - iz;
    t.ux = fx * fx * (3.0f - 2.0f * fx);
    t.uy = fy * fy * (3.0f - 2.0f * fy);
    t.uz = fz * fz * (3.0f - 2.0f * fz);
    const int cx = (int)ix, cy = (int)iy, cz = (int)iz;
    const unsigned want = (unsigned)(__mul24(cz, L.nxy) + __mul24(cy, L.nx) + cx - L.origin);
    unsigned idx = want < L.last ? want : L.last;
    if (oob && want > L.last) atomicAdd(oob, 1u);
#if defined(RRT_PROBE) && (RRT_PROBE & 16)     /* timing probe (wrong pixels): every lane reads the FIRST lane's cell -- one line per load, what a
                                                 * perfectly coalesced / LDS-broadcast lookup could cost at best */
    idx = (unsigned)__builtin_amdgcn_readfirstlane((int)idx);
#endif
    const char* base = reinterpret_cast<const char*>(L.cells);
    t.q0 = *reinterpret_cast<const float4*>(base + (size_t)(idx << 4));
    t.q1 = *reinterpret_cast<const float4*>(base + (size_t)((idx + (unsigned)L.nxy) << 4));
    return t;
}
RRT_DEV float lut_blend(const LutTap& t) {
    float a = t.q0.x + t.ux * t.q0.y;
    float b = t.q0.z + t.ux * t.q0.w;
    float c = t.q1.x + t.ux * t.q1.y;
    float d = t.q1.z + t.ux * t.q1.w;
    return lerp(lerp(a, b, t.uy), lerp(c, d, t.uy), t.uz);
}
RRT_DEV float noise3d_lut(const NoiseLut& L, v3 p, unsigned* oob) { return lut_blend(lut_fetch(L, p, oob)); }

/*
 * BANDED layout of the fine dust families (round 5; rrt_noise_table with RRT_TABLE_BANDED, MEDIA == 3 in the kernels).
 * The dust coordinates shear with time * omega(rc), omega = (10/rc)^1.5 in [0.253, 1] (densities.h:88-93: differential
 * rotation), so the z extent of ONE dense box over all radii grows like 0.75 t0 and is unaddressable at full coverage a few
 * minutes into the reference's unbounded clock (main.cpp:515) -- although a sample only ever touches the z range of ITS OWN
 * radius.  The three families that dominate the volume (ridge octaves 1 and 2 at 2.1 and 4.41 cells per unit, the detail
 * octave at 4.0) therefore get one small dense box per BAND of omega: a sample picks its band from its own omega (which it
 * has: `kepler`), reads that band's box geometry (one 32-byte record per family, a per-lane load that hits L1), and looks
 * its cells up exactly as before.  Bands are uniform in omega, which makes their z extents equal (width ~ t * d omega).
 * [495, 505 s] at full coverage: unaddressable dense (3.4 GB for ridge octave 2 alone), ~1.5 GB banded.  Same bits: the
 * records are the same hash31 values.  The coarse families (both warps, ridge octave 0) stay in the one dense box.
 */
struct BandLut { unsigned cell0; int origin; int nx, nxy; unsigned last; unsigned pad[3]; };      /* 32 bytes */
struct DustBands {
    const BandLut* entries;        /* [family 0..2][band]; family 0 = ridge octave 1, 1 = ridge octave 2, 2 = detail octave 0;
                                      then kLutAccOctaves records: the ACCRETION table's octaves, one box each (below) */
    int n_bands;
    float w_min, w_scale;          /* band = clamp((int)((omega - w_min) * w_scale), 0, n_bands - 1) */
};
constexpr int kBandFamilies = 3;
/* The same layout splits the accretion table by OCTAVE: its y coordinate drifts with 0.35 t and fbm scales it by 2.05 per
 * octave (densities.h:44-54, math_utils.h:116), so at t = 500 s the four table-served octaves sit at y ~ 175, 370, 770 and
 * 1580 -- one box over all of them is 1 500 cells tall (0.96 GB) where each octave needs at most 160 (0.1 GB together). */
RRT_DEV int dust_band(const DustBands& B, float omega) {
    const int b = (int)((omega - B.w_min) * B.w_scale);
    return b < 0 ? 0 : (b >= B.n_bands ? B.n_bands - 1 : b);
}
/* the box of (family, band) as a NoiseLut whose fields are per-lane values; `table` = the allocation's first cell */
RRT_DEV NoiseLut record_lut(const float4* table, const BandLut& e, unsigned families) {
    NoiseLut L;
    L.cells = table + e.cell0;
    L.origin = e.origin; L.nx = e.nx; L.nxy = e.nxy; L.last = e.last; L.families = families;
    return L;
}
RRT_DEV NoiseLut band_lut(const NoiseLut& acc0, const NoiseLut& dust, const DustBands& B, int family, int band) {
    return record_lut(acc0.cells, B.entries[family * B.n_bands + band], dust.families);    /* acc0.cells: the table starts with accretion octave 0 */
}
RRT_DEV NoiseLut acc_octave_lut(const NoiseLut& acc0, const DustBands& B, int octave) {
    return record_lut(acc0.cells, B.entries[kBandFamilies * B.n_bands + octave], acc0.families);
}

/* Per-lane distance (in lattice cells at scale 1, x weighted 1/4: a 128-byte line holds 8 x-neighbours) of
 * this lane's noise-space point from the first active lane's; lut_fits(spread, s) is wave-uniform: at `s`
 * cells per unit all active lanes stay within kLutCells cells of each other. */
#ifndef RRT_LUT_CELLS
#define RRT_LUT_CELLS 12.0f
#endif
constexpr float kLutCells = RRT_LUT_CELLS;
RRT_DEV float lut_spread(v3 c) {
    const float fx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(c.x)));
    const float fy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(c.y)));
    const float fz = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(c.z)));
    return __builtin_fmaxf(__builtin_fmaxf(fabsf(c.x - fx) * 0.25f, fabsf(c.y - fy)), fabsf(c.z - fz));
}
RRT_DEV bool lut_fits(float spread, float cells_per_unit) { return __all(spread * cells_per_unit <= kLutCells); }

/*
 * Correctly rounded sqrt and divide for the march loop.
 *
 * hipcc's own expansions of sqrtf and `/` are correctly rounded too, but carry range
 * scaling (v_div_scale / v_div_fixup / denormal rescue) that this loop never needs and
 * that costs ~19-21 issue slots each on gfx950 (profiles/r01_valu_microbench.txt).  The
 * operands here are tame (r in [1, 1.6e4], quotients normal or exactly zero -- a denormal
 * quotient would need a ray parallel to its position vector to within 1e-13 rad), so the
 * bare Newton/Markstein cores are enough; both are checked bit-for-bit against the hardware-IEEE forms over the whole
 * operand range on the GPU (tests/test_gpu_units.py::test_fast_sqrt_div_*).
 *
 *   sqrt_rsq:  y0 = v_rsq_f32(x) (1 ulp); one coupled Goldschmidt step for g ~ sqrt(x),
 *              h ~ 1/(2 sqrt(x)); final residual correction g + (x - g*g)*h.
 *   div_seeded: the FMA core of LLVM's f32 fdiv (refine the reciprocal once, then three
 *              residual corrections), started from a seed accurate to ~2^-20.
 */
RRT_DEV void sqrt_rsq(float x, float& root, float& inv_root) {
    float y0 = __builtin_amdgcn_rsqf(x);
    float g = x * y0;
    float h = 0.5f * y0;
    float r = __builtin_fmaf(-h, g, 0.5f);
    g = __builtin_fmaf(g, r, g);
    h = __builtin_fmaf(h, r, h);
    float d = __builtin_fmaf(-g, g, x);
    root = __builtin_fmaf(d, h, g);
    inv_root = h + h;
}

/*
 * The march's divide: refine the seed once (e, y), multiply, ONE Markstein residual correction (round 3; two before:
 * -DRRT_DIV_ROUNDS=2).  Why one is enough: the seed is good to ~2^-21, so y = seed + e*seed carries 2^-42 before its
 * own rounding and is the CORRECTLY ROUNDED reciprocal of b except when 1/b lies within 2^-42 of a rounding boundary
 * (probability ~2^-17); with a correctly rounded reciprocal and a faithful q, Markstein's theorem makes q + r*y the
 * correctly rounded quotient.  The second correction could only matter when that rare y meets a quotient within 2^-24
 * ulp of a rounding boundary (probability ~1e-7): a 1e-12 corner that the measurement does not even show --
 * rrt_selfcheck_div on 2^44 march-shaped operand sets (3.5e13 divides, tools/div_rounds_probe.py,
 * profiles/r03_div_rounds_probe.txt): ONE correction 2 mismatches, TWO corrections the same 2 mismatches, both on
 * denominators whose significand is within 5 ulp of 2 (0x4bfffffb: Markstein's known exception, where the refined
 * reciprocal itself is off and no number of residual corrections repairs it).  That floor, 5.7e-14 per divide = one
 * acceleration in ~250 4K frames, was already in round 2's build; VERDICT r02 asked for >= 2^34 clean cases.
 * THE DOCUMENTED EXCEPTION of "correctly rounded division" (round 4): a denominator whose significand lies an odd number
 * d <~ 11 of ulps below 2 has a reciprocal within d^2/4 * 2^-46 of a rounding tie, closer than the 2^-42 the once-refined
 * reciprocal carries; with a seed a few ulps off, y comes out one ulp low and the quotient with it.  Pinned as an expected
 * mismatch by tests/test_gpu_units.py::test_divide_known_exception_is_what_the_documents_say (0x33666662 / 0x4bfffffb, seed
 * 0x33000006); closing it would take two more instructions on each of the 8 divides of a step (5.6 %).  With seeds as the
 * march's own roots produce them: 0 mismatches in 2.2e13 divides (rrt_selfcheck_div_march, profiles/r04_div_march_seeds_probe.txt).
 */
#ifndef RRT_DIV_ROUNDS
#define RRT_DIV_ROUNDS 1
#endif
RRT_DEV float div_seeded(float a, float b, float seed) {
    float e = __builtin_fmaf(-b, seed, 1.0f);
    float y = __builtin_fmaf(e, seed, seed);
    float q = a * y;
    float r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
#if RRT_DIV_ROUNDS >= 2
    r = __builtin_fmaf(-b, q, a);
    q = __builtin_fmaf(r, y, q);
#endif
    return q;
}

/* sqrtf for operands in [2^-40, 2^64) (every float in that range checked against v_sqrt-based sqrtf) */
#ifdef RRT_NO_LEAN
RRT_DEV float sqrt_tame(float x) { return sqrtf(x); }
#else
RRT_DEV float sqrt_tame(float x) { float r, y; sqrt_rsq(x, r, y); return r; }
#endif

/* smoothstep (math_utils.h:45-48) with literal edges: the divisor e1 - e0 is a constant of magnitude 0.4 .. 5 and
 * the dividend a bounded difference, so the division is tame (a zero dividend gives the IEEE zero) */
template <bool LEAN>
RRT_DEV float smoothstep_t(float e0, float e1, float x) {
    const float q = LEAN ? rrt_div_const(x - e0, e1 - e0) : (x - e0) / (e1 - e0);   /* literal edges: a constant divisor */
    const float t = fmin2(fmax2(q, 0.0f), 1.0f);
    return t * t * (3.0f - 2.0f * t);
}

/* Division / square root of the media code: LEAN = the bare cores above on operands that are tame by
 * construction (the render kernels), otherwise hipcc's IEEE forms (unit kernels on arbitrary points). */
template <bool LEAN> struct Ar {
    static RRT_DEV float div(float a, float b) { return LEAN ? rrt_div_tame(a, b) : a / b; }
    static RRT_DEV float sqrt(float x) { return LEAN ? sqrt_tame(x) : sqrtf(x); }
};

/*
 * getGeodesicAcc, geodesics.h:30-45, with SPIN_AXIS = (0,1,0), EVENT_HORIZON = 2:
 *   radial = (-1.5f*2.0f * L2 / (r2*r2*r)) * p        (-1.5f*2.0f folds to -3.0f)
 *   drag   = ((2.0f*a*2.0f) / (r2*r)) * (p.z, 0, -p.x)
 * drag_c = (2.0f*a)*2.0f is computed once on the host (exact scaling).
 * r2, r and y ~ 1/r come from the caller (the march loop already has them for the
 * stage-1 point); both reciprocal seeds are powers of y.
 */
template <bool SPIN>
RRT_DEV v3 geodesic_acc_r(v3 p, v3 v, float drag_c, float r2, float r, float y) {
    v3 L = cross(p, v);
    float L2 = dot(L, L);
    float y2 = y * y;
    float y3 = y2 * y;
    float d2 = r2 * r;
    float d1 = (r2 * r2) * r;
    float radial_mag = div_seeded(-3.0f * L2, d1, y3 * y2);
    v3 acc = mul(p, radial_mag);
    if (SPIN) {
        float ds = div_seeded(drag_c, d2, y3);
        acc.x = acc.x + p.z * ds;
        acc.z = acc.z + (-p.x) * ds;
    }
    if (__builtin_expect(__any(r2 < 1.0f), 0)) {       /* geodesics.h:33: sqrt(r2) < 1  <=>  r2 < 1 */
        if (r2 < 1.0f) acc = mk(0.f, 0.f, 0.f);
    }
    return acc;
}

template <bool SPIN>
RRT_DEV v3 geodesic_acc(v3 p, v3 v, float drag_c) {
    float r2 = dot(p, p);
    float r, y;
    sqrt_rsq(r2, r, y);
    if (__builtin_expect(__any(!(r2 >= 1.0f)), 0)) {   /* r2 == 0 / tiny: keep the seeds finite */
        if (!(r2 >= 1.0f)) { r = sqrtf(r2); y = 1.0f; }
    }
    return geodesic_acc_r<SPIN>(p, v, drag_c, r2, r, y);
}

/*
 * integrate_rk4, integrators.h:23-59 (MASS_POS = 0: the sub() calls are identities).
 * `hh` = h*0.5f and `h6` = h/6.0f are passed in (h takes three values in the march).
 * 2*a + b is evaluated as fma(2, a, b): identical bits, because 2*a is exact.
 */
template <bool SPIN>
RRT_DEV void integrate_rk4_r(v3& p, v3& v, float h, float hh, float h6, float drag_c,
                             float r2, float r, float y) {
    v3 p0 = p, v0 = v;
    v3 kv1 = geodesic_acc_r<SPIN>(p0, v0, drag_c, r2, r, y);
    v3 v2 = add(v0, mul(kv1, hh));
    v3 p2 = add(p0, mul(v0, hh));
    v3 kv2 = geodesic_acc<SPIN>(p2, v2, drag_c);
    v3 v3_ = add(v0, mul(kv2, hh));
    v3 p3 = add(p0, mul(v2, hh));
    v3 kv3 = geodesic_acc<SPIN>(p3, v3_, drag_c);
    v3 v4 = add(v0, mul(kv3, h));
    v3 p4 = add(p0, mul(v3_, h));
    v3 kv4 = geodesic_acc<SPIN>(p4, v4, drag_c);
    v3 kv_sum, kp_sum;
    kv_sum.x = kv1.x + __builtin_fmaf(2.0f, kv2.x, __builtin_fmaf(2.0f, kv3.x, kv4.x));
    kv_sum.y = kv1.y + __builtin_fmaf(2.0f, kv2.y, __builtin_fmaf(2.0f, kv3.y, kv4.y));
    kv_sum.z = kv1.z + __builtin_fmaf(2.0f, kv2.z, __builtin_fmaf(2.0f, kv3.z, kv4.z));
    kp_sum.x = v0.x + __builtin_fmaf(2.0f, v2.x, __builtin_fmaf(2.0f, v3_.x, v4.x));
    kp_sum.y = v0.y + __builtin_fmaf(2.0f, v2.y, __builtin_fmaf(2.0f, v3_.y, v4.y));
    kp_sum.z = v0.z + __builtin_fmaf(2.0f, v2.z, __builtin_fmaf(2.0f, v3_.z, v4.z));
    v = add(v0, mul(kv_sum, h6));
    p = add(p0, mul(kp_sum, h6));
}

template <bool SPIN>
RRT_DEV void integrate_rk4(v3& p, v3& v, float h, float drag_c) {
    float r2 = dot(p, p);
    float r, y;
    sqrt_rsq(r2, r, y);
    if (__builtin_expect(__any(!(r2 >= 1.0f)), 0)) {
        if (!(r2 >= 1.0f)) { r = sqrtf(r2); y = 1.0f; }
    }
    integrate_rk4_r<SPIN>(p, v, h, h * 0.5f, h / 6.0f, drag_c, r2, r, y);
}

/*
 * Correctly rounded sqrt WITHOUT the v_rsq_f32: Goldschmidt iterations from a caller-supplied estimate y0 of
 * 1/sqrt(x).  A transcendental instruction costs ~13 cycles in a VALU stream on gfx950 (6 ordinary issue slots,
 * profiles/r02_valu_issue_microbench.txt), and the march always has an excellent estimate at hand: the radius of
 * RK4 stage k differs from stage k-1's by |v| h/2 at most (<= 1 %), stage 3's from stage 2's and the next step's
 * from stage 4's by O(h^2) only.  ITERS coupled iterations (3 FMAs each, quadratic: error e -> 1.5 e^2) bring such
 * an estimate to rounding level, then the same residual correction as sqrt_rsq.  The residual r of the LAST
 * iteration measures the error that iteration started from; the result is used only if |r| <= kSeedTol, i.e. if
 * that error was small enough for the iteration to converge to rounding level -- otherwise (first step of a ray,
 * a huge jump) the caller falls back to sqrt_rsq.  This is the plain form of the idea; the march runs sqrt_seeded_yh
 * below (the same iteration, acceptance on the first residual), which is the one checked against sqrtf over two full
 * binades x seed errors up to the tolerance on the GPU (rrt_selfcheck_sqrt_seeded).
 */
constexpr float kSeedTol = 1.5e-4f;         /* 1.5 * tol^2 = 3.4e-8 < 2^-24.8 */
template <int ITERS>
RRT_DEV bool sqrt_seeded(float x, float y0, float& root, float& inv_root) {
    float g = x * y0;
    float h = 0.5f * y0;
    float r = 0.0f;
#pragma unroll
    for (int i = 0; i < ITERS; ++i) {
        r = __builtin_fmaf(-h, g, 0.5f);
        g = __builtin_fmaf(g, r, g);
        h = __builtin_fmaf(h, r, h);
    }
    float d = __builtin_fmaf(-g, g, x);
    root = __builtin_fmaf(d, h, g);
    inv_root = h + h;
    return fabsf(r) <= kSeedTol;
}

/*
 * The march's step (`integrate_rk4_lean`): integrate_rk4_r with every stage radius a seeded square root, in as few
 * instructions as that takes.  The loop is VALU-issue bound at ~95 % of all issue slots, so only the instruction COUNT moves
 * it; what a straightforward seeded step (sqrt_seeded per stage, round 2) carries beyond the arithmetic, and this one does not:
 *   - `h = 0.5f * y0` at the head of every seeded square root: each root already produces h = y/2 (the Goldschmidt
 *     half-reciprocal) next to y = h + h, so the pair (y, h) is handed on instead of y alone (-1 per root);
 *   - the acceptance test moves from the LAST to the FIRST residual, r1 = 1/2 - h0*g0 = (1 - x*y0^2)/2, which measures
 *     the seed's error e directly (r1 = -e - e^2/2): one iteration leaves 1.5 e^2, so the two-iteration roots accept
 *     |r1| <= kSeedTol2 = 9e-3 (then the second iteration starts within 1.3e-4 < kSeedTol, the case the one-iteration
 *     form is checked for) and the one-iteration roots |r1| <= kSeedTol as before.  Testing the first residual also
 *     closes a hole of the last-residual test: a seed with x*y0^2 ~ 4 converges to MINUS the root with a tiny last
 *     residual (it needs a radius that doubles within half a step, which no ray does, but it was accepted);
 *   - the `r < 1` guard of geodesics.h:33 on every acceleration: an ACCEPTED stage radius lies within 1 % of the
 *     radius its seed came from, and the chain of seeds starts at the loop-top radius, which has passed the horizon
 *     test r >= 2.02 (or, for the loop-top root itself, at the previous step's last stage): every accepted radius
 *     is > 1.9, so the guard can only fire on lanes that took the v_rsq fall-back, and is evaluated there (-4 compares);
 *   - VAC (a compile-time flag for the wave-uniform vacuum step, rrt_kernels.h: vacuum_run): h, h/2 and h/6 are literals.
 * Bits are unchanged: every root is still the correctly rounded one (or the fall-back's), y and h only seed the
 * Markstein divides, which deliver the correctly rounded quotient from any seed of that quality.
 */
constexpr float kSeedTol2 = 9e-3f;          /* first residual of a two-iteration root: 1.5 * (9.05e-3)^2 = 1.23e-4 < kSeedTol */

/* returns REJECTED (the seed was not good enough; NaN included): callers branch on that one predicate only, so a
 * single v_cmp serves the wave ballot and the lane mask */
template <int ITERS>
RRT_DEV bool sqrt_seeded_yh(float x, float y0, float h0, float& root, float& y, float& h_out) {
    float g = x * y0;
    float h = h0;
    float r = __builtin_fmaf(-h, g, 0.5f);
    const float first = r;
    g = __builtin_fmaf(g, r, g);
    h = __builtin_fmaf(h, r, h);
    if (ITERS == 2) {
        r = __builtin_fmaf(-h, g, 0.5f);
        g = __builtin_fmaf(g, r, g);
        h = __builtin_fmaf(h, r, h);
    }
    float d = __builtin_fmaf(-g, g, x);
    root = __builtin_fmaf(d, h, g);
    y = h + h;
    h_out = h;
    bool rejected = !(fabsf(first) <= (ITERS == 2 ? kSeedTol2 : kSeedTol));
    if (ITERS == 2) {
        /* Round 4: the one operand class on which an ACCEPTED two-iteration root was not the correctly rounded one --
         * x = 4^k (1 + 2^-23), the float right above a power of four, whose root 2^k (1 + 2^-24 - 2^-49) lies 2^-26 ulp under a
         * rounding tie: the half-reciprocal of the second iteration sits at a binade boundary there and can come out two
         * of the finer ulps high, which tips g + d h over the tie (rrt_selfcheck_div_march: 176 of 1.1e12 roots with seed
         * errors spread over the acceptance interval, every one of this form; none among the one-iteration roots, none
         * after this guard: profiles/r04_div_march_seeds_probe.txt).  Two instructions on the two roots of a GENERIC step
         * (the vacuum step has one-iteration roots only): such an x takes the v_rsq fall-back, which is checked for every
         * float. */
        rejected = rejected || (rrt_f2u(x) & 0x00ffffffu) == 0x00800001u;
    }
    return rejected;
}

/* the v_rsq fall-back of a rejected root, with the `r < 1` case of geodesic_acc(); `small` = geodesics.h:33 fires */
RRT_DEV void radius_fallback(float r2, float& r, float& y, float& h, bool& small) {
    sqrt_rsq(r2, r, y);
    h = 0.5f * y;
    small = false;
    if (!(r2 >= 1.0f)) {
        /* r2 in [0, 1): the acceleration is zeroed whatever the seeds are, and y = 0 makes the NEXT root reject its
         * seed (first residual 1/2), so that a following radius < 1 is seen by its own fall-back; NaN: y = 1 keeps
         * the arithmetic going (everything is NaN from here on, as in the reference) */
        small = r2 < 1.0f;
        r = sqrtf(r2); y = small ? 0.0f : 1.0f; h = 0.5f * y;
    }
}

/* returns the wave mask of lanes whose radius is < 1 (geodesics.h:33); 0 unless a lane took the fall-back */
template <int ITERS>
RRT_DEV unsigned long long stage_radius_yh(float r2, float y0, float h0, float& r, float& y, float& h) {
    const bool rejected = sqrt_seeded_yh<ITERS>(r2, y0, h0, r, y, h);
    unsigned long long small_mask = 0ull;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(rejected) != 0ull, 0)) {
        bool small = false;
        if (rejected) radius_fallback(r2, r, y, h, small);
        small_mask = __builtin_amdgcn_ballot_w64(small);
    }
    return small_mask;
}

/* fused forms of the 3-vector helpers (RRT_ARITH_FMAD / RRT_ARITH_FAST): one rounding per multiply-add */
RRT_DEV float dot_fma(v3 a, v3 b) { return __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)); }
RRT_DEV v3 axpy(v3 x, float a, v3 y) {       /* a*x + y, fused */
    return mk(__builtin_fmaf(x.x, a, y.x), __builtin_fmaf(x.y, a, y.y), __builtin_fmaf(x.z, a, y.z));
}
RRT_DEV v3 cross_fma(v3 a, v3 b) {
    return mk(__builtin_fmaf(a.y, b.z, -(a.z * b.y)), __builtin_fmaf(a.z, b.x, -(a.x * b.z)), __builtin_fmaf(a.x, b.y, -(a.y * b.x)));
}

/* geodesic_acc_r without the guard; lanes in `small_mask` (only ever set behind radius_fallback) get the zero of
 * geodesics.h:33.  The mask is a scalar: the straight path pays one s_cmp, no vector instruction.
 * FMA (RRT_ARITH_FMAD): the same expression tree with every multiply-add fused -- cross and dot products, the drag term --
 * and the two divisions still correctly rounded (div_seeded): what a contracting compiler with IEEE division makes of
 * geodesics.h:30-45 (nvcc's defaults for the reference: -fmad=true, -prec-div=true, -prec-sqrt=true). */
template <bool SPIN, bool FMA = false>
RRT_DEV v3 geodesic_acc_ng(v3 p, v3 v, float drag_c, float r2, float r, float y, unsigned long long small_mask) {
    v3 L = FMA ? cross_fma(p, v) : cross(p, v);
    float L2 = FMA ? dot_fma(L, L) : dot(L, L);
    float y2 = y * y;
    float y3 = y2 * y;
    float d2 = r2 * r;
    float d1 = (r2 * r2) * r;
    float radial_mag = div_seeded(-3.0f * L2, d1, y3 * y2);
    v3 acc = mul(p, radial_mag);
    if (SPIN) {
        float ds = div_seeded(drag_c, d2, y3);
        if (FMA) {
            acc.x = __builtin_fmaf(p.z, ds, acc.x);
            acc.z = __builtin_fmaf(-p.x, ds, acc.z);
        } else {
            acc.x = acc.x + p.z * ds;
            acc.z = acc.z + (-p.x) * ds;
        }
    }
    if (__builtin_expect(small_mask != 0ull, 0)) {
        if ((small_mask >> (threadIdx.x & 63)) & 1ull) acc = mk(0.f, 0.f, 0.f);
    }
    return acc;
}

/* One RK4 step (integrators.h:23-59) from the loop-top radius (r2, r, y, h) of the pre-step position; (y_next,
 * h_next) = the reciprocal radius of the last stage position, the seed of the next step's loop-top root.
 * The loop-top radius has passed the caller's horizon test (r >= 2.02), so stage 1 needs no `r < 1` case.  VAC: h = STEP_SIZE_M exactly (no zone applies), constants folded. */
#ifndef RRT_EXTRAP_SEEDS
#define RRT_EXTRAP_SEEDS 1
#endif
/* VAC only (RRT_EXTRAP_SEEDS): the two-iteration roots of stages 2 and 4 become one-iteration roots with a seed
 * extrapolated LINEARLY from the two reciprocal radii half a step apart that the march already holds -- stage 4 from
 * (loop top, stage 3), stage 2 from (the previous vacuum step's stage 3 ~ its stage 2 position, this loop top): the
 * error is y'' (h/2)^2 <= 2 (h / 2r)^2 = 5e-5 relative at r = 30, inside the one-iteration tolerance kSeedTol, and the
 * acceptance test catches everything else (first vacuum step after a step of another size: hc_prev belongs to
 * another spacing, the seed is rejected, the v_rsq fall-back runs once).  -2 instructions per vacuum step.
 * Sign: the acceptance test is even in the seed (a seed of MINUS the reciprocal root converges to minus the root with a
 * zero residual), so seeds must be positive by provenance -- they are: every h is either the v_rsq fall-back's or
 * h0 (1 + r) of an accepted root with |r| <= 9e-3, i.e. positive by induction, and an extrapolated 2 h_a - h_b of two
 * such values could only be negative if the radius had tripled within half a vacuum step (0.15 |v| at r >= 30).
 * FMA (RRT_ARITH_FMAD, round 5): stage states, squared radii and the final combination as fused multiply-adds (one rounding
 * where the source has two); roots and divisions exactly as in the strict step -- correctly rounded.  ~223 instead of ~283
 * VALU instructions per vacuum step.  Not bit-comparable with the strict step (every fused product skips a rounding), which
 * is the arithmetic the reference's own binary has under nvcc's default -fmad=true. */
template <bool SPIN, bool VAC, bool FMA = false>
RRT_DEV void integrate_rk4_lean(v3& p, v3& v, float h_in, float hh_in, float h6_in, float drag_c,
                                float r2, float r, float y, float hy, float& y_next, float& h_next, float& hc_prev) {
    const float h = VAC ? kStepSize : h_in;
    const float hh = VAC ? 0.5f * kStepSize : hh_in;
    const float h6 = VAC ? kStepSize / 6.0f : h6_in;
    constexpr bool EXTRAP = VAC && RRT_EXTRAP_SEEDS;
    v3 p0 = p, v0 = v;
    v3 kv1 = geodesic_acc_ng<SPIN, FMA>(p0, v0, drag_c, r2, r, y, 0ull);
    v3 v2 = FMA ? axpy(kv1, hh, v0) : add(v0, mul(kv1, hh));
    v3 p2 = FMA ? axpy(v0, hh, p0) : add(p0, mul(v0, hh));
    float r2b = FMA ? dot_fma(p2, p2) : dot(p2, p2), rb, yb, hb;
    unsigned long long sb;
    if (EXTRAP) {
        const float h0 = __builtin_fmaf(2.0f, hy, -hc_prev);
        sb = stage_radius_yh<1>(r2b, h0 + h0, h0, rb, yb, hb);
    } else {
        sb = stage_radius_yh<2>(r2b, y, hy, rb, yb, hb);
    }
    v3 kv2 = geodesic_acc_ng<SPIN, FMA>(p2, v2, drag_c, r2b, rb, yb, sb);
    v3 v3_ = FMA ? axpy(kv2, hh, v0) : add(v0, mul(kv2, hh));
    v3 p3 = FMA ? axpy(v2, hh, p0) : add(p0, mul(v2, hh));
    float r2c = FMA ? dot_fma(p3, p3) : dot(p3, p3), rc, yc, hc;
    const unsigned long long sc = stage_radius_yh<1>(r2c, yb, hb, rc, yc, hc);
    v3 kv3 = geodesic_acc_ng<SPIN, FMA>(p3, v3_, drag_c, r2c, rc, yc, sc);
    v3 v4 = FMA ? axpy(kv3, h, v0) : add(v0, mul(kv3, h));
    v3 p4 = FMA ? axpy(v3_, h, p0) : add(p0, mul(v3_, h));
    float r2d = FMA ? dot_fma(p4, p4) : dot(p4, p4), rd, yd, hd;
    unsigned long long sd;
    if (EXTRAP) {
        const float h0 = __builtin_fmaf(2.0f, hc, -hy);
        sd = stage_radius_yh<1>(r2d, h0 + h0, h0, rd, yd, hd);
    } else {
        sd = stage_radius_yh<2>(r2d, yc, hc, rd, yd, hd);
    }
    hc_prev = VAC ? hc : 0.0f;            /* a generic step has another spacing: no extrapolation across it */
    v3 kv4 = geodesic_acc_ng<SPIN, FMA>(p4, v4, drag_c, r2d, rd, yd, sd);
    v3 kv_sum, kp_sum;
    kv_sum.x = kv1.x + __builtin_fmaf(2.0f, kv2.x, __builtin_fmaf(2.0f, kv3.x, kv4.x));
    kv_sum.y = kv1.y + __builtin_fmaf(2.0f, kv2.y, __builtin_fmaf(2.0f, kv3.y, kv4.y));
    kv_sum.z = kv1.z + __builtin_fmaf(2.0f, kv2.z, __builtin_fmaf(2.0f, kv3.z, kv4.z));
    kp_sum.x = v0.x + __builtin_fmaf(2.0f, v2.x, __builtin_fmaf(2.0f, v3_.x, v4.x));
    kp_sum.y = v0.y + __builtin_fmaf(2.0f, v2.y, __builtin_fmaf(2.0f, v3_.y, v4.y));
    kp_sum.z = v0.z + __builtin_fmaf(2.0f, v2.z, __builtin_fmaf(2.0f, v3_.z, v4.z));
    v = FMA ? axpy(kv_sum, h6, v0) : add(v0, mul(kv_sum, h6));
    p = FMA ? axpy(kp_sum, h6, p0) : add(p0, mul(kp_sum, h6));
    y_next = yd;
    h_next = hd;
}

/*
 * FAST arithmetic mode (rrt_params.arith_mode = RRT_ARITH_FAST; NOT the parity path).
 * Same equations (geodesics.h:30-45, integrators.h:23-59) evaluated the way a GPU compiler with
 * contraction would: fused multiply-adds, 1/r from v_rsq_f32 (1 ulp) instead of correctly rounded
 * sqrt and divides.  Every step is perturbed at the 1e-7 relative level, so frames differ from the
 * strict path / the oracle by rounding noise that near-critical rays amplify; the measured
 * deviation is reported by tests/test_gpu_frames.py::test_fast_mode_* and DESIGN.md.
 */
template <bool SPIN>
RRT_DEV v3 geodesic_acc_fast(v3 p, v3 v, float drag_c, float r2, float y) {
    v3 L = mk(__builtin_fmaf(p.y, v.z, -(p.z * v.y)), __builtin_fmaf(p.z, v.x, -(p.x * v.z)),
              __builtin_fmaf(p.x, v.y, -(p.y * v.x)));
    float L2 = __builtin_fmaf(L.z, L.z, __builtin_fmaf(L.y, L.y, L.x * L.x));
    float y2 = y * y;
    float y3 = y2 * y;
    float mag = (-3.0f * L2) * (y3 * y2);
    v3 acc = mul(p, mag);
    if (SPIN) {
        float ds = drag_c * y3;
        acc.x = __builtin_fmaf(p.z, ds, acc.x);
        acc.z = __builtin_fmaf(-p.x, ds, acc.z);
    }
    if (__builtin_expect(__any(r2 < 1.0f), 0)) {
        if (r2 < 1.0f) acc = mk(0.f, 0.f, 0.f);
    }
    return acc;
}

template <bool SPIN>
RRT_DEV void integrate_rk4_fast(v3& p, v3& v, float h, float hh, float h6, float drag_c, float r2, float y) {
    v3 p0 = p, v0 = v;
    v3 kv1 = geodesic_acc_fast<SPIN>(p0, v0, drag_c, r2, y);
    v3 v2 = axpy(kv1, hh, v0);
    v3 p2 = axpy(v0, hh, p0);
    float r2b = dot_fma(p2, p2);
    v3 kv2 = geodesic_acc_fast<SPIN>(p2, v2, drag_c, r2b, __builtin_amdgcn_rsqf(r2b));
    v3 v3_ = axpy(kv2, hh, v0);
    v3 p3 = axpy(v2, hh, p0);
    float r2c = dot_fma(p3, p3);
    v3 kv3 = geodesic_acc_fast<SPIN>(p3, v3_, drag_c, r2c, __builtin_amdgcn_rsqf(r2c));
    v3 v4 = axpy(kv3, h, v0);
    v3 p4 = axpy(v3_, h, p0);
    float r2d = dot_fma(p4, p4);
    v3 kv4 = geodesic_acc_fast<SPIN>(p4, v4, drag_c, r2d, __builtin_amdgcn_rsqf(r2d));
    v3 kv_sum = add(kv1, axpy(kv2, 2.0f, axpy(kv3, 2.0f, kv4)));
    v3 kp_sum = add(v0, axpy(v2, 2.0f, axpy(v3_, 2.0f, v4)));
    v = axpy(kv_sum, h6, v0);
    p = axpy(kp_sum, h6, p0);
}

/* calculateRedshiftFactor, geodesics.h:11-25; `r` = length(p) is passed in by callers that already hold it.
 * LEAN (render kernels; called only for samples with a density > 0.001, i.e. cylindrical radius in [10, 25] and
 * r in [10, 30)): the tame operands are r (2/r, sqrt(1 - 2/r) with argument in [0.8, 0.94]), r^1.5 + a in
 * [30, 170] for |a| <= 1, the cylindrical radius `mag` in [10, 25] of the gas direction, and 1 - v^2 in
 * [0.998, 1].  The Doppler denominator gamma*(1 - v cos) is NOT bounded away from zero (the ray "velocity" is not
 * normalised) and keeps the IEEE division, as does everything when |a| > 1. */
template <bool LEAN>
RRT_DEV float redshift_factor_r(v3 p, float r, v3 ray_vel, float spin) {
    if (r < kEventHorizon * 1.01f) return 0.0f;
    const float gx = -p.z, gz = p.x;
    const float m2 = gx * gx + 0.0f * 0.0f + gz * gz;                              /* length(make_float3(-z, 0, x))^2 */
    if (LEAN && __builtin_expect(fabsf(spin) <= 1.0f && r >= 9.0f && r < 64.0f && m2 >= 1.0f && m2 < 4096.0f, 1)) {
        const float g_gravity = sqrt_tame(1.0f - rrt_div_tame(kEventHorizon, r));
        const float v_mag = rrt_div_tame(1.0f, r * sqrt_tame(r) + spin);          /* rrt_powf(r, 1.5f) == r * sqrt(r) */
        const float mag = sqrt_tame(m2);                                           /* >= 1: normalize() divides (math_utils.h:23-27) */
        const v3 gas_dir = mk(rrt_div_tame(gx, mag), 0.0f, rrt_div_tame(gz, mag)); /* 0 / mag == +0 */
        const float cos_theta = dot(ray_vel, gas_dir);
        const float gamma = rrt_div_tame(1.0f, sqrt_tame(1.0f - v_mag * v_mag));
        const float g_doppler = 1.0f / (gamma * (1.0f - v_mag * cos_theta));
        return g_gravity * g_doppler;
    }
    float g_gravity = sqrtf(1.0f - kEventHorizon / r);
    float v_mag = 1.0f / (rrt_powf(r, 1.5f) + spin);
    v3 gas_dir = normalize(mk(-p.z, 0.f, p.x));
    float cos_theta = dot(ray_vel, gas_dir);
    float gamma = 1.0f / sqrtf(1.0f - v_mag * v_mag);
    float g_doppler = 1.0f / (gamma * (1.0f - v_mag * cos_theta));
    return g_gravity * g_doppler;
}
RRT_DEV float redshift_factor(v3 p, v3 ray_vel, float spin) { return redshift_factor_r<false>(p, length(p), ray_vel, spin); }

/* getDiskTemperature, densities.h:12-15 (LEAN: r in [10, 64) -- the callers' density gate) */
template <bool LEAN>
RRT_DEV float disk_temperature_t(float r) {
    if (r < kIsco) return 0.0f;
    const float x = (LEAN && r < 64.0f) ? rrt_div_const(r, kIsco) : r / kIsco;
    return kDiskTempRef * rrt_powf(x, -0.75f);
}
RRT_DEV float disk_temperature(float r) { return disk_temperature_t<false>(r); }

/* RRT_PROBE (dev builds only, wrong pixels): bit 0 drops the accretion density, bit 1 the dust density, bit 2 the
 * emission block, bit 3 replaces every noise3D by a cheap expression, bit 4 makes every table lookup of a wave read one
 * cell (lut_fetch) -- timing probes that apportion the media cost (tools/ab_views.py; profiles/README.md round 3). */
/* unroll factors of the media loops (1 = rolled, the shipped form; A/B builds override them) */
#define RRT_PRAGMA_STR(x) _Pragma(#x)
#define RRT_PRAGMA_UNROLL(n) RRT_PRAGMA_STR(unroll n)
#ifndef RRT_WARP_UNROLL
#define RRT_WARP_UNROLL 1
#endif
#ifndef RRT_ACC_UNROLL
#define RRT_ACC_UNROLL 1
#endif
#ifndef RRT_RIDGE_UNROLL
#define RRT_RIDGE_UNROLL 1
#endif
/* one noise3D evaluation, from the table when the wave-uniform switch says so */
template <bool LUT>
RRT_DEV float noise3d_sel(v3 p, const NoiseLut& L, bool from_table, unsigned* oob) {
    if (RRT_PROBE & 8) return 0.45f + 0.01f * p.x;
    if (LUT && from_table) return noise3d_lut(L, p, oob);
    return noise3d(p);
}

/* Two successive table lookups whose positions are both known: their four loads are issued together, so one
 * memory latency is exposed instead of two (RRT_LUT_PAIRS=0: one after the other). */
#ifndef RRT_LUT_PAIRS
#define RRT_LUT_PAIRS 1
#endif

RRT_DEV void noise3d_lut_pair2(const NoiseLut& L0, const NoiseLut& L1, v3 p0, v3 p1, unsigned* oob, float& n0, float& n1) {
    if (RRT_PROBE & 8) { n0 = 0.45f + 0.01f * p0.x; n1 = 0.45f + 0.01f * p1.x; return; }
    const LutTap a = lut_fetch(L0, p0, oob);
    const LutTap b = lut_fetch(L1, p1, oob);
    n0 = lut_blend(a);
    n1 = lut_blend(b);
}
RRT_DEV void noise3d_lut_pair(const NoiseLut& L, v3 p0, v3 p1, unsigned* oob, float& n0, float& n1) {
    noise3d_lut_pair2(L, L, p0, p1, oob, n0, n1);
}

/* fbm(p, 2) (math_utils.h:112-121) with a table switch per octave */
template <bool LUT>
RRT_DEV float fbm2_sel(v3 p, const NoiseLut& L, bool t0, bool t1, unsigned* oob) {      /* (octave 1 from L's own box when t1) */
    float v = 0.0f, a = 0.5f;
    if (LUT && RRT_LUT_PAIRS && t0 && t1) {
        float n0, n1;
        noise3d_lut_pair(L, p, mk(p.x * 2.05f + 10.0f, p.y * 2.05f + 10.0f, p.z * 2.05f + 10.0f), oob, n0, n1);
        v += a * n0;
        a *= 0.5f;
        v += a * n1;
        return v;
    }
#pragma unroll 1
    for (int i = 0; i < 2; ++i) {
        v += a * noise3d_sel<LUT>(p, L, i == 0 ? t0 : t1, oob);
        p = mk(p.x * 2.05f + 10.0f, p.y * 2.05f + 10.0f, p.z * 2.05f + 10.0f);
        a *= 0.5f;
    }
    return v;
}

/* Highest octave of each noise call family that the tables cover (rrt_hip.hip sizes the boxes from these). */
#ifndef RRT_LUT_ACC_OCT
#define RRT_LUT_ACC_OCT 4
#endif
constexpr int kLutAccOctaves = RRT_LUT_ACC_OCT;      /* accretion fbm(.,5): octaves 0..3 */
#ifndef RRT_LUT_RIDGE_OCT
#define RRT_LUT_RIDGE_OCT 3
#endif
#ifndef RRT_LUT_DETAIL
#define RRT_LUT_DETAIL 1
#endif
constexpr int kLutRidgeOctaves = RRT_LUT_RIDGE_OCT;    /* dust ridge sum: octaves 0..2 */
constexpr bool kLutDetail = RRT_LUT_DETAIL != 0;        /* first octave of the dust detail fbm */

/*
 * getAccretionDensity, densities.h:20-62.  EARLY_OUT=false, LUT=false is the literal function (unit
 * tests); the render kernels use EARLY_OUT=true (see below) and, with a noise table, LUT=true.
 */
/* What both density functions derive from the sample position alone -- cylindrical radius and radial gate
 * (densities.h:21-22, :70-71), q = ISCO/rc and its square root (:32, :41, :79, :89), the azimuth (:38, :88) --
 * evaluated once per sample when a render kernel needs both functions (the cloud zone lies inside the disk zone). */
struct DiskPoint { float rc, q, sq, azimuth; bool has_azimuth; };

template <bool LEAN>
RRT_DEV bool disk_point(v3 p, DiskPoint& d) {           /* false: outside the radial gate, both densities are 0 */
    const float rc2 = p.x * p.x + 0.0f * 0.0f + p.z * p.z;
    if (LEAN && !(rc2 >= 1.0f)) return false;          /* rc < 1 < ISCO; keeps sqrt_tame in range */
    d.rc = Ar<LEAN>::sqrt(rc2);
    if (d.rc < kIsco || d.rc > kDiskOut) return false;
    /* Exact early-out (round 3, render kernels): far from the mid-plane both densities are 0 before anything else is
     * computed.  The accretion slab exponent is -y^2 rc / (12.8 + 1e-7 rc) up to 1e-6 relative (thick^2 = 0.64 * 10/rc),
     * so y^2 rc > 135 puts it below -10.54 < -10.5, where accretion_density_at returns 0 (its pre-test); the dust slab
     * there is e^(-y^2 / 0.125) <= e^-43, far under the `base < 0.001f` return of densities.h:85.  A quarter of the
     * accretion calls of the outer disk end here, 12 instructions in, instead of behind two divides and two roots. */
    if (LEAN && (p.y * p.y) * d.rc > 135.0f) return false;
    d.q = Ar<LEAN>::div(kIsco, d.rc);                   /* in [0.4, 1] */
    d.sq = Ar<LEAN>::sqrt(d.q);                         /* == powf(q, 0.5f); q * sq == powf(q, 1.5f) (rrt_math.h) */
    d.azimuth = 0.0f; d.has_azimuth = false;
    return true;
}
RRT_DEV float disk_azimuth(v3 p, DiskPoint& d) {
    if (!d.has_azimuth) { d.azimuth = rrt_atan2f(p.z, p.x); d.has_azimuth = true; }
    return d.azimuth;
}

/* Both density functions have a seam where `time` first enters (densities.h:39, :90).  Above it is the HEAD: what the sample
 * position alone decides -- the envelope, or a return of 0 before `time` is reached.  Below it is the TAIL, which reads the
 * envelope, rc, q, sq, the height and the azimuth.  PART says how much of the one text an instance runs:
 *   kWhole   head then tail: the function (the in-line kernels, the workspace path, the unit hooks)
 *   kHead    returns the envelope at the seam (an early-out's 0 above it): the march cache's fill, once per retained sample
 *   kTail    starts at the seam with `envelope` as given: every replayed frame (sample_record / eval_sample_record below);
 *            of `p` only p.y is read, and the azimuth is the one dp holds
 * so that the record path cannot drift from the literal one: there is no second text. */
enum DensityPart { kWhole = 0, kHead = 1, kTail = 2 };

template <bool EARLY_OUT, bool LUT, bool BANDED = false, int PART = kWhole>
RRT_DEV float accretion_density_at(v3 p, float time, DiskPoint& dp, const NoiseLut& L, unsigned* oob, const DustBands* bands = nullptr,
                                   float envelope_in = 0.0f) {
    /* The render kernels (EARLY_OUT) call this only inside the disk zone, |y| < 4 and r < 30 (raymarcher.cu:57), so
     * every division / square root below has tame operands once the radial gate has passed: rc in [10, 25],
     * q = 10/rc in [0.4, 1], thick in [0.5, 0.8], y*y < 16 (a y*y too small for the bare division to be exact,
     * < 2^-100, feeds exp(-0) = 1 either way). */
    constexpr bool LEAN = EARLY_OUT;
    const float rc = dp.rc, q = dp.q;
    float envelope;
    if constexpr (PART == kTail) envelope = envelope_in;
    else {
    const float thick = kDiskH * dp.sq;                /* DISK_H_M * powf(q, 0.5f) */
    const float slab_arg = Ar<LEAN>::div(-(p.y * p.y), 2.0f * thick * thick + 1e-7f);
    /* Exact pre-test of the early-out below (round 3), before expf / powf / the rim are paid for: slab <= e^-10.5
     * (1 + 3e-7) < 2.7537e-5, fall = q^0.4 <= 1 + 3e-7 (q <= 1) and rim <= 1, so envelope * 30.02f < 8.3e-4 <= 0.001f and
     * the test below returns 0 as well.  Beyond 4.58 scale heights -- a quarter of the disk zone's |y| < 4 at the outer
     * radii -- nothing else of this function is evaluated.  (NaN compares false and takes the long way.) */
    if (EARLY_OUT && slab_arg < -10.5f) return 0.0f;
    float rim = 1.0f;                                   /* taper of the outer 15 % (:25-30) */
    const float rim_from = kDiskOut * 0.85f;
    if (rc > rim_from) {
        rim = 1.0f - (LEAN ? rrt_div_const(rc - rim_from, kDiskOut - rim_from) : (rc - rim_from) / (kDiskOut - rim_from));
        rim *= rim;
    }
    const float slab = rrt_expf(slab_arg);
    const float fall = rrt_powf(q, 0.4f);
    envelope = slab * fall * rim;

    /*
     * Exact early-out (not in the reference): the streak factor is <= 6 (densities.h:59), so the
     * result is <= envelope * (0.02f + 5.0f*6.0f); rounding is monotone, so if that bound is
     * <= 0.001f the caller's `d_disk > 0.001f` test (raymarcher.cu:71,76) fails and the value is
     * never used.
     */
    if (EARLY_OUT && envelope * (0.02f + 5.0f * 6.0f) <= 0.001f) return 0.0f;
    }
    /* ---- the seam: with EARLY_OUT the envelope is > 3.3e-5 or a NaN here, never 0 ---- */
    if constexpr (PART == kHead) return envelope;

    const float azimuth = disk_azimuth(p, dp);
    const float kepler = 3.5f * (q * dp.sq);            /* 3.5f * powf(q, 1.5f) */
    const float turned = azimuth - time * kepler;
    float sn, cs;
    rrt_sincosf(turned, &sn, &cs);
    const v3 swirl = mk(rc * cs, p.y * 4.0f, rc * sn);
    const float drift = time * 0.35f;
    v3 at = mk(swirl.x * 0.45f + 0.0f, swirl.y * 0.45f + drift, swirl.z * 0.45f + 0.0f);

    unsigned from_table = 0u;                           /* bit o: octave o is read from the table */
    if (LUT) {
        const float sp = lut_spread(at);
        float cells = 1.0f;
#pragma unroll
        for (int o = 0; o < kLutAccOctaves; ++o) {
            if (lut_fits(sp, cells)) from_table |= 1u << o;
            cells *= 2.05f;
        }
        from_table &= L.families;
    }
    float n = 0.0f, amp = 0.5f;                         /* fbm(at, 5), math_utils.h:112-121 */
RRT_PRAGMA_UNROLL(RRT_ACC_UNROLL)
    for (int o = 0; o < 5; ++o) {
        if (LUT && RRT_LUT_PAIRS && ((from_table >> o) & 3u) == 3u) {     /* this octave and the next: one round trip */
            const v3 at1 = mk(at.x * 2.05f + 10.0f, at.y * 2.05f + 10.0f, at.z * 2.05f + 10.0f);
            float n0, n1;
            if (BANDED) noise3d_lut_pair2(acc_octave_lut(L, *bands, o), acc_octave_lut(L, *bands, o + 1), at, at1, oob, n0, n1);
            else noise3d_lut_pair(L, at, at1, oob, n0, n1);
            n += amp * n0;
            amp *= 0.5f;
            n += amp * n1;
            at = at1;
            ++o;
        } else if (BANDED && LUT && ((from_table >> o) & 1u)) {
            n += amp * noise3d_sel<LUT>(at, acc_octave_lut(L, *bands, o), true, oob);
        } else {
            n += amp * noise3d_sel<LUT>(at, L, (from_table >> o) & 1u, oob);
        }
        at = mk(at.x * 2.05f + 10.0f, at.y * 2.05f + 10.0f, at.z * 2.05f + 10.0f);
        amp *= 0.5f;
    }
    float streak = fmax2(0.0f, n - 0.32f);
    streak = rrt_powf(streak * 2.8f, 1.6f);
    streak = fmin2(6.0f, streak);
    return envelope * (0.02f + 5.0f * streak);
}
template <bool EARLY_OUT, bool LUT>
RRT_DEV float accretion_density(v3 p, float time, const NoiseLut& L, unsigned* oob) {
    DiskPoint dp;
    if (!disk_point<EARLY_OUT>(p, dp)) return 0.0f;
    return accretion_density_at<EARLY_OUT, LUT>(p, time, dp, L, oob);
}

/* getDustCloudDensity, densities.h:69-132.  LEAN (the render kernels, which call it only inside the cloud zone
 * |y| < 0.75, r < 25: raymarcher.cu:58): the same tame-operand argument as in accretion_density. */
template <bool LUT, bool LEAN = true, bool BANDED = false, int PART = kWhole>       /* PART: see accretion_density_at */
RRT_DEV float dust_density_at(v3 p, float time, DiskPoint& dp, const NoiseLut& L, unsigned* oob, const DustBands* bands = nullptr,
                              const NoiseLut* acc0 = nullptr, float envelope_in = 0.0f) {
    const float rc = dp.rc, q = dp.q;
    float envelope;
    if constexpr (PART == kTail) envelope = envelope_in;
    else {
    const float outer = smoothstep_t<LEAN>(kDiskOut, kDiskOut * 0.8f, rc);
    const float inner = smoothstep_t<LEAN>(kIsco, kIsco + 5.0f, rc);
    const float thick = kCloudH * 0.5f * rrt_powf(q, 0.2f);
    const float slab = rrt_expf(Ar<LEAN>::div(-(p.y * p.y), 2.0f * thick * thick + 1e-7f));
    envelope = slab * outer * inner;
    if (envelope < 0.001f) return 0.0f;                 /* densities.h:85 */
    }
    /* ---- the seam: the envelope is >= 0.001 or a NaN here, never 0 ---- */
    if constexpr (PART == kHead) return envelope;

    const float azimuth = disk_azimuth(p, dp);
    const float kepler = q * dp.sq;                     /* 1.0f * powf(q, 1.5f) */
    const float sheared = azimuth - time * kepler;

    const v3 sc = mk(rc * 0.8f, p.y * 15.0f, sheared * 10.0f);     /* `coords`, :93 */

    /* table switches, wave-uniform: bit 0/1 warp-1 octaves, 2/3 warp-2 octaves, 4.. ridge octaves,
     * 8 detail octave 0; the scales are the factors each family applies to `sc` */
    unsigned from_table = 0u;
    if (LUT) {
        const float sp = lut_spread(sc);
        if (lut_fits(sp, 0.15f)) from_table |= 1u;
        if (lut_fits(sp, 0.15f * 2.05f)) from_table |= 2u;
        if (lut_fits(sp, 0.4f)) from_table |= 4u;
        if (lut_fits(sp, 0.4f * 2.05f)) from_table |= 8u;
        float cells = 1.0f;
#pragma unroll
        for (int k = 0; k < kLutRidgeOctaves; ++k) {
            if (lut_fits(sp, cells)) from_table |= 16u << k;
            cells *= 2.1f;
        }
        if (kLutDetail && lut_fits(sp, 4.0f)) from_table |= 256u;             /* the detail fbm's second octave (8.2 cells per unit) is never coherent */
        from_table &= L.families;
    }

    /* first warp, :95-99: fbm(c, 2), fbm(c + (1,2,3), 2), fbm(c + (4,5,6), 2) with c = sc*0.15
     * (c + 0 for the first: adding +0.0f changes no result, see noise3d) */
    const v3 c15 = mul(sc, 0.15f);
    float wx = 0.f, wy = 0.f, wz = 0.f;
RRT_PRAGMA_UNROLL(RRT_WARP_UNROLL)
    for (int k = 0; k < 3; ++k) {
        const float ox = k == 0 ? 0.0f : (k == 1 ? 1.0f : 4.0f);
        const float oy = k == 0 ? 0.0f : (k == 1 ? 2.0f : 5.0f);
        const float oz = k == 0 ? 0.0f : (k == 1 ? 3.0f : 6.0f);
        const float f = fbm2_sel<LUT>(mk(c15.x + ox, c15.y + oy, c15.z + oz), L, from_table & 1u, from_table & 2u, oob);
        if (k == 0) wx = f; else if (k == 1) wy = f; else wz = f;
    }
    /* second warp, :101-106: offsets (0,0,0), (2,1,0), (0,3,1) on (sc + 3*w1)*0.4 */
    const v3 c40 = mul(add(sc, mul(mk(wx, wy, wz), 3.0f)), 0.4f);
    float vx = 0.f, vy = 0.f, vz = 0.f;
RRT_PRAGMA_UNROLL(RRT_WARP_UNROLL)
    for (int k = 0; k < 3; ++k) {
        const float ox = k == 1 ? 2.0f : 0.0f;
        const float oy = k == 0 ? 0.0f : (k == 1 ? 1.0f : 3.0f);
        const float oz = k == 2 ? 1.0f : 0.0f;
        const float f = fbm2_sel<LUT>(mk(c40.x + ox, c40.y + oy, c40.z + oz), L, from_table & 4u, from_table & 8u, oob);
        if (k == 0) vx = f; else if (k == 1) vy = f; else vz = f;
    }
    const v3 fc = add(sc, mul(mk(vx, vy, vz), 1.5f));              /* `final_coords`, :108 */

    /* BANDED: the boxes of ridge octaves 1, 2 and of the detail octave are those of this sample's omega band */
    const int band = BANDED ? dust_band(*bands, kepler) : 0;

    float n = 0.0f, amp = 1.0f, freq = 1.0f;                       /* ridged sum, :111-120 */
    const unsigned ridge_bits = (from_table >> 4) & ((1u << kLutRidgeOctaves) - 1u);
RRT_PRAGMA_UNROLL(RRT_RIDGE_UNROLL)
    for (int k = 0; k < 5; ++k) {
        /* Exact early-out (round 3, render kernels only): every ridge term is <= amp (1 - |2 noise - 1| <= 1), so the
         * finished sum is <= n + 2 amp (the remaining amplitudes amp, amp/2 ... add up to < 2 amp; the float sum of at
         * most five such terms stays within 1e-6 of that).  If even that gives n * 0.55f <= 0.4f, the smoothstep below
         * is 0, strands is 0 and so is the density: the remaining octaves and the detail fbm cannot change it. */
        if (LEAN && k > 0 && n + 2.0f * amp <= 0.7272f) return 0.0f;
        if (LUT && RRT_LUT_PAIRS && ((ridge_bits >> k) & 3u) == 3u) {
            float n0, n1;
            if (BANDED) {                                          /* octave k from its own box, k + 1 (1 or 2) from its band's */
                const NoiseLut La = k == 0 ? L : band_lut(*acc0, L, *bands, k - 1, band);
                noise3d_lut_pair2(La, band_lut(*acc0, L, *bands, k, band), mul(fc, freq), mul(fc, freq * 2.1f), oob, n0, n1);
            } else {
                noise3d_lut_pair(L, mul(fc, freq), mul(fc, freq * 2.1f), oob, n0, n1);
            }
            n += (1.0f - fabsf(n0 * 2.0f - 1.0f)) * amp;
            amp *= 0.5f;
            freq *= 2.1f;
            n += (1.0f - fabsf(n1 * 2.0f - 1.0f)) * amp;
            ++k;
        } else {
            float nv;
            if (BANDED && LUT && k >= 1 && k <= 2 && ((ridge_bits >> k) & 1u)) nv = noise3d_sel<LUT>(mul(fc, freq), band_lut(*acc0, L, *bands, k - 1, band), true, oob);
            else nv = noise3d_sel<LUT>(mul(fc, freq), L, (ridge_bits >> k) & 1u, oob);
            const float wisp = 1.0f - fabsf(nv * 2.0f - 1.0f);
            n += wisp * amp;
        }
        amp *= 0.5f;
        freq *= 2.1f;
    }
    float strands = smoothstep_t<LEAN>(0.4f, 0.8f, n * 0.55f);
    strands = rrt_powf(strands, 4.0f);
    /* Exact early-out (round 3, render kernels only): detail = fbm(.,2) < 0.75, so the factor below is < 0.9000004 and
     * the result < envelope * strands * 10.800005 (1 + 2e-7); at or under 9.25e-5 that is < 0.000999 <= 0.001f: the
     * caller's `d_cloud > 0.001f` gates (raymarcher.cu:71,91) discard it whatever the detail noise is. */
    if (LEAN && envelope * strands <= 9.25e-5f) return 0.0f;
    const v3 dc = mul(fc, 4.0f);
    const float detail = (BANDED && LUT && (from_table & 256u))
        ? fbm2_sel<LUT>(mk(dc.x + 0.0f, dc.y + time * 0.5f, dc.z + 0.0f), band_lut(*acc0, L, *bands, 2, band), true, false, oob)
        : fbm2_sel<LUT>(mk(dc.x + 0.0f, dc.y + time * 0.5f, dc.z + 0.0f), L, from_table & 256u, false, oob);
    strands *= (0.6f + 0.4f * detail);
    return envelope * strands * 12.0f;
}
template <bool LUT, bool LEAN = true>
RRT_DEV float dust_density(v3 p, float time, const NoiseLut& L, unsigned* oob) {
    DiskPoint dp;
    if (!disk_point<LEAN>(p, dp)) return 0.0f;
    return dust_density_at<LUT, LEAN, false>(p, time, dp, L, oob);
}

/* Both densities of one in-zone sample as the render kernels need them (raymarcher.cu:68-69): the position-only
 * terms are shared (DiskPoint).
 * INVARIANT: the outputs are valid ONLY for comparison with the `d > 0.001f` gates of raymarcher.cu:71,76,91.
 * The early-outs of disk_point / accretion_density_at / dust_density_at (y^2 rc > 135; slab exponent < -10.5;
 * envelope * 30.02 <= 0.001; n + 2 amp <= 0.7272; envelope * strands <= 9.25e-5) return 0 where the literal functions
 * return a small density AT OR UNDER the gate -- bit-equal to the literal value wherever that value exceeds the gate, and
 * merely "<= 0.001" elsewhere.  Every consumer here (sample_emission; the three-pass pool keeps the sample POINTS, never
 * these values) tests the gate and nothing else.  A new consumer of the raw densities -- a debug density output, say --
 * must call the literal instantiations (EARLY_OUT / LEAN = false).  Pinned by tests/test_gpu_units.py::
 * test_early_outs_agree_with_the_literal_densities_through_the_gate on points straddling every threshold. */
/* MEDIA as in the kernels: 1 = arithmetic noise, 2 = dense lattice-hash tables, 3 = tables with the fine dust families banded */
template <int MEDIA>
RRT_DEV void media_densities(v3 p, float time, bool in_disk, bool in_cloud, const NoiseLut& lut_acc, const NoiseLut& lut_dust,
                             const DustBands& bands, unsigned* oob, float& d_disk, float& d_cloud) {
    d_disk = 0.0f; d_cloud = 0.0f;
    DiskPoint dp;
    if (!disk_point<true>(p, dp)) return;
    if (in_disk && !(RRT_PROBE & 1)) d_disk = accretion_density_at<true, MEDIA >= 2, MEDIA == 3>(p, time, dp, lut_acc, oob, &bands);
    if (in_cloud && !(RRT_PROBE & 2)) d_cloud = dust_density_at<MEDIA >= 2, true, MEDIA == 3>(p, time, dp, lut_dust, oob, &bands, &lut_acc);
}

/* ---- radiative transfer of one in-zone sample, raymarcher.cu:67-117 ---- */
struct Radiance { float r, g, b, t; };

/* Emission (ex, ey, ez) and transmittance of one sample; false when the sample contributes nothing
 * (raymarcher.cu:71 not taken).  The reference evaluates calculateRedshiftFactor(rel_p, vel) in both
 * components (:77, :92) with the same arguments; it is evaluated once here. */
/* STORED: the redshift factor -- a function of the sample point, the ray direction and the spin only -- is `stored_g`, kept
 * by a sample record, instead of redshift_factor_r on the raw operands (rel_p, vel and spin are not read then). */
template <bool STORED = false>
RRT_DEV bool sample_emission(float d_disk, float d_cloud, v3 rel_p, float r, v3 vel, float h, float spin,
                             float& ex, float& ey, float& ez, float& step_trans, float stored_g = 0.0f) {
    const bool disk_on = d_disk > 0.001f, dust_on = d_cloud > 0.001f;
    if (!(disk_on || dust_on)) return false;
    if (RRT_PROBE & 4) { ex = d_disk; ey = d_cloud; ez = 0.f; step_trans = 0.99f; return true; }
    /* a density above the gate means the cylindrical radius is in [10, 25] and the sample inside a zone, so
     * r in [10, 30): the tame range of the lean divisions / square roots (their guards fall back otherwise) */
    ex = 0.f; ey = 0.f; ez = 0.f;
    float opacity = 0.f;
    float shift_g;
    if constexpr (STORED) shift_g = stored_g;
    else shift_g = redshift_factor_r<true>(rel_p, r, vel, spin);
    if (disk_on) {                                               /* thermal disk, raymarcher.cu:76-88 */
        const float temp = disk_temperature_t<true>(r);
        const bool tame = temp >= 1.0f;                          /* temp in [6.6e6, 1.5e7] for r in [10, 30) */
        const float rel_temp = tame ? rrt_div_const(temp, kDiskTempRef) : temp / kDiskTempRef;
        const float root_temp = tame ? sqrt_tame(rel_temp) : rrt_powf(rel_temp, 0.5f);
        const float power = rrt_powf(shift_g, 4.0f) * root_temp * d_disk * kDiskLum;
        const float hue = shift_g * rrt_powf(rel_temp, 0.4f) * 2.5f;
        ex += power;                                             /* 1.0f * power */
        ey += fmin2(0.25f, 0.12f * hue) * power;
        ez += fmax2(0.0f, 0.01f * (hue - 2.0f)) * power;
        opacity += d_disk * kDiskOpacity;
    }
    if (dust_on) {                                               /* scattering dust, raymarcher.cu:91-105 */
        const float rr = fmax2(r, kIsco);
        const float lit = 0.5f + 3.0f * rrt_powf(rr < 64.0f ? rrt_div_tame(kIsco, rr) : kIsco / rr, 1.2f);
        const float glow = d_cloud * kCloudLum * lit;
        /* smoothstep(0.7f, 1.3f, g), math_utils.h:45-48: a constant divisor; g has no upper bound (the Doppler
         * denominator can vanish), so the three-instruction divide is kept to dividends it is checked for */
        const float grade_q = fabsf(shift_g) < 1.0e9f ? rrt_div_const(shift_g - 0.7f, 1.3f - 0.7f) : (shift_g - 0.7f) / (1.3f - 0.7f);
        const float grade_t = fmin2(fmax2(grade_q, 0.0f), 1.0f);
        const float grade = grade_t * grade_t * (3.0f - 2.0f * grade_t);
        ex += 0.60f * glow * lerp(1.2f, 0.8f, grade);
        ey += 0.65f * glow * lerp(0.8f, 1.1f, grade);
        ez += 0.80f * glow * lerp(0.6f, 1.4f, grade);
        opacity += d_cloud * kCloudOpacity;
    }
    step_trans = rrt_expf(-(opacity * h));                       /* Beer-Lambert factor of this step, :107-108 */
    return true;
}

/* ---- sample records: what `time` cannot move of one retained sample (the march cache) ----
 * A retained sample is a fixed point with a fixed ray direction, and `time` enters its evaluation in five places only, all of
 * them in the densities' tails (turned, drift, sheared, the detail fbm twice).  Everything above the seams is a function of
 * (rel_p, vel, spin) and of the arithmetic that produced `r`: the cache's fill derives it once (sample_record) and every
 * replayed frame starts from it (eval_sample_record).
 *   rc, y, azimuth   what the tails read of the position (q and sq are recomputed from rc: one divide, one root)
 *   shift_g          redshift_factor_r<true> on the raw operands: its fall-back branch, and the NaN a non-finite vel.y travels
 *                    as (kRowPlanes), arrive exactly as sample_emission would have computed them
 *   r                the march's radius: disk_temperature, the dust's `lit`, and with y the zone rule for the step length
 *   env_acc, env_dust   the heads' envelopes; +0 wherever the literal path returns density 0 before it reaches `time` --
 *                    outside the zone, disk_point false, slab_arg < -10.5, envelope * 30.02 <= 0.001, dust envelope < 0.001.
 *                    An envelope that reaches its seam is never 0 (see there), so `!= 0` IS the early-out's branch.
 * A sample whose two envelopes are both +0 has both densities 0 at every `time`: it can never be taken (prunable). */
struct SampleRecord { float rc, y, azimuth, shift_g, r, env_acc, env_dust; };

RRT_DEV bool record_prunable(const SampleRecord& s) { return !(s.env_acc != 0.0f || s.env_dust != 0.0f); }

RRT_DEV SampleRecord sample_record(v3 rel_p, float r, v3 vel, float spin) {
    SampleRecord s;
    s.rc = 0.0f; s.y = rel_p.y; s.azimuth = 0.0f; s.shift_g = 0.0f; s.r = r; s.env_acc = 0.0f; s.env_dust = 0.0f;
    const bool in_disk = fabsf(rel_p.y) < kDiskH * 5.0f && r < kDiskOut + 5.0f;
    const bool in_cloud = fabsf(rel_p.y) < kCloudH * 1.5f && r < kCloudOut;
    DiskPoint dp;
    if (!disk_point<true>(rel_p, dp)) return s;
    s.rc = dp.rc;
    const NoiseLut none{};
    if (in_disk && !(RRT_PROBE & 1)) s.env_acc = accretion_density_at<true, false, false, kHead>(rel_p, 0.0f, dp, none, nullptr);
    if (in_cloud && !(RRT_PROBE & 2)) s.env_dust = dust_density_at<false, true, false, kHead>(rel_p, 0.0f, dp, none, nullptr);
    if (record_prunable(s)) return s;
    s.azimuth = disk_azimuth(rel_p, dp);
    s.shift_g = redshift_factor_r<true>(rel_p, r, vel, spin);
    return s;
}

/* the length of the sample's march step, by the zone rule (raymarcher.cu:56-62) */
RRT_DEV float record_step(const SampleRecord& s, float h_near, float h_disk, float h_vac) {
    const bool near_bh = s.r < 18.0f;
    const bool in_disk = fabsf(s.y) < kDiskH * 5.0f && s.r < kDiskOut + 5.0f;
    return near_bh ? h_near : (in_disk ? h_disk : h_vac);
}

/* media_densities + sample_emission of one sample, from its record; h: record_step */
template <int MEDIA>
RRT_DEV bool eval_sample_record(const SampleRecord& s, float time, float h, const NoiseLut& lut_acc, const NoiseLut& lut_dust,
                                const DustBands& bands, float& ex, float& ey, float& ez, float& step_trans) {
    if (record_prunable(s)) return false;
    DiskPoint dp;
    dp.rc = s.rc;
    dp.q = Ar<true>::div(kIsco, s.rc);                  /* as disk_point: an envelope that is not 0 means rc in [10, 25] */
    dp.sq = Ar<true>::sqrt(dp.q);
    dp.azimuth = s.azimuth; dp.has_azimuth = true;
    const v3 p = mk(0.0f, s.y, 0.0f);                   /* the tails read p.y only */
    float d_disk = 0.0f, d_cloud = 0.0f;
    if (s.env_acc != 0.0f) d_disk = accretion_density_at<true, MEDIA >= 2, MEDIA == 3, kTail>(p, time, dp, lut_acc, nullptr, &bands, s.env_acc);
    if (s.env_dust != 0.0f) d_cloud = dust_density_at<MEDIA >= 2, true, MEDIA == 3, kTail>(p, time, dp, lut_dust, nullptr, &bands, &lut_acc, s.env_dust);
    return sample_emission<true>(d_disk, d_cloud, p, s.r, p, h, 0.0f, ex, ey, ez, step_trans, s.shift_g);
}

/* Beer-Lambert accumulation of one sample, raymarcher.cu:109-115 */
RRT_DEV void accumulate_emission(Radiance& acc, float ex, float ey, float ez, float step_trans) {
    float factor = (1.0f - step_trans) * acc.t;
    acc.r += ex * factor;
    acc.g += ey * factor;
    acc.b += ez * factor;
    acc.t *= step_trans;
}

RRT_DEV void accumulate_sample(Radiance& acc, float d_disk, float d_cloud, v3 rel_p, float r, v3 vel,
                               float h, float spin) {
    float ex, ey, ez, s;
    if (!sample_emission(d_disk, d_cloud, rel_p, r, vel, h, spin, ex, ey, ez, s)) return;
    accumulate_emission(acc, ex, ey, ez, s);
}

/* ---- per-pixel camera effects, camera_effects/post_processing.h:13-31 ---- */
RRT_DEV void lens_distort(float& uvx, float& uvy, float k) {                 /* apply_lens_distortion :19-24 */
    const float tx = uvx - 0.5f, ty = uvy - 0.5f;
    const float r2 = tx * tx + ty * ty;
    const float f = 1.0f + r2 * k;
    uvx = tx * f + 0.5f;
    uvy = ty * f + 0.5f;
}
RRT_DEV v3 bloom_part(v3 c, float threshold) {                               /* get_bloom_contribution :27-31 */
    const float luma = c.x * 0.2126f + c.y * 0.7152f + c.z * 0.0722f;
    const bool on = luma > threshold;
    return mk(on ? c.x : 0.f, on ? c.y : 0.f, on ? c.z : 0.f);
}
RRT_DEV v3 vignette(v3 c, float uvx, float uvy, float intensity) {           /* apply_vignette :13-17 */
    const float dx = uvx - 0.5f, dy = uvy - 0.5f;
    const float dist = sqrtf(dx * dx + dy * dy + 0.0f * 0.0f);
    const float vg = smoothstep(0.8f, 0.2f, dist * intensity);
    return mul(c, vg);
}

/* ---- sky lookup (replaces tex2D<float4>, raymarcher.cu:134-146; the filter is the
 *      build's definition, identical to oracle/rrt_oracle.c:sky_fetch) ---- */
struct SkyTex { const uint8_t* texels; int w, h, frac_bits; };

RRT_DEV int wrapi(int i, int n) { int m = i % n; return m < 0 ? m + n : m; }
RRT_DEV int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

RRT_DEV void sky_fetch(const SkyTex& s, float tx, float ty, float out[4]) {
    float xb = tx * (float)s.w - 0.5f;
    float yb = ty * (float)s.h - 0.5f;
    float fi = floorf(xb), fj = floorf(yb);
    float a = xb - fi, b = yb - fj;
    if (s.frac_bits > 0) {
        float q = (float)(1 << s.frac_bits);
        a = floorf(a * q + 0.5f) / q;
        b = floorf(b * q + 0.5f) / q;
    }
    int i0 = wrapi((int)fi, s.w), i1 = wrapi((int)fi + 1, s.w);
    int j0 = clampi((int)fj, 0, s.h - 1), j1 = clampi((int)fj + 1, 0, s.h - 1);
    float w00 = (1.0f - a) * (1.0f - b);
    float w10 = a * (1.0f - b);
    float w01 = (1.0f - a) * b;
    float w11 = a * b;
    const uint32_t* t = reinterpret_cast<const uint32_t*>(s.texels);
    uint32_t t00 = t[(size_t)j0 * s.w + i0], t10 = t[(size_t)j0 * s.w + i1];
    uint32_t t01 = t[(size_t)j1 * s.w + i0], t11 = t[(size_t)j1 * s.w + i1];
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) {
        float c00 = (float)((t00 >> (8 * ch)) & 255u) / 255.0f;
        float c10 = (float)((t10 >> (8 * ch)) & 255u) / 255.0f;
        float c01 = (float)((t01 >> (8 * ch)) & 255u) / 255.0f;
        float c11 = (float)((t11 >> (8 * ch)) & 255u) / 255.0f;
        out[ch] = w00 * c00 + w10 * c10 + w01 * c01 + w11 * c11;
    }
}

RRT_DEV void sample_sky(const SkyTex& s, v3 dir, float off, float out[4]) {
    float phi = rrt_atan2f(dir.z, dir.x) + off;
    float theta = rrt_asinf(dir.y);
    float tx = 0.5f + phi / (2.0f * kPi);
    float ty = 0.5f - theta / kPi;
    sky_fetch(s, tx, ty, out);
}

}  // namespace rrt
#endif
