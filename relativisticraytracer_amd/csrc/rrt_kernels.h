/*
 * rrt_kernels.h -- the gfx950 kernels of the render path and the structures they share with the host side.
 *
 * A SECTION of rrt_hip.hip (included once, inside its anonymous namespace, after `using namespace rrt`): without relocatable
 * device code a kernel and its launch site have to share a translation unit, so the split is textual -- device code here, host
 * registries / launch logic / C ABI in rrt_hip.hip, camera host code in rrt_camera.cpp, test hooks in rrt_test_hooks.h.
 *
 * Replaces the reference's only kernel, raymarch_kernel (src/raymarcher.cu:15-174):
 *   raymarch_pixels<SPIN,MEDIA,DEBUG,ARITH>   single-kernel path: one ray per lane, media sampled in line
 *   march_defer / eval_sample_rows / composite_and_shade (/ pool_next_round, zero_words)
 *                                             three-pass path through a caller-owned workspace, in rounds, as two chains;
 *                                             with KEEP: passes 2 and 3 over the march cache's retained rows (KeepArgs)
 *   supersample_pixels / panorama_pixels / stereo_pixels / motion_pixels      the sampled launches over a virtual (s w) x (s h) frame
 *   adaptive_mask (rrt_adaptive.h) / refine_pixels<SPIN,MEDIA,ARITH,RAY>      adaptive supersampling: list the aliasing pixels, refine them
 *   probe_costs / probe_to_tiles              coarse march-only probe of a view: first-frame dispatch order, row-tile costs
 *   clock_probe_kernel                        the shader clock the chip holds
 *   assemble_tiles_kernel / assemble_all_kernel / assemble_map_kernel   scatter gathered row-tile shards into the frame
 *   build_noise_table                         the lattice-hash tables (rrt_noise_table)
 */
#ifndef RRT_KERNELS_H
#define RRT_KERNELS_H

/* ------------------------------------------------------------------ deferred-sampling workspace
 * Three-pass path: pass 1 marches the geodesics only and appends the in-medium
 * sample points of a wavefront, one 64-lane "row" per march step that needs one, to a bump-allocated
 * pool in HBM; pass 2 evaluates the densities + emission of every row with the whole chip, wherever
 * the row came from; pass 3 composites each ray's samples in march order and shades the pixel.
 * The pool is handed out in blocks of kBlockRows rows, and blocks in runs of consecutive blocks whose
 * length doubles (1, 2, 4 ... kMaxRun = 8) every time a wave comes back for more: one atomic per run (a
 * single counter saturates near 90 atomics/us) and only ~log2(n) dependent pointer hops when pass 3
 * walks a heavy wave's samples.  Block layout: kBlockRows x five SoA float[64] planes (p.xyz, vel.x, vel.z in;
 * ex, ey, ez, transmittance out in planes 0-3), then a trailer {lane mask of each row; in the first
 * block of a run: start and length of the wave's next run}.  Unused rows keep a zero mask. */
/* Round 4: the pool is reused in ROUNDS.  A round = march until the pool is full (waves the pool ran out under are
 * SUSPENDED: pre-step state and the radiance composited so far are saved per ray) -> evaluate the pooled rows -> composite
 * them; the next round resumes the suspended waves into the emptied pool.  Any pool serves any view; the in-line fall-back
 * only finishes what is still suspended after the last round the host enqueued. */
struct DeferCounters {
    unsigned next_block, overflow_waves;      /* of the current round */
    unsigned last_overflow;                   /* waves suspended when this round started (0: nothing left to do) */
    unsigned rounds_run, rounds_with_work;    /* rounds enqueued so far / rounds whose march had something to do */
    unsigned peak_blocks;                     /* most blocks any round used */
    unsigned suspended_left;                  /* waves still suspended after the last round: finished in line */
    unsigned pruned_lanes;                    /* march cache fill: lanes cleared from the rows' input masks (was padding) */
    unsigned long long total_blocks;
};
/* state: 0 untouched, 1 marched to its end this round, 2 suspended (the pool ran out under it), 3 shaded.
 * flags bit 0: the rays' radiance so far is saved in `finals` (planes 7-10). */
struct WaveHdr { unsigned first_block, n_runs, state, flags; };
/* Longest run of blocks a wave takes at once.  Runs double (1, 2, 4 ...) up to this, and a wave's last run is on average half
 * empty: with 32 (rounds 1-3) an eighth of the 4K frame from inside the disk allocated 1.46 M rows for 1.2 M samples' worth and
 * needed a second -- sparse, latency-bound -- round in a 2 GiB pool; with 8 it allocates 1.28 M, fits, and takes 7.9 instead of
 * 9.6 ms; the bench view is indifferent (profiles/r04_max_run_ab.txt).  Shorter runs mean more atomics (one per run: ~20 k per
 * such frame, spread over milliseconds) and more link hops in pass 3 (a 2000-row wave: 32 instead of 12). */
#ifndef RRT_MAX_RUN
#define RRT_MAX_RUN 8
#endif
constexpr unsigned kMaxRun = RRT_MAX_RUN;
constexpr unsigned kMaxRunsWalked = 4096;                          /* runs of one wave that pass 3 will walk */
constexpr unsigned kBlockRows = 8;
/* Round 5: a row is FIVE float[64] planes in (p.xyz, vel.x, vel.z), was six.  The only consumer of the sample's velocity is
 * calculateRedshiftFactor's cos_theta = dot(ray_vel, gas_dir) (geodesics.h:18-19), and gas_dir.y is +0 exactly (0 / mag), so
 * vel.y only ever enters as vel.y * 0 = +-0 added to vel.x * gas_dir.x: it can change the sign of a zero cos_theta and nothing
 * else (1 - v * (+-0) = 1) -- unless vel.y is not finite, when the product is NaN; the march poisons vel.x with NaN in that
 * case, which makes cos_theta the same NaN.  17 % less pool traffic on the way in (profiles/r05_pass_counters_*.txt).
 * The march cache's retained rows keep the five planes but not their meaning: its fill rewrites them to (rc, p.y, azimuth,
 * shift_g, r) -- a sample record, see kOutBlockEnv below; the NaN in vel.x has become the NaN in shift_g by then. */
constexpr unsigned kRowPlanes = 5;
constexpr unsigned kRowData = kRowPlanes * 256;
constexpr unsigned kBlockTrailer = kBlockRows * kRowData;         /* masks[kBlockRows] (u64), then next (u32) */
constexpr unsigned kBlockBytes = kBlockTrailer + kBlockRows * 8 + 64;
constexpr unsigned kNoBlock = 0xffffffffu;

constexpr int kMaxChains = 2;
constexpr size_t kCounterStride = 64;      /* bytes between the chains' DeferCounters at the head of the workspace */
static_assert(sizeof(DeferCounters) <= kCounterStride, "one counter block per chain");
/* Retained geodesics (the march cache): passes 2 and 3 instantiated with KEEP keep a row's place --
 * pass 2 writes (ex, ey, ez, transmittance) and the row's live mask to planes of their own, block b of the pool's slice at
 * out_blocks + b * kOutBlockBytes: kBlockRows x four float[64] planes, then the kBlockRows masks, then the records' envelope
 * planes (kOutBlockEnv) -- and pass 3 reads the first two there
 * (the links between a wave's runs stay in the input blocks).  `replay`: the rows are those an earlier launch's pass 1 left;
 * n_blocks of the slice are in use, every wave has marched to its end, the headers and counters are not written. */
struct KeepArgs {
    uint8_t* out_blocks;
    unsigned n_blocks;
    int replay;
};
/* Blocks a replaying wave of pass 2 takes from the cursor at once (round 11, profiles/r11_replay_handout_ab.txt).  One counter
 * saturates near 90 atomics per microsecond (kMaxRun above) and the 4K bench frame hands out 210 k blocks in ~2.5 ms: with 1 the
 * replay runs at the counter's rate (3.26 ms, whatever else is resident; the static stride took 3.1-3.2 alone); with 2 it takes
 * 2.84-2.96 ms; with 4 the last helpings are too coarse, 3.01-3.09.  Chunks that shrink towards the end (from 2: 2.86-2.96, from
 * 4: 2.99-3.08) did not separate from the fixed 2. */
#ifndef RRT_REPLAY_CHUNK
#define RRT_REPLAY_CHUNK 2
#endif
constexpr unsigned kReplayChunk = RRT_REPLAY_CHUNK;
constexpr unsigned kOutRowData = 4 * 256;
constexpr unsigned kOutBlockMasks = kBlockRows * kOutRowData;
/* Sample records (rrt_device.h: SampleRecord).  The fill's pass 2 (KEEP, !replay) rewrites every retained row in place -- same
 * lanes, same five planes -- from the raw (p.xyz, vel.x, vel.z) the march left to (rc, p.y, azimuth, shift_g, r), and puts the
 * two envelopes in two more planes per row behind the out-block's masks; it clears the lanes that can never be taken from the
 * row's input mask (pass 3 reads the out-masks only).  A replay evaluates records; a fill the pool ran out under is never
 * replayed (rrt_mc::Policy::fill_verified) and the refill's march writes raw rows again, so no pass ever meets a row of the
 * other kind. */
constexpr unsigned kOutEnvData = 2 * 256;
constexpr unsigned kOutBlockEnv = kOutBlockMasks + kBlockRows * 8;
constexpr unsigned kOutBlockBytes = kOutBlockEnv + kBlockRows * kOutEnvData;
/* ------------------------------------------------------------------ lattice-hash tables: box of lattice points, fill kernel */
struct LutBox { int x0, y0, z0, nx, ny, nz; };

__global__ __launch_bounds__(256) void build_noise_table(float4* cells, LutBox b) {
    const size_t n = (size_t)b.nx * b.ny * b.nz;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % b.nx), y = (int)((i / b.nx) % b.ny), z = (int)(i / ((size_t)b.nx * b.ny));
        /* "+ 0.0f": the lattice coordinate as noise3d() forms it (ix + 0.0f, ix + 1.0f; rrt_device.h) */
        const float fx = (float)(x + b.x0) + 0.0f, fy = (float)(y + b.y0) + 0.0f, fz = (float)(z + b.z0) + 0.0f;
        const float h00 = hash31(fx, fy, fz), h10 = hash31(fx + 1.0f, fy, fz);
        const float h01 = hash31(fx, fy + 1.0f, fz), h11 = hash31(fx + 1.0f, fy + 1.0f, fz);
        cells[i] = make_float4(h00, h10 - h00, h01, h11 - h01);
    }
}

/* ------------------------------------------------------------------ kernel arguments */
struct RowMap {        /* local row -> image row, and where its pixels go */
    int n_local_rows;  /* rows rendered by this launch                               */
    int y_base;        /* first image row of tile 0 of shard 0                        */
    int tile_rows;     /* R                                                           */
    int shard;         /* s                                                           */
    int n_shards;      /* G: local tile k is image tile s + k*G                       */
    const int* tile_of_local;   /* rrt_tile_map: local tile k is image tile tile_of_local[k] (increasing); NULL: the rule above */
};

struct FrameArgs {
    uchar4* out;
    int width, height;
    float time;
    rrt_camera cam;
    SkyTex sky;
    /* effects (camera_settings.h) */
    int use_bloom, use_vignette, use_ca, use_lens;
    float bloom_threshold, bloom_intensity, vignette_intensity, ca_amount, distortion_amount;
    /* params */
    float spin, drag_c;
    int max_steps;
    int nudge_ulps; unsigned nudge_seed;      /* rrt_params.nudge_ulps / .nudge_seed: the conditioning probe (primary_ray) */
    RowMap rows;
    rrt_debug_outputs dbg;
    /* deferred-sampling workspace (three-pass path), all NULL for the single-kernel path */
    struct DeferCounters* ctr;
    struct WaveHdr* hdr;
    float* finals;          /* 7 arrays of n_lanes: vx, vy, vz, code (steps | hit << 31 | resume << 30), px, py, pz */
    size_t n_lanes;
    uint8_t* sample_blocks;
    unsigned block_capacity;
    /* lattice-hash tables (rrt_noise_table); only read by the kernels instantiated with MEDIA >= 2; dust_bands only with
     * MEDIA == 3 (the fine dust families in per-omega-band boxes: rrt_device.h, DustBands) */
    NoiseLut lut_acc, lut_dust;
    DustBands dust_bands;
    /* cost-ordered dispatch of the single-kernel path (rrt_tile_order): dispatch slot -> wave tile, and where a wave
     * leaves the clocks it took; both NULL: the static centre-out order */
    const unsigned* tile_perm;
    unsigned* tile_cost;
    int tile_order_id;      /* host side only: rrt_params.tile_order */
    /* a launch that covers only dispatch rows grid_row_base + k * grid_row_stride, k < gridDim.y, of a frame's grid_rows rows
     * of wave tiles (the three-pass path's chains, round 4; stride 2 = every other row, round 5); grid_rows == 0: the kernel's
     * own grid is the whole launch */
    int grid_rows, grid_row_base, grid_row_stride;
};

/* image row of local row `lr`, and the local output row it is stored at */
__device__ __forceinline__ bool map_row(const RowMap& m, int height, int lr, int& y, int& out_row) {
    if (lr >= m.n_local_rows) return false;
    int k = lr / m.tile_rows;
    int rr = lr - k * m.tile_rows;
    int t = m.tile_of_local ? m.tile_of_local[k] : m.shard + k * m.n_shards;
    int ty0 = m.y_base + t * m.tile_rows;
    y = ty0 + rr;
    if (y >= height) return false;
    int rows_k = min(m.tile_rows, height - ty0);
    out_row = k * m.tile_rows + (rows_k - 1 - rr);     /* each tile bottom-up, raymarcher.cu:168 */
    return true;
}

/* v moved by k ulps, k uniform in [-K, K] from a 32-bit mix of (x, y, seed, component).  The bit pattern is stepped as a
 * sign-magnitude integer, so a step across zero lands on the small float of the other sign; never used on non-finite v. */
__device__ __forceinline__ uint32_t nudge_mix(uint32_t v) {
    v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
    return v;
}
__device__ __forceinline__ float nudge_component(float v, int K, unsigned seed, int x, int y, unsigned comp) {
    const uint32_t h = nudge_mix(nudge_mix((uint32_t)x * 0x9e3779b1u + (uint32_t)y) ^ (seed * 0x85ebca6bu + comp * 0xc2b2ae35u));
    const int k = (int)(h % (uint32_t)(2 * K + 1)) - K;
    const uint32_t b = rrt_f2u(v);
    int m = (int)(b & 0x7fffffffu);                  /* magnitude as an integer; sign apart */
    m = (b >> 31) ? -m : m;
    m += k;
    const uint32_t out = m < 0 ? (0x80000000u | (uint32_t)(-m)) : (uint32_t)m;
    return rrt_u2f(out);
}
/* The conditioning probe (rrt_params.nudge_ulps; oracle: rrto_nudge_direction, the same function): every component of the unit
 * direction of pixel (x, y) -- of the virtual, eye-local pixel in a sampled launch -- moves by a whole number of ulps in [-K, K]
 * drawn from a hash of (x, y, seed, component).  K == 0, every frame but a probe's: nothing. */
__device__ __forceinline__ void nudge_direction(v3& vel, int K, unsigned seed, int x, int y) {
    if (__builtin_expect(K != 0, 0)) {
        vel.x = nudge_component(vel.x, K, seed, x, y, 0u);
        vel.y = nudge_component(vel.y, K, seed, x, y, 1u);
        vel.z = nudge_component(vel.z, K, seed, x, y, 2u);
    }
}

/* Primary ray of pixel (x, y): raymarcher.cu:20-34 (+ lens distortion, post_processing.h:19-24). */
__device__ __forceinline__ void primary_ray(const FrameArgs& a, int x, int y, float& uvx, float& uvy, v3& p, v3& vel) {
    uvx = (float)x / (float)a.width;
    uvy = (float)y / (float)a.height;
    if (a.use_lens) lens_distort(uvx, uvy, a.distortion_amount);
    float u_coord = uvx * 2.0f - 1.0f;
    float v_coord = uvy * 2.0f - 1.0f;
    float aspect = (float)a.width / (float)a.height;
    u_coord *= aspect;
    const v3 cfw = mk(a.cam.forward[0], a.cam.forward[1], a.cam.forward[2]);
    const v3 crt = mk(a.cam.right[0], a.cam.right[1], a.cam.right[2]);
    const v3 cup = mk(a.cam.up[0], a.cam.up[1], a.cam.up[2]);
    p = mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]);
    vel = normalize(add(cfw, add(mul(crt, u_coord), mul(cup, v_coord))));
    nudge_direction(vel, a.nudge_ulps, a.nudge_seed, x, y);
}

/* Everything after the march up to the tone map: sky, composition, post-FX -- raymarcher.cu:124-161.  The ray's HDR value
 * (rrt_debug_outputs.d_hdr). */
__device__ __forceinline__ v3 shade_hdr(const FrameArgs& a, float uvx, float uvy, bool hit, v3 vel, Radiance acc) {
    float bg_r = 0.f, bg_g = 0.f, bg_b = 0.f;
    if (!hit) {
        v3 d = normalize(vel);
        float s[4];
        if (a.use_ca) {
            sample_sky(a.sky, d, a.ca_amount, s);  bg_r = s[0];
            sample_sky(a.sky, d, 0.0f, s);         bg_g = s[1];
            sample_sky(a.sky, d, -a.ca_amount, s); bg_b = s[2];
        } else {                                   /* offset 0: the three lookups coincide */
            sample_sky(a.sky, d, 0.0f, s);
            bg_r = s[0]; bg_g = s[1]; bg_b = s[2];
        }
    }
    float hx = acc.r + bg_r * acc.t;
    float hy = acc.g + bg_g * acc.t;
    float hz = acc.b + bg_b * acc.t;

    /* raymarcher.cu:154-161, post_processing.h:13-31 */
    if (a.use_bloom) {
        const v3 bl = bloom_part(mk(hx, hy, hz), a.bloom_threshold);
        hx = hx + bl.x * a.bloom_intensity;
        hy = hy + bl.y * a.bloom_intensity;
        hz = hz + bl.z * a.bloom_intensity;
    }
    if (a.use_vignette) {
        const v3 vg = vignette(mk(hx, hy, hz), uvx, uvy, a.vignette_intensity);
        hx = vg.x; hy = vg.y; hz = vg.z;
    }
    return mk(hx, hy, hz);
}

/* Tone map of an HDR value (before the u8 cast) and the RGBA8 store -- raymarcher.cu:164-173. */
__device__ __forceinline__ void tone_map(v3 hdr, float& out_r, float& out_g, float& out_b) {
    out_r = 1.0f - rrt_expf(-hdr.x * kExposure);
    out_g = 1.0f - rrt_expf(-hdr.y * kExposure);
    out_b = 1.0f - rrt_expf(-hdr.z * kExposure);
}
__device__ __forceinline__ void store_rgba8(uchar4* out, size_t oi, float out_r, float out_g, float out_b) {
    out[oi] = make_uchar4((unsigned char)(int)(out_r * 255.0f), (unsigned char)(int)(out_g * 255.0f),
                          (unsigned char)(int)(out_b * 255.0f), 255);
}

/* Everything after the march: sky, composition, post-FX, tone map, RGBA8 store -- raymarcher.cu:124-173. */
template <bool DEBUG>
__device__ __forceinline__ void shade_and_store(const FrameArgs& a, int x, int y, int out_row, float uvx, float uvy,
                                                bool hit, v3 p, v3 vel, Radiance acc, int steps) {
    const v3 c = shade_hdr(a, uvx, uvy, hit, vel, acc);
    const float hx = c.x, hy = c.y, hz = c.z;
    float out_r, out_g, out_b;
    tone_map(c, out_r, out_g, out_b);
    const size_t oi = (size_t)out_row * a.width + x;
    store_rgba8(a.out, oi, out_r, out_g, out_b);
    if (DEBUG) {
        const size_t di = (size_t)y * a.width + x;
        if (a.dbg.d_ldr) { float* q = a.dbg.d_ldr + 4 * oi; q[0] = out_r; q[1] = out_g; q[2] = out_b; q[3] = 1.0f; }
        if (a.dbg.d_hdr) { float* q = a.dbg.d_hdr + 4 * oi; q[0] = hx; q[1] = hy; q[2] = hz; q[3] = 1.0f; }
        if (a.dbg.d_steps) a.dbg.d_steps[di] = steps;
        if (a.dbg.d_hit) a.dbg.d_hit[di] = hit ? 1 : 0;
        if (a.dbg.d_pos) { float* q = a.dbg.d_pos + 3 * di; q[0] = p.x; q[1] = p.y; q[2] = p.z; }
        if (a.dbg.d_vel) { float* q = a.dbg.d_vel + 3 * di; q[0] = vel.x; q[1] = vel.y; q[2] = vel.z; }
        if (a.dbg.d_rad) { float* q = a.dbg.d_rad + 4 * di; q[0] = acc.r; q[1] = acc.g; q[2] = acc.b; q[3] = acc.t; }
    }
}

/* The step size takes three values (the `in_cloud_zone` arm of raymarcher.cu:62 is unreachable: the
 * cloud zone lies inside the disk zone); h*0.5f and h/6.0f (integrators.h:31,57) are folded per value
 * at compile time. */
constexpr float kHVac = kStepSize, kHNear = kStepSize * 0.1f, kHDisk = kStepSize * 0.3f;

/*
 * Per-pixel pipeline, one ray per lane (reference raymarch_kernel, src/raymarcher.cu:15-174).
 * A wavefront covers an 8x8 pixel tile (the workgroup geometry is further down) so that its 64 rays
 * stay spatially coherent (similar step counts, similar zone entry).
 */
/* radius of a position exactly as the march sees it (strict: correctly rounded root of the unfused r2; FMAD: the
 * correctly rounded root of the fused r2; fast: r2*rsq), with the `r2 < 1` case of geodesic_acc().  The loop top of the
 * fast march, pass 2's samples and the unit hooks; the lean loop has its own seeded roots (rrt_device.h: sqrt_seeded_yh). */
constexpr int kArithStrict = RRT_ARITH_STRICT, kArithFast = RRT_ARITH_FAST, kArithFmad = RRT_ARITH_FMAD;
template <int ARITH>
__device__ __forceinline__ void march_radius(v3 rel_p, float& r2, float& r, float& y) {
    if (ARITH == kArithFast) {
        r2 = dot_fma(rel_p, rel_p);
        y = __builtin_amdgcn_rsqf(r2);
        r = r2 * y;
    } else {
        r2 = ARITH == kArithFmad ? dot_fma(rel_p, rel_p) : dot(rel_p, rel_p);
        sqrt_rsq(r2, r, y);
    }
    if (__builtin_expect(__any(!(r2 >= 1.0f)), 0)) {
        if (!(r2 >= 1.0f)) { r = sqrtf(r2); y = 1.0f; }
    }
}

/* Step size of raymarcher.cu:54-62 from the zone flags; h*0.5f is exact, h/6.0f is folded per value. */
__device__ __forceinline__ void zone_step(bool near_bh, bool in_disk, float& h, float& hh, float& h6) {
    h = near_bh ? kHNear : (in_disk ? kHDisk : kHVac);
    hh = 0.5f * h;                                      /* == h * 0.5f of integrators.h:31, one multiply */
    h6 = near_bh ? kHNear / 6.0f : (in_disk ? kHDisk / 6.0f : kHVac / 6.0f);
}

/* r >= kVacuumR rules out the horizon test (r < 2.02) and every zone of raymarcher.cu:56-58 (near_bh r < 18, disk zone
 * r < 30, cloud zone r < 25): the step is h = STEP_SIZE_M with no media sample.  About nine steps in ten of the bench
 * frame are taken by wavefronts whose 64 rays are all out there. */
constexpr float kVacuumR = kDiskOut + 5.0f;

/* The whole march of one ray with the media sampled in line: raymarcher.cu:41-121.
 * MEDIA: 0 = densities read 0 ("skybox only"), 1 = full media, 2 = full media with the lattice-hash tables, 3 = with the
 * tables in their banded layout (rrt_device.h: DustBands).
 * `i`: in = first step (0, or where a resumed ray stopped), out = steps taken.  When every lane starts at the
 * same step the loop counter stays in a scalar register; the per-ray count is written once, at the exit.
 *
 * The loop of RRT_ARITH_FAST (not the parity path): one flat loop, v_rsq radius, integrate_rk4_fast (rrt_device.h).  (A step
 * without the per-stage `r < 1` guards -- 5 fewer vector instructions, repeated with guards in the unreachable case -- was
 * measured and dropped: the longer basic blocks it leaves let the scheduler interleave independent chains, and on gfx950 a
 * VALU instruction issued 2-6 slots after its producer costs 10-15 % more than one issued right behind it;
 * profiles/README.md, round 2.) */
template <bool SPIN, int MEDIA>
__device__ __forceinline__ void march_inline_fast(const FrameArgs& a, v3& p, v3& vel, Radiance& acc, bool& hit, int& i,
                                                  unsigned* oob) {
    int steps = i > a.max_steps ? i : a.max_steps;      /* if the loop runs out */
    for (int k = i; k < a.max_steps; ++k) {
        const v3 rel_p = p;                             /* p - MASS_POS, MASS_POS = 0 */
        float r2, r, y;
        march_radius<kArithFast>(rel_p, r2, r, y);
        if (r < kEventHorizon * 1.01f) { hit = true; acc.t = 0.0f; steps = k; break; }

        const bool near_bh = r < 18.0f;
        const bool in_disk = fabsf(rel_p.y) < kDiskH * 5.0f && r < kDiskOut + 5.0f;
        const bool in_cloud = fabsf(rel_p.y) < kCloudH * 1.5f && r < kCloudOut;
        float h, hh, h6;
        zone_step(near_bh, in_disk, h, hh, h6);

        integrate_rk4_fast<SPIN>(p, vel, h, hh, h6, a.drag_c, r2, y);

        if (MEDIA != 0 && (in_disk || in_cloud)) {
            float d_disk, d_cloud;
            media_densities<MEDIA>(rel_p, a.time, in_disk, in_cloud, a.lut_acc, a.lut_dust, a.dust_bands, oob, d_disk, d_cloud);
            accumulate_sample(acc, d_disk, d_cloud, rel_p, r, vel, h, a.spin);
        }
        if (r > 250.0f && dot(rel_p, vel) > 0.0f) { steps = k + 1; break; }
    }
    i = steps;
}

/* The vacuum steps of a wavefront run in a loop of their own, every exit of which is wave-uniform.  In a flat loop the vacuum
 * and the generic path meet before the back edge, and the step that is taken nine times in ten pays the register copies of
 * that meeting (FMAD: 14 v_mov on 221 arithmetic instructions; strict: 5 on 278).  Here the
 * loop-carried state has one producer; with the body written out twice a step can write its results into the registers of
 * the state before last, which the escape test (pre-step position, post-step velocity: raymarcher.cu:120) has released by
 * then: 216 VALU per FMAD vacuum step, 276 strict, no copy left (tools/isa_histogram.py; 4K bench frame 32.2 -> 30.3 ms
 * FMAD, 37.2 -> 35.9 strict, same bytes: profiles/r06_vac_inner_ab.txt).  A lane that escapes does not leave by itself -- a
 * divergent exit would make the step counter a per-lane value: the WAVE leaves (1), the escaped lanes end their march at the
 * caller, the others come back in.  The escape test's dot product sits behind a wave-uniform `some lane is beyond r = 250`
 * (evaluated on every step it cost the 4K frame 0.4 ms).
 * In: the loop-top radius (r2, r, y, hy) of p, accepted and >= kVacuumR in every live lane.  Returns why the wave left:
 * 1 = a lane escaped (`escaped`; k counts its last step), 2 = out of steps, 3 = some lane needs the generic step: (r2, r, y,
 * hy, rejected, rej_mask) are then the loop-top values of the new p.
 * RRT_VAC_INNER: how many times the body is written out, 1 or 2. */
#ifndef RRT_VAC_INNER
#define RRT_VAC_INNER 2
#endif
static_assert(RRT_VAC_INNER == 1 || RRT_VAC_INNER == 2, "vacuum_run writes its body out once or twice");
template <bool SPIN, bool FMA>
__device__ __forceinline__ int vacuum_run(v3& p, v3& vel, float drag_c, int& k, int max_steps, float& r2, float& r, float& y, float& hy,
                                          float& ys, float& hs, float& hcp, bool& rejected, unsigned long long& rej_mask, bool& escaped) {
#define RRT_VAC_STEP                                                                                                  \
    {                                                                                                                 \
        const v3 q = p;                                                                                               \
        integrate_rk4_lean<SPIN, true, FMA>(p, vel, 0.f, 0.f, 0.f, drag_c, r2, r, y, hy, ys, hs, hcp);                \
        ++k;                                                                                                          \
        escaped = false;                                                                                              \
        if (__builtin_amdgcn_ballot_w64(r > 250.0f) != 0ull) {                        /* raymarcher.cu:120 */         \
            escaped = r > 250.0f && (FMA ? dot_fma(q, vel) : dot(q, vel)) > 0.0f;                                     \
            if (__builtin_amdgcn_ballot_w64(escaped) != 0ull) return 1;                                               \
        }                                                                                                             \
        if (k >= max_steps) return 2;                                                                                 \
        r2 = FMA ? dot_fma(p, p) : dot(p, p);                                                                         \
        rejected = sqrt_seeded_yh<1>(r2, ys, hs, r, y, hy);                                                           \
        rej_mask = __builtin_amdgcn_ballot_w64(rejected);                                                             \
        if ((rej_mask | __builtin_amdgcn_ballot_w64(!(r >= kVacuumR))) != 0ull) return 3;                             \
    }
    for (;;) {
        RRT_VAC_STEP
#if RRT_VAC_INNER >= 2
        RRT_VAC_STEP
#endif
    }
#undef RRT_VAC_STEP
}

/* FAST: march_inline_fast.  Otherwise the lean loop (rrt_device.h: integrate_rk4_lean; FMAD: with fused multiply-adds): the
 * loop-top radius from the seed pair the previous step handed on, the vacuum steps in vacuum_run, every other step generic.
 * UK: every lane of the wave enters at the same step `i` (the single kernel: 0), so the step counter is one number per wave;
 * the loop says so once per outer iteration (v_readfirstlane), which keeps the counter and the vacuum loop's exit code in
 * scalar registers whatever the compiler makes of the merged exits of the outer loop. */
template <bool SPIN, int MEDIA, int ARITH, bool UK = false>
__device__ __forceinline__ void march_inline(const FrameArgs& a, v3& p, v3& vel, Radiance& acc, bool& hit, int& i,
                                             unsigned* oob) {
    constexpr bool FMA = ARITH == kArithFmad;
    if constexpr (ARITH == kArithFast) {
        march_inline_fast<SPIN, MEDIA>(a, p, vel, acc, hit, i, oob);
    } else {
        int steps = i > a.max_steps ? i : a.max_steps;  /* if the loop runs out */
        float ys = 0.0f, hs = 0.0f;                     /* (1/r, 1/(2r)) estimate for the next loop-top radius; 0: none yet */
        float hcp = 0.0f;                               /* 1/(2r) at the previous vacuum step's stage 3 (seed extrapolation) */
        int k = i;
        while (k < a.max_steps) {
            if (UK) k = __builtin_amdgcn_readfirstlane(k);
            v3 rel_p = p;                               /* p - MASS_POS, MASS_POS = 0 */
            float r2 = FMA ? dot_fma(rel_p, rel_p) : dot(rel_p, rel_p);
            float r, y, hy;
            bool rejected = sqrt_seeded_yh<1>(r2, ys, hs, r, y, hy);
            /* wave-uniform: every live lane holds an accepted radius >= kVacuumR (two compares, scalar logic) */
            unsigned long long rej_mask = __builtin_amdgcn_ballot_w64(rejected);
            if ((rej_mask | __builtin_amdgcn_ballot_w64(!(r >= kVacuumR))) == 0ull) {
                bool escaped;
                const int why = vacuum_run<SPIN, FMA>(p, vel, a.drag_c, k, a.max_steps, r2, r, y, hy, ys, hs, hcp, rejected, rej_mask, escaped);
                if (escaped) { steps = k; break; }      /* k counts the step just taken */
                if (why != 3) continue;
                rel_p = p;
            }
            if (rej_mask != 0ull) {
                bool small;                             /* r < 1 ends the ray at the horizon test below */
                if (rejected) radius_fallback(r2, r, y, hy, small);
            }
            if (r < kEventHorizon * 1.01f) { hit = true; acc.t = 0.0f; steps = k; break; }
            const bool near_bh = r < 18.0f;
            const bool in_disk = fabsf(rel_p.y) < kDiskH * 5.0f && r < kDiskOut + 5.0f;
            const bool in_cloud = fabsf(rel_p.y) < kCloudH * 1.5f && r < kCloudOut;
            float h, hh, h6;
            zone_step(near_bh, in_disk, h, hh, h6);
            integrate_rk4_lean<SPIN, false, FMA>(p, vel, h, hh, h6, a.drag_c, r2, r, y, hy, ys, hs, hcp);
            if (MEDIA != 0 && (in_disk || in_cloud)) {
                float d_disk, d_cloud;
                media_densities<MEDIA>(rel_p, a.time, in_disk, in_cloud, a.lut_acc, a.lut_dust, a.dust_bands, oob, d_disk, d_cloud);
                accumulate_sample(acc, d_disk, d_cloud, rel_p, r, vel, h, a.spin);
            }
            ++k;
            if (r > 250.0f && (FMA ? dot_fma(rel_p, vel) : dot(rel_p, vel)) > 0.0f) { steps = k; break; }     /* raymarcher.cu:120 */
        }
        i = steps;
    }
}

/* Workgroup geometry of the per-ray kernels.  A wavefront covers a compact kTileW x kTileH pixel tile (8x8
 * unless RRT_TILE_W says otherwise), so its 64 rays stay spatially coherent: similar step counts, similar
 * zone entry, and sample points that share lattice cells of the low noise octaves (which is what makes the
 * noise tables pay).  RRT_WG_WAVES = 1: one wavefront per workgroup (a CU slot is released as soon as that wave
 * is done -- no waiting for three siblings); 4: a 2x2 block of wave tiles per 256-thread workgroup. */
#ifndef RRT_WG_WAVES
#define RRT_WG_WAVES 1
#endif
#ifndef RRT_TILE_W
#define RRT_TILE_W 8
#endif
constexpr int kWGWaves = RRT_WG_WAVES;
constexpr int kWGThreads = 64 * kWGWaves;
constexpr int kTileW = RRT_TILE_W, kTileH = 64 / kTileW;
static_assert(kTileW * kTileH == 64 && (kTileW & (kTileW - 1)) == 0, "a wave tile is 64 pixels, power-of-two wide");
constexpr int kWGPixX = kWGWaves == 4 ? 2 * kTileW : kTileW, kWGPixY = kWGWaves == 4 ? 2 * kTileH : kTileH;
constexpr int kMaxGridY = 65535;               /* HIP's limit for gridDim.y: a launch covers at most kMaxGridY * kWGPixY rows */

/* Workgroups are dispatched in blockIdx order; the rows through the middle of the frame hold the
 * longest rays (shadow edge, disk), so row-blocks are visited from the middle outwards: mid, mid+1,
 * mid-1, ...  Longest-first shortens the tail of a launch; it changes no pixel. */
__device__ __forceinline__ int dispatch_row(const FrameArgs& a) { return a.grid_row_base + (int)blockIdx.y * a.grid_row_stride; }
__device__ __forceinline__ int row_block(const FrameArgs& a) {
    const int nb = a.grid_rows ? a.grid_rows : (int)gridDim.y, j = dispatch_row(a), mid = (nb - 1) >> 1;
    return (j & 1) ? mid + ((j + 1) >> 1) : mid - (j >> 1);
}
/* Workgroups go to the 8 XCDs round-robin in linear-id order (statically: ids = k mod 8 all run on one XCD), and
 * each XCD has its own L2.  RRT_XCD_RUN = L > 0 deals the tile columns of a grid row out so that the workgroups
 * sharing an XCD cover runs of L adjacent columns (a bijection inside every group of 8 L workgroups; it changes which
 * workgroup renders a tile, no pixel).  Measured (profiles/r02_xcd_columns_ab.txt): one contiguous run per XCD -- the
 * usual GEMM recipe -- is 1.5-2x SLOWER here, because an XCD then owns a vertical stripe of the image and the
 * stripes through the hole and the disk cost several times the outer ones: the round-robin interleave is what
 * balances this kernel.  Default 0 = identity. */
#ifndef RRT_XCD_RUN
#define RRT_XCD_RUN 0
#endif
__device__ __forceinline__ int tile_column(const FrameArgs& a) {
    const int bx = blockIdx.x;
    if (RRT_XCD_RUN <= 0) return bx;
    constexpr int L = RRT_XCD_RUN > 0 ? RRT_XCD_RUN : 1, G = 8 * L;
    const int base = (bx / G) * G;
    if (base + G > (int)gridDim.x) return bx;                 /* the ragged last group keeps its place */
    const unsigned id = (unsigned)dispatch_row(a) * gridDim.x + bx;          /* dispatch order: id % 8 labels the XCD */
    return base + (int)(id & 7u) * L + (((bx - base) >> 3) % L);
}
/* A wave tile's cost is its lifetime in shader clocks / 16, clamped to 22 bits (a wave that lives 30 ms); the order only
 * needs bits 6..21 of it (0.5 us steps), which is what the radix sort looks at: two 8-bit passes. */
constexpr unsigned kTileCostMax = (1u << 22) - 1u;
constexpr int kTileCostSortLo = 6, kTileCostSortHi = 22;
static_assert(kTileCostSortHi - kTileCostSortLo == 16 && (kTileCostMax >> kTileCostSortHi) == 0u, "rrt_tile_sort.h sorts 16 key bits in two passes");

/* the wave tile (row_block * gridDim.x + column) this workgroup renders: the static order above, or the launch's
 * cost-ordered permutation */
__device__ __forceinline__ unsigned wave_tile(const FrameArgs& a) {
    if (a.tile_perm) return a.tile_perm[(unsigned)dispatch_row(a) * gridDim.x + blockIdx.x];
    return (unsigned)(row_block(a) * (int)gridDim.x + tile_column(a));
}
__device__ __forceinline__ bool lane_pixel(const FrameArgs& a, int& x, int& y, int& out_row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int col, rb;
    if (a.tile_perm) { const unsigned t = wave_tile(a); rb = (int)(t / gridDim.x); col = (int)(t - (unsigned)rb * gridDim.x); }
    else { col = tile_column(a); rb = row_block(a); }
    x = col * kWGPixX + (wave & 1) * kTileW + (lane & (kTileW - 1));
    const int lr = rb * kWGPixY + (wave >> 1) * kTileH + lane / kTileW;
    return x < a.width && map_row(a.rows, a.height, lr, y, out_row);
}
/* max over the live lanes of a wave; lanes that are not executing contribute 0 */
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned other = (unsigned)__shfl_xor((int)v, o);
        v = other > v ? other : v;
    }
    return v;
}
/* where a wavefront keeps its bookkeeping in the three-pass workspace: by the wave TILE it renders, so that the three passes
 * (and the rounds) find the same slot whatever order they are dispatched in */
__device__ __forceinline__ unsigned wave_slot(const FrameArgs& a) {
    return wave_tile(a) * (unsigned)kWGWaves + (threadIdx.x >> 6);
}
/* add this wave's lifetime (clocks / 16) to its tile's cost (every lane stores the same word) */
__device__ __forceinline__ void add_tile_cost(const FrameArgs& a, unsigned long long t_start) {
#ifdef RRT_WAVE_TIMELINE     /* dev probe (tools/wave_timeline.py): when the wave started and ended, in microseconds mod 65536, instead of its cost */
    if (RRT_WAVE_TIMELINE == 1) {
        a.tile_cost[wave_tile(a)] = (unsigned)((t_start / 100ull) & 0xffffull) | ((unsigned)((__builtin_amdgcn_s_memrealtime() / 100ull) & 0xffffull) << 16);
        return;
    }
#endif
    const unsigned long long dt = (__builtin_readcyclecounter() - t_start) >> 4;
    const unsigned t = wave_tile(a);
    const unsigned long long sum = (unsigned long long)a.tile_cost[t] + dt;
    a.tile_cost[t] = sum > kTileCostMax ? kTileCostMax : (unsigned)sum;
}

/* Single-kernel path: one ray per lane, media sampled in line (reference raymarch_kernel,
 * src/raymarcher.cu:15-174). */
/* Register budgets.  The bare march takes what the ILP-first scheduler wants (73 VGPRs = 7 waves per SIMD; it keeps its
 * rate down to 4: profiles/r03_march_occupancy_probe.txt).  The kernels that carry the media code are held to 96 = 5 waves:
 * the table-served media code loses 3.6 % at 4 waves and gains 0.7 % at 6 (80 VGPRs: no spill under the default scheduler
 * since the rrt_math.h rewrite, eight spills under max-ilp, which is worth more: r03_media_waves_ab.txt, r03_sched_strategy_ab.txt). */
#ifndef RRT_MEDIA_WAVES
#define RRT_MEDIA_WAVES 5
#endif
template <bool SPIN, int MEDIA, bool DEBUG, int ARITH>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 && !DEBUG ? RRT_MEDIA_WAVES : 1))      /* 2nd: minimum waves per SIMD */
void raymarch_pixels(const FrameArgs a) {
    const unsigned long long t_start = a.tile_cost ? __builtin_readcyclecounter() : 0ull;
    int x, y, out_row;
    if (!lane_pixel(a, x, y, out_row)) return;
    float uvx, uvy;
    v3 p, vel;
    primary_ray(a, x, y, uvx, uvy, p, vel);
    Radiance acc = {0.f, 0.f, 0.f, 1.0f};
    bool hit = false;
    int i = 0;
    march_inline<SPIN, MEDIA, ARITH, true>(a, p, vel, acc, hit, i, DEBUG ? a.dbg.d_lut_oob : nullptr);
    shade_and_store<DEBUG>(a, x, y, out_row, uvx, uvy, hit, p, vel, acc, i);
    if (a.tile_cost) {          /* what this wave cost, for the next launch's order (every lane stores the same word) */
        const unsigned long long dt = (__builtin_readcyclecounter() - t_start) >> 4;
        a.tile_cost[wave_tile(a)] = dt > kTileCostMax ? kTileCostMax : (unsigned)dt;
    }
}

/* s x s supersampled frame (rrt_launch_raymarch_ss, include/rrt.h has the contract): sub-sample (i, j) of output pixel (x, y) is
 * pixel (s x + i, s y + j) of the (s w) x (s h) frame, and the pixel is the mean of its s^2 post-FX HDR values, tone-mapped once.
 * `a` describes that VIRTUAL frame (a.width = s w, a.height = s h: primary_ray, the nudge hash and the vignette see its pixel
 * coordinates) except for a.rows, which maps OUTPUT rows of the w x h frame.  A wave covers an 8x8 tile of the virtual sample
 * grid -- (8/s)^2 output pixels, a pixel's sub-samples in lanes of the same wave -- so the waves are exactly those of
 * raymarch_pixels on the big frame (same coherence, same wave-uniform vacuum loop).  Virtual local row lr' is output local row
 * lr' / s, sub-row lr' mod s: a pixel's lanes are all valid or all invalid.  Sub-sample (i, j) sits in lane
 * (8 j' + i') with i = i' mod s, j = j' mod s, so an xor butterfly over lane masks 1 .. s/2, then 8 .. 8 s/2 sums a pixel's row
 * pairwise in natural order and then its row sums the same way; the sum lands in every lane of the pixel (addition commutes
 * exactly) and its first lane, which holds the low operand at every level, tone-maps and stores.  hdr_out (may be NULL): the
 * mean HDR, alpha 1, indexed like the frame. */
/* The sum of an output pixel's s x s sub-samples (lane mapping: supersample_pixels), in every lane of the pixel. */
__device__ __forceinline__ void pixel_sum(v3& c, const int s) {
    for (int m = 1; m < s; m <<= 1) {                   /* the sub-row: ((s0 + s1) + (s2 + s3)) ... */
        c.x = c.x + __shfl_xor(c.x, m); c.y = c.y + __shfl_xor(c.y, m); c.z = c.z + __shfl_xor(c.z, m);
    }
    for (int m = kTileW; m < s * kTileW; m <<= 1) {     /* ... then the row sums */
        c.x = c.x + __shfl_xor(c.x, m); c.y = c.y + __shfl_xor(c.y, m); c.z = c.z + __shfl_xor(c.z, m);
    }
}

static_assert(kTileW == 8 && kTileH == 8, "supersample_pixels maps a pixel's sub-samples into an 8x8 wave tile (s = 8: one pixel per wave)");
/* A lane of a sampled launch (the mapping above): its sub-sample's virtual pixel (vx, vy) and virtual local row vlr, its output
 * pixel's column x and local output row out_row */
struct SampleLane {
    int vx, vy, vlr, x, out_row;
    __device__ bool stores(int s) const { return ((vx | vlr) & (s - 1)) == 0; }   /* the pixel's first lane stores */
};
/* false: the lane is outside the frame (all of a pixel's lanes are) */
__device__ __forceinline__ bool sample_lane(const FrameArgs& a, const int s, SampleLane& l) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    l.vx = tile_column(a) * kWGPixX + (wave & 1) * kTileW + (lane & (kTileW - 1));
    l.vlr = row_block(a) * kWGPixY + (wave >> 1) * kTileH + lane / kTileW;
    const int w = a.width / s, h = a.height / s;
    l.x = l.vx / s;
    int y;
    if (l.x >= w || !map_row(a.rows, h, l.vlr / s, y, l.out_row)) return false;
    l.vy = s * y + (l.vlr - (l.vlr / s) * s);
    return true;
}
/* A sampled pixel's epilogue: the mean of its sum c (inv = 1 / (number of samples), a power of two: the mean is exact given the
 * sum), tone-mapped and stored at oi; hdr_out (may be NULL): the mean HDR, alpha 1, indexed like the frame. */
__device__ __forceinline__ void store_mean(v3 c, float inv, uchar4* out, float4* hdr_out, size_t oi) {
    c = mk(c.x * inv, c.y * inv, c.z * inv);
    float out_r, out_g, out_b;
    tone_map(c, out_r, out_g, out_b);
    store_rgba8(out, oi, out_r, out_g, out_b);
    if (hdr_out) hdr_out[oi] = make_float4(c.x, c.y, c.z, 1.0f);
}

/* supersample_pixels (kRayPinhole), panorama_pixels (kRayProjection) and stereo_pixels (kRayStereo): the same waves, march,
 * shading and butterfly; only the primary ray differs */
#include "rrt_projection.h"
enum SampledRay { kRayPinhole, kRayProjection, kRayStereo };
template <bool SPIN, int MEDIA, int ARITH, SampledRay RAY>
__device__ __forceinline__ void sampled_pixels(const FrameArgs& a, const int s, float4* const hdr_out, const ProjArgs& pj,
                                               const StereoArgs& sa) {
    SampleLane l;
    if (!sample_lane(a, s, l)) return;
    const auto march_shade = [&](v3 p, v3 vel, float uvx, float uvy) {
        Radiance acc = {0.f, 0.f, 0.f, 1.0f};
        bool hit = false;
        int i = 0;
        march_inline<SPIN, MEDIA, ARITH, true>(a, p, vel, acc, hit, i, nullptr);
        return shade_hdr(a, uvx, uvy, hit, vel, acc);
    };
    v3 c = mk(0.f, 0.f, 0.f);
    if constexpr (RAY == kRayStereo) {
        /* the lane's eye from its composite virtual pixel, then the eye-local pixel every pixel-dependent term sees */
        const bool right = l.vx >= sa.right_x && l.vy >= sa.right_y;
        const int x = right ? l.vx - sa.right_x : l.vx, y = right ? l.vy - sa.right_y : l.vy;
        float o[3], d[3], uvx, uvy;
        stereo_ray(pj, sa, right ? RRT_EYE_RIGHT : RRT_EYE_LEFT, x, y, a.cam, a.use_lens, a.distortion_amount, o, d, uvx, uvy);
        v3 vel = mk(d[0], d[1], d[2]);
        if (__builtin_expect(a.nudge_ulps != 0, 0)) {         /* as primary_ray, on the eye-local virtual pixel */
            vel.x = nudge_component(vel.x, a.nudge_ulps, a.nudge_seed, x, y, 0u);
            vel.y = nudge_component(vel.y, a.nudge_ulps, a.nudge_seed, x, y, 1u);
            vel.z = nudge_component(vel.z, a.nudge_ulps, a.nudge_seed, x, y, 2u);
        }
        c = march_shade(mk(o[0], o[1], o[2]), vel, uvx, uvy);
    } else if constexpr (RAY == kRayProjection) {
        float d[3];
        if (projection_dir(pj, a.width, a.height, l.vx, l.vy, a.cam, d)) {     /* outside the disc: HDR exactly 0, no march */
            v3 vel = mk(d[0], d[1], d[2]);
            if (__builtin_expect(a.nudge_ulps != 0, 0)) {     /* as primary_ray, on the virtual pixel */
                vel.x = nudge_component(vel.x, a.nudge_ulps, a.nudge_seed, l.vx, l.vy, 0u);
                vel.y = nudge_component(vel.y, a.nudge_ulps, a.nudge_seed, l.vx, l.vy, 1u);
                vel.z = nudge_component(vel.z, a.nudge_ulps, a.nudge_seed, l.vx, l.vy, 2u);
            }
            c = march_shade(mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]), vel, 0.f, 0.f);
        }
    } else {
        float uvx, uvy;
        v3 p, vel;
        primary_ray(a, l.vx, l.vy, uvx, uvy, p, vel);
        c = march_shade(p, vel, uvx, uvy);
    }
    pixel_sum(c, s);
    if (!l.stores(s)) return;
    store_mean(c, 1.0f / (float)(s * s), a.out, hdr_out, (size_t)l.out_row * (a.width / s) + l.x);
}

template <bool SPIN, int MEDIA, int ARITH>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 ? RRT_MEDIA_WAVES : 1))      /* raymarch_pixels' register budget */
void supersample_pixels(const FrameArgs a, const int s, float4* const hdr_out) {
    sampled_pixels<SPIN, MEDIA, ARITH, kRayPinhole>(a, s, hdr_out, ProjArgs{}, StereoArgs{});
}

/* Panorama (rrt_launch_raymarch_pano, include/rrt.h has the contract): supersample_pixels with the projection's primary ray
 * (rrt_projection.h: projection_dir, the source the host query runs too) instead of primary_ray -- the same waves over the virtual
 * grid, march, shading and pixel_sum butterfly.  The host clears use_lens and use_vignette (both are defined on the pinhole's uv).
 * A fisheye sub-sample outside the disc stays in its lanes -- pixel_sum shuffles across all of a pixel's lanes -- but branches
 * around the march and the shading with HDR exactly 0: its lane is masked off, so it adds no trips to the wave's vacuum loop and
 * takes no part in its ballots. */
template <bool SPIN, int MEDIA, int ARITH>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 ? RRT_MEDIA_WAVES : 1))      /* raymarch_pixels' register budget */
void panorama_pixels(const FrameArgs a, const int s, float4* const hdr_out, const ProjArgs pj) {
    sampled_pixels<SPIN, MEDIA, ARITH, kRayProjection>(a, s, hdr_out, pj, StereoArgs{});
}

/* Stereo (rrt_launch_raymarch_stereo, include/rrt.h has the contract): supersample_pixels over the COMPOSITE virtual frame (a.width
 * x a.height: both eyes; a.rows maps the composite's output rows), each lane's ray from stereo_ray (rrt_projection.h, the source
 * the host query runs too) on its eye-local pixel.  A pixel's s x s sub-samples lie in one eye (the eye boundary is a whole output
 * pixel), so the butterfly is unchanged.  The eye is uniform across a wave when the boundary (s*height rows, or s*width columns)
 * is a multiple of 8 virtual pixels; otherwise the wave that straddles it is split per lane -- coherence, not correctness.  For
 * equirect the host clears use_lens and use_vignette, as for panorama_pixels. */
template <bool SPIN, int MEDIA, int ARITH>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 ? RRT_MEDIA_WAVES : 1))      /* raymarch_pixels' register budget */
void stereo_pixels(const FrameArgs a, const int s, float4* const hdr_out, const ProjArgs pj, const StereoArgs sa) {
    sampled_pixels<SPIN, MEDIA, ARITH, kRayStereo>(a, s, hdr_out, pj, sa);
}

/* Adaptive supersampling (rrt_launch_raymarch_adaptive, include/rrt.h has the contract): the refine pass.  adaptive_mask
 * (rrt_adaptive.h) has left the frame indices of the pixels to refine in a list; this kernel renders exactly those pixels as
 * supersample_pixels / panorama_pixels would and overwrites them in the base frame.  `a` describes the VIRTUAL (s w) x (s h) frame,
 * as theirs.  A wave is an 8x8 tile of virtual samples made of (8/s)^2 pixel SLOTS: slot (sa, sb) of wave k takes list entry
 * k (8/s)^2 + sb (8/s) + sa, and lane (i', j') is sub-sample (i' mod s, j' mod s) of slot (i'/s, j'/s) -- the lane layout pixel_sum
 * assumes, so the sum's order is supersample_pixels' and the pixel's first lane stores.  A ray's result does not depend on which
 * rays share its wavefront (tests/test_gpu_march_waves.py), which is what lets scattered pixels fill a wave.
 * The host does not know the count: it launches for width*height entries, and a slot past the device-side count leaves before
 * the march -- all of its lanes together, and whole waves on one scalar load.  The ray selection is a private copy of
 * sampled_pixels' (factoring it out of there would move the existing kernels' registers). */
#include "rrt_adaptive.h"
template <bool SPIN, int MEDIA, int ARITH, SampledRay RAY>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 ? RRT_MEDIA_WAVES : 1))      /* raymarch_pixels' register budget */
void refine_pixels(const FrameArgs a, const RefineArgs ra, const ProjArgs pj) {
    static_assert(RAY == kRayPinhole || RAY == kRayProjection, "no adaptive stereo");
    const int s = ra.s, lane = threadIdx.x & 63, li = lane & (kTileW - 1), lj = lane / kTileW;
    const int shift = __ffs(s) - 1, per = kTileW >> shift;          /* s is a power of two: slots per axis */
    const unsigned wave = (blockIdx.y * gridDim.x + blockIdx.x) * (unsigned)kWGWaves + (threadIdx.x >> 6);
    const unsigned slot = wave * (unsigned)(per * per) + (unsigned)((lj >> shift) * per + (li >> shift));
    if (slot >= *ra.count) return;
    const unsigned idx = ra.list[slot];                             /* stored row * width + x of the w x h frame */
    const int w = a.width >> shift, h = a.height >> shift;
    const int out_row = (int)(idx / (unsigned)w), x = (int)(idx - (unsigned)out_row * (unsigned)w);
    const int vx = s * x + (li & (s - 1)), vy = s * (h - 1 - out_row) + (lj & (s - 1));       /* rows are stored bottom-up */
    const auto march_shade = [&](v3 p, v3 vel, float uvx, float uvy) {
        Radiance acc = {0.f, 0.f, 0.f, 1.0f};
        bool hit = false;
        int i = 0;
        march_inline<SPIN, MEDIA, ARITH, true>(a, p, vel, acc, hit, i, nullptr);
        return shade_hdr(a, uvx, uvy, hit, vel, acc);
    };
    v3 c = mk(0.f, 0.f, 0.f);
    if constexpr (RAY == kRayProjection) {
        float d[3];
        if (projection_dir(pj, a.width, a.height, vx, vy, a.cam, d)) {         /* outside the disc: HDR exactly 0, no march */
            v3 vel = mk(d[0], d[1], d[2]);
            if (__builtin_expect(a.nudge_ulps != 0, 0)) {         /* as primary_ray, on the virtual pixel */
                vel.x = nudge_component(vel.x, a.nudge_ulps, a.nudge_seed, vx, vy, 0u);
                vel.y = nudge_component(vel.y, a.nudge_ulps, a.nudge_seed, vx, vy, 1u);
                vel.z = nudge_component(vel.z, a.nudge_ulps, a.nudge_seed, vx, vy, 2u);
            }
            c = march_shade(mk(a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]), vel, 0.f, 0.f);
        }
    } else {
        float uvx, uvy;
        v3 p, vel;
        primary_ray(a, vx, vy, uvx, uvy, p, vel);
        c = march_shade(p, vel, uvx, uvy);
    }
    pixel_sum(c, s);
    if (((li | lj) & (s - 1)) != 0) return;
    store_mean(c, 1.0f / (float)(s * s), a.out, ra.hdr_out, (size_t)idx);
}

/* Motion-blurred frame (rrt_launch_raymarch_mb, include/rrt.h has the contract): sub-frame k is supersample_pixels' frame at
 * (m.time[k], m.cam[k]), and the pixel is the mean of the K sub-frames' sums, tone-mapped once.  The waves are supersample_pixels'
 * (an 8x8 tile of the virtual sample grid); a wave-uniform loop over k runs the march once per sub-frame in the same lanes -- a
 * pixel's K rays are nearly coherent -- forms T_k with the same butterfly and folds it into the temporal tree.  Time and camera are
 * read from the by-value MotionArgs at the uniform k, so they stay scalar and the march is raymarch_pixels' code.
 * Registers: the media kernels use every scalar register across the march, so nothing else may stay live across it.  The tree's
 * partials (level l: the sum of the 2^l sub-frames before k) and the lane's pixel coordinates live in per-lane LDS slots (<= 4
 * levels x 3 floats + 3 ints, x 64 lanes = 3.75 KB per one-wave workgroup), and the launch's scalars are read afresh where they are
 * used (motion_arg) -- hoisted out of the loop, they would hold registers across the march and spill.  Every lane of a pixel folds
 * the same bits (the butterfly leaves the sum in all of them); its first lane stores. */
constexpr int kMaxTimes = 16;
struct MotionArgs { float time[kMaxTimes]; rrt_camera cam[kMaxTimes]; };
struct MotionLaunch {                                   /* motion_pixels' one kernel argument */
    FrameArgs a;                                        /* the virtual frame, as supersample_pixels' */
    MotionArgs m;
    int s, n;                                           /* n: the number of sub-frames */
    float4* hdr_out;
};

/* A field of the kernel argument read where it is used: the load cannot be hoisted out of the loop over the sub-frames. */
template <class T>
__device__ __forceinline__ T motion_arg(size_t offset) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) char* KP;
    KP base = (KP)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(base));
    return *(const __attribute__((address_space(4))) T*)(base + offset);
#else
    return T();
#endif
}
/* in a kernel whose one argument is the struct it names `Launch` */
#define RRT_SUB_ARG(field) motion_arg<decltype(((Launch*)nullptr)->field)>(offsetof(Launch, field))

static_assert(kWGWaves == 1, "motion_pixels' LDS slots are sized for one-wave workgroups");
template <bool SPIN, int MEDIA, int ARITH>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 ? RRT_MEDIA_WAVES : 1))      /* raymarch_pixels' register budget */
void motion_pixels(const MotionLaunch L) {
    using Launch = MotionLaunch;
    __shared__ float part[4][3][kWGThreads];            /* levels 0..3: n <= 16 never stores level 4 */
    __shared__ volatile int where[3][kWGThreads];       /* vx, vy, the output index (-1: another lane of the pixel stores) */
    const int t = threadIdx.x;
    {
        const int s = L.s;
        SampleLane l;
        if (!sample_lane(L.a, s, l)) return;
        where[0][t] = l.vx;
        where[1][t] = l.vy;
        where[2][t] = l.stores(s) ? l.out_row * (L.a.width / s) + l.x : -1;
    }
    v3 c;
    for (int k = 0; k < L.n; ++k) {
        FrameArgs b = L.a;
        b.time = L.m.time[k];
        b.cam = L.m.cam[k];
        b.width = RRT_SUB_ARG(a.width); b.height = RRT_SUB_ARG(a.height);               /* what primary_ray reads */
        b.use_lens = RRT_SUB_ARG(a.use_lens); b.distortion_amount = RRT_SUB_ARG(a.distortion_amount);
        b.nudge_ulps = RRT_SUB_ARG(a.nudge_ulps); b.nudge_seed = RRT_SUB_ARG(a.nudge_seed);
        float uvx, uvy;
        v3 p, vel;
        primary_ray(b, where[0][t], where[1][t], uvx, uvy, p, vel);
        Radiance acc = {0.f, 0.f, 0.f, 1.0f};
        bool hit = false;
        int i = 0;
        march_inline<SPIN, MEDIA, ARITH, true>(b, p, vel, acc, hit, i, nullptr);
        b.sky = RRT_SUB_ARG(a.sky);                                                      /* what shade_hdr reads */
        b.use_bloom = RRT_SUB_ARG(a.use_bloom); b.bloom_threshold = RRT_SUB_ARG(a.bloom_threshold);
        b.bloom_intensity = RRT_SUB_ARG(a.bloom_intensity); b.use_vignette = RRT_SUB_ARG(a.use_vignette);
        b.vignette_intensity = RRT_SUB_ARG(a.vignette_intensity); b.use_ca = RRT_SUB_ARG(a.use_ca); b.ca_amount = RRT_SUB_ARG(a.ca_amount);
        c = shade_hdr(b, uvx, uvy, hit, vel, acc);
        pixel_sum(c, L.s);
        int l = 0;                                      /* ((T0 + T1) + (T2 + T3)) ...: close the levels sub-frame k completes */
        for (int j = k; j & 1; j >>= 1, ++l)
            c = add(mk(part[l][0][t], part[l][1][t], part[l][2][t]), c);
        if (k + 1 < L.n) { part[l][0][t] = c.x; part[l][1][t] = c.y; part[l][2][t] = c.z; }
    }
    const int oi = where[2][t];
    if (oi < 0) return;
    const int s = RRT_SUB_ARG(s);
    store_mean(c, 1.0f / (float)(s * s * RRT_SUB_ARG(n)), RRT_SUB_ARG(a.out), RRT_SUB_ARG(hdr_out), (size_t)oi);
}

/* Depth of field (rrt_launch_raymarch_dof, include/rrt.h has the contract): motion_pixels with a lens point per sample.  Sample k
 * is supersample_pixels' frame at (m.time[k], m.cam[k]) whose primary ray is lens_ray's (rrt_projection.h, the source the host
 * query runs too) through the lens point (m.lx[k], m.ly[k]); cx = lx / focus and cy = ly / focus come rounded from the host.  All
 * six are read from the by-value LensArgs at the uniform k, so they stay scalar, and a pixel's K rays share the wave's lanes.  The
 * nudge runs here, after lens_ray, on the virtual pixel (primary_ray's own).  Registers, LDS slots and the re-read kernel
 * arguments are motion_pixels'.  The two kernels stay written out: one forced-inline body behind both keeps every resource figure
 * but moves motion_pixels' register allocation, and its FMAD s = 1 frames measured 1.5-2 % slower (depth of field). */
struct LensArgs { float time[kMaxTimes]; rrt_camera cam[kMaxTimes]; float lx[kMaxTimes], ly[kMaxTimes], cx[kMaxTimes], cy[kMaxTimes]; };
struct LensLaunch {                                     /* lens_pixels' one kernel argument */
    FrameArgs a;                                        /* the virtual frame, as supersample_pixels' */
    LensArgs m;
    int s, n;                                           /* n: the number of lens samples */
    float4* hdr_out;
};

template <bool SPIN, int MEDIA, int ARITH>
__global__ __launch_bounds__(kWGThreads, (MEDIA != 0 ? RRT_MEDIA_WAVES : 1))      /* raymarch_pixels' register budget */
void lens_pixels(const LensLaunch L) {
    using Launch = LensLaunch;
    __shared__ float part[4][3][kWGThreads];            /* levels 0..3: n <= 16 never stores level 4 */
    __shared__ volatile int where[3][kWGThreads];       /* vx, vy, the output index (-1: another lane of the pixel stores) */
    const int t = threadIdx.x;
    {
        const int s = L.s;
        SampleLane l;
        if (!sample_lane(L.a, s, l)) return;
        where[0][t] = l.vx;
        where[1][t] = l.vy;
        where[2][t] = l.stores(s) ? l.out_row * (L.a.width / s) + l.x : -1;
    }
    v3 c;
    for (int k = 0; k < L.n; ++k) {
        FrameArgs b = L.a;
        b.time = L.m.time[k];
        b.cam = L.m.cam[k];
        float uvx, uvy;
        v3 p, vel;
        {
            const int x = where[0][t], y = where[1][t];
            float o[3], d[3];
            lens_ray(RRT_SUB_ARG(a.width), RRT_SUB_ARG(a.height), x, y, b.cam, RRT_SUB_ARG(a.use_lens),
                     RRT_SUB_ARG(a.distortion_amount), L.m.lx[k], L.m.ly[k], L.m.cx[k], L.m.cy[k], o, d, uvx, uvy);
            p = mk(o[0], o[1], o[2]);
            vel = mk(d[0], d[1], d[2]);
            const int nudge_ulps = RRT_SUB_ARG(a.nudge_ulps);
            if (__builtin_expect(nudge_ulps != 0, 0)) {             /* nudge_direction written out: the seed is read only here */
                const unsigned seed = RRT_SUB_ARG(a.nudge_seed);
                vel.x = nudge_component(vel.x, nudge_ulps, seed, x, y, 0u);
                vel.y = nudge_component(vel.y, nudge_ulps, seed, x, y, 1u);
                vel.z = nudge_component(vel.z, nudge_ulps, seed, x, y, 2u);
            }
        }
        Radiance acc = {0.f, 0.f, 0.f, 1.0f};
        bool hit = false;
        int i = 0;
        march_inline<SPIN, MEDIA, ARITH, true>(b, p, vel, acc, hit, i, nullptr);
        b.sky = RRT_SUB_ARG(a.sky);                                                      /* what shade_hdr reads */
        b.use_bloom = RRT_SUB_ARG(a.use_bloom); b.bloom_threshold = RRT_SUB_ARG(a.bloom_threshold);
        b.bloom_intensity = RRT_SUB_ARG(a.bloom_intensity); b.use_vignette = RRT_SUB_ARG(a.use_vignette);
        b.vignette_intensity = RRT_SUB_ARG(a.vignette_intensity); b.use_ca = RRT_SUB_ARG(a.use_ca); b.ca_amount = RRT_SUB_ARG(a.ca_amount);
        c = shade_hdr(b, uvx, uvy, hit, vel, acc);
        pixel_sum(c, L.s);
        int l = 0;                                      /* ((T0 + T1) + (T2 + T3)) ...: close the levels sample k completes */
        for (int j = k; j & 1; j >>= 1, ++l)
            c = add(mk(part[l][0][t], part[l][1][t], part[l][2][t]), c);
        if (k + 1 < L.n) { part[l][0][t] = c.x; part[l][1][t] = c.y; part[l][2][t] = c.z; }
    }
    const int oi = where[2][t];
    if (oi < 0) return;
    const int s = RRT_SUB_ARG(s);
    store_mean(c, 1.0f / (float)(s * s * RRT_SUB_ARG(n)), RRT_SUB_ARG(a.out), RRT_SUB_ARG(hdr_out), (size_t)oi);
}

/* rrt_launch_projection_map: projection_dir of every pixel, (dir, inside) in the frame's bottom-up layout */
__global__ __launch_bounds__(256) void projection_map(float4* out, int W, int H, const rrt_camera cam, const ProjArgs pj) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)W * H) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    float d[3];
    const bool inside = projection_dir(pj, W, H, x, y, cam, d);
    out[(size_t)(H - 1 - y) * W + x] = make_float4(d[0], d[1], d[2], inside ? 1.0f : 0.0f);
}

/* ---- three-pass path, pass 1: geodesics only; sample points of in-medium steps go to the pool ---- */
/* amdgpu_num_sgpr(80): gfx950 admits 8 waves per SIMD only up to 80 SGPRs (7 for 82-96); this loop needs
 * the occupancy (measured: 4 waves/SIMD is 15 % slower than 8).
 * RESUME (rounds after the first): only wavefronts the pool ran out under (state 2) do anything -- their suspended rays
 * carry on from the saved pre-step state; rays of the same wave that had already ended stay as they are. */
#ifndef RRT_DEFER_WAVES
#define RRT_DEFER_WAVES 8
#endif
#if RRT_DEFER_WAVES >= 8
#define RRT_DEFER_SGPR_ATTR __attribute__((amdgpu_num_sgpr(80)))
#else
#define RRT_DEFER_SGPR_ATTR
#endif
template <bool SPIN, int ARITH, bool RESUME>
__global__ __launch_bounds__(kWGThreads, RRT_DEFER_WAVES) RRT_DEFER_SGPR_ATTR void march_defer(const FrameArgs a) {
    constexpr bool FAST = ARITH == kArithFast, FMA = ARITH == kArithFmad;
    if (RESUME && a.ctr->last_overflow == 0u) return;            /* nothing was suspended: the whole grid leaves at once */
#ifdef RRT_WAVE_TIMELINE
    const unsigned long long t_start = a.tile_cost ? __builtin_amdgcn_s_memrealtime() : 0ull;
#else
    const unsigned long long t_start = a.tile_cost ? __builtin_readcyclecounter() : 0ull;
#endif
    int x = 0, y = 0, out_row = 0;
    const bool valid = lane_pixel(a, x, y, out_row);
    if (!__any(valid)) return;
    /* lanes without a pixel stay alive (all 64 lanes take part in the wave-level bookkeeping below); they march nothing */
    const int lane = threadIdx.x & 63;
    const unsigned wid = wave_slot(a);
    const size_t li = (size_t)wid * 64 + lane;
    v3 p = mk(1000.f, 0.f, 0.f), vel = mk(0.f, 0.f, 0.f);
    bool hit = false;
    bool active = valid;                                          /* this lane marches in this round */
    int i = 0;
    if (RESUME) {
        if (a.hdr[wid].state != 2u) return;                       /* wave-uniform: marched to its end, or shaded already */
        const unsigned code = reinterpret_cast<const unsigned*>(a.finals)[3 * a.n_lanes + li];
        vel = mk(a.finals[li], a.finals[a.n_lanes + li], a.finals[2 * a.n_lanes + li]);
        p = mk(a.finals[4 * a.n_lanes + li], a.finals[5 * a.n_lanes + li], a.finals[6 * a.n_lanes + li]);
        hit = (code >> 31) != 0;
        i = (int)(code & 0x3fffffffu);
        active = valid && (code & 0x40000000u) != 0;
    } else if (valid) {
        float uvx, uvy;
        primary_ray(a, x, y, uvx, uvy, p, vel);
    }

    /* wave-level bookkeeping; identical in every lane that is still marching */
    unsigned first_block = kNoBlock, n_runs = 0;
    unsigned run_start = kNoBlock, run_len = 0, run_blk = 0;      /* current run; block run_start + run_blk in use */
    unsigned used = kBlockRows;                                   /* rows used in the current block */
    bool overflow = false;                                        /* this lane stopped because the pool is full */

    constexpr bool LEAN = !FAST;                               /* the lean step and vacuum_run (march_inline has the notes) */
    float y_seed = 0.0f, h_seed = 0.0f, hc_prev = 0.0f;        /* (LEAN) a resumed ray starts without seeds: its first root takes
                                                                * the v_rsq fall-back, which is the same correctly rounded root */
    /* `i` is a per-lane variable only across rounds: the lanes that march in a round all start at the same step (0, or the
     * step the pool ran out at, which is a wave-uniform event) -- but a first round can PROVE it to the compiler-independent
     * v_readfirstlane below, a resumed one only by that argument, so only the first round keeps the counter scalar */
    constexpr bool UK = !RESUME && LEAN;
    for (; active && i < a.max_steps; ++i) {
        if (UK) i = __builtin_amdgcn_readfirstlane(i);
        v3 rel_p = p;
        float r2, r, yv, hv = 0.0f;
        /* `vacuum` is false wherever it is read below vacuum_run: it and the branches it guards are what is left of the flat
         * loop.  They stay because the compiler's output depends on them (without them every instance of this kernel comes
         * out different, the lean ones ~400 instructions shorter): taking them out is a change to measure, not a clean-up. */
        bool vacuum = false;
        if constexpr (LEAN) {
            r2 = FMA ? dot_fma(rel_p, rel_p) : dot(rel_p, rel_p);
            bool rejected = sqrt_seeded_yh<1>(r2, y_seed, h_seed, r, yv, hv);
            unsigned long long rej_mask = __builtin_amdgcn_ballot_w64(rejected);
            vacuum = (rej_mask | __builtin_amdgcn_ballot_w64(!(r >= kVacuumR))) == 0ull;
            if (vacuum) {                                          /* the vacuum steps in their own loop (vacuum_run) */
                bool escaped;
                const int why = vacuum_run<SPIN, FMA>(p, vel, a.drag_c, i, a.max_steps, r2, r, yv, hv, y_seed, h_seed, hc_prev, rejected,
                                                      rej_mask, escaped);
                if (escaped) break;                                /* i counts the step just taken */
                if (why != 3) { --i; continue; }                   /* (the loop's own ++i) */
                rel_p = p;
                vacuum = false;
            }
            if (!vacuum && rej_mask != 0ull) {
                bool small;
                if (rejected) radius_fallback(r2, r, yv, hv, small);
            }
        } else march_radius<kArithFast>(rel_p, r2, r, yv);
        if (r < kEventHorizon * 1.01f) { hit = true; break; }

        bool in_disk = false, in_cloud = false;
        float h = kHVac, hh = 0.5f * kHVac, h6 = kHVac / 6.0f;
        if (!vacuum) {                                             /* wave-uniform */
            const bool near_bh = r < 18.0f;
            in_disk = fabsf(rel_p.y) < kDiskH * 5.0f && r < kDiskOut + 5.0f;
            in_cloud = fabsf(rel_p.y) < kCloudH * 1.5f && r < kCloudOut;
            zone_step(near_bh, in_disk, h, hh, h6);
        }

        /* Both density functions return 0 unless the cylindrical radius rc = sqrtf(x*x + 0*0 + z*z) is in
         * [ISCO, DISK_OUT] (densities.h:21-22, :70-71), and behind disk_point()'s first exact early-out, y^2 rc > 135; only
         * the other steps need a sample.  Round 5: the test here is a cheap SUPERSET of that gate on rc^2 -- no square root:
         * rc = RN(sqrt(rc2)) in [10, 25] implies rc2 in (99.9999, 625.0002), and RN(RN(y y) rc) <= 135 implies
         * (y y)^2 rc2 <= 135^2 (1 + 2e-6) -- the few samples it admits beyond the exact gate evaluate to the identity in pass 2
         * (disk_point() returns false) and are dropped there, so the bytes cannot depend on it.
         * The row is reserved BEFORE the step is taken: if the pool is full the lane stops here with its
         * pre-step state intact, and the next round (or, after the last one, pass 3 in line) resumes it. */
        unsigned long long need_mask = 0ull;
        bool need = false;
        float* row_f = nullptr;
        if (!vacuum && __any(in_disk || in_cloud)) {
            if (in_disk || in_cloud) {
                const float rc2 = rel_p.x * rel_p.x + 0.0f * 0.0f + rel_p.z * rel_p.z;
                const float yy = rel_p.y * rel_p.y;
                need = rc2 >= 99.99f && rc2 <= 625.01f && (yy * yy) * rc2 <= 18227.0f;          /* 135^2 = 18225 */
            }
            need_mask = __ballot(need);
        }
        if (need_mask != 0ull) {
            const int leader = __ffsll((long long)__ballot(1)) - 1;
            if (used == kBlockRows) {                              /* wave-uniform: next block */
                if (run_start != kNoBlock && run_blk + 1 < run_len) {
                    ++run_blk;                                     /* still inside the current run */
                } else {                                           /* take a new run, twice as long */
                    const unsigned len = run_len == 0 ? 1u : (run_len * 2 > kMaxRun ? kMaxRun : run_len * 2);
                    unsigned start = 0;
                    if (lane == leader) start = atomicAdd(&a.ctr->next_block, len);
                    start = __builtin_amdgcn_readfirstlane(start);
                    if (start + len > a.block_capacity) {
                        /* the pool is full: blocks [start, capacity) now belong to this failed run; give them empty
                         * masks so that pass 2 finds nothing in them */
                        if (lane == leader) {
                            for (unsigned b2 = start; b2 < a.block_capacity; ++b2) {
                                ulonglong2* m = reinterpret_cast<ulonglong2*>(a.sample_blocks + (size_t)b2 * kBlockBytes + kBlockTrailer);
#pragma unroll
                                for (unsigned k = 0; k < kBlockRows / 2; ++k) m[k] = make_ulonglong2(0ull, 0ull);
                            }
                        }
                        overflow = true;
                        break;
                    }
                    if (lane == leader) {                          /* lanes 0-7 may have left the loop already */
                        for (unsigned b2 = 0; b2 < len; ++b2) {
                            ulonglong2* m = reinterpret_cast<ulonglong2*>(a.sample_blocks + (size_t)(start + b2) * kBlockBytes +
                                                                          kBlockTrailer);
#pragma unroll
                            for (unsigned k = 0; k < kBlockRows / 2; ++k) m[k] = make_ulonglong2(0ull, 0ull);
                        }
                        unsigned* link = reinterpret_cast<unsigned*>(a.sample_blocks + (size_t)start * kBlockBytes +
                                                                     kBlockTrailer + kBlockRows * 8);
                        link[0] = kNoBlock; link[1] = 0u;
                        if (run_start != kNoBlock) {
                            unsigned* prev = reinterpret_cast<unsigned*>(a.sample_blocks + (size_t)run_start * kBlockBytes +
                                                                         kBlockTrailer + kBlockRows * 8);
                            prev[0] = start; prev[1] = len;
                        }
                    }
                    if (first_block == kNoBlock) first_block = start;
                    run_start = start; run_len = len; run_blk = 0;
                    ++n_runs;
                }
                used = 0;
            }
            uint8_t* base = a.sample_blocks + (size_t)(run_start + run_blk) * kBlockBytes;
            if (lane == leader) reinterpret_cast<unsigned long long*>(base + kBlockTrailer)[used] = need_mask;
            row_f = reinterpret_cast<float*>(base + used * kRowData) + lane;
            ++used;
        }

        if constexpr (LEAN) {
            if (vacuum) integrate_rk4_lean<SPIN, true, FMA>(p, vel, 0.f, 0.f, 0.f, a.drag_c, r2, r, yv, hv, y_seed, h_seed, hc_prev);
            else integrate_rk4_lean<SPIN, false, FMA>(p, vel, h, hh, h6, a.drag_c, r2, r, yv, hv, y_seed, h_seed, hc_prev);
        } else integrate_rk4_fast<SPIN>(p, vel, h, hh, h6, a.drag_c, r2, yv);

        if (!vacuum && need) {                                                /* pre-step position, post-step velocity */
            row_f[0] = rel_p.x; row_f[64] = rel_p.y; row_f[128] = rel_p.z;
            /* vel.y is not stored (kRowPlanes); a non-finite one travels as a NaN in vel.x (vel.y - vel.y is 0 iff finite) */
            row_f[192] = (vel.y - vel.y == 0.0f) ? vel.x : __builtin_nanf(""); row_f[256] = vel.z;
        }
        if (r > 250.0f && (FMA ? dot_fma(rel_p, vel) : dot(rel_p, vel)) > 0.0f) { ++i; break; }
    }

    /* wave-level epilogue: all 64 lanes are here */
    const bool any_overflow = __any(overflow);
    /* lanes that left the loop early hold stale copies of the bookkeeping: the lane that ran longest has
     * the final run count, and any lane that saw the first allocation has first_block */
    n_runs = wave_max_u32(n_runs);
    first_block = ~wave_max_u32(~first_block);
    /* terminal (or, on overflow, resumable) state of every ray; pass 3 shades all pixels -- keeping the sky
     * and post-FX code with its scalar operands out of this kernel keeps it at 8 waves per SIMD */
    a.finals[li] = vel.x;
    a.finals[a.n_lanes + li] = vel.y;
    a.finals[2 * a.n_lanes + li] = vel.z;
    reinterpret_cast<unsigned*>(a.finals)[3 * a.n_lanes + li] =
        (unsigned)i | (hit ? 0x80000000u : 0u) | (overflow ? 0x40000000u : 0u);
    a.finals[4 * a.n_lanes + li] = p.x;
    a.finals[5 * a.n_lanes + li] = p.y;
    a.finals[6 * a.n_lanes + li] = p.z;
    if (lane == 0) {
        a.hdr[wid].first_block = first_block; a.hdr[wid].n_runs = n_runs; a.hdr[wid].state = any_overflow ? 2u : 1u;
        if (any_overflow) atomicAdd(&a.ctr->overflow_waves, 1u);
    }
    if (a.tile_cost) add_tile_cost(a, t_start);
}

/* zero the workspace's counters and wave headers.  A kernel, not hipMemsetAsync: the memset NODE a captured launch turned
 * into did not reliably clear them on a second replay of the graph (counters came back holding the previous replay's values
 * plus stray words; round 4, tests/test_gpu_frames.py::test_streams_graph_capture_and_borrowed_sky) */
__global__ __launch_bounds__(256) void zero_words(uint4* p, size_t n16) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n16) p[i] = make_uint4(0u, 0u, 0u, 0u);
}

/* between two rounds (one thread): close the round's statistics and empty the pool */
__global__ void pool_next_round(DeferCounters* c, unsigned capacity, int last) {
    const unsigned used = c->next_block < capacity ? c->next_block : capacity;
    if (used > c->peak_blocks) c->peak_blocks = used;
    c->total_blocks += used;
    if (c->rounds_run == 0u || c->last_overflow != 0u) ++c->rounds_with_work;
    ++c->rounds_run;
    c->last_overflow = c->overflow_waves;
    if (last) c->suspended_left = c->overflow_waves;
    c->next_block = 0u; c->overflow_waves = 0u;
}

/* ---- pass 2: densities + emission of every pooled sample row, grid-stride over the pool ---- */
/* Round 5: pass 2 is the one latency-bound kernel with spare registers -- 40 % of its wave-cycles sit in s_waitcnt at 3.8
 * resident waves per SIMD (profiles/r05_pmc_diag_before_nt.txt) -- and its code fits 64 VGPRs with two spilled registers: 8 waves
 * per SIMD (the grid is exactly 8 192 waves) instead of 5 is worth 3 % of a full disk-heavy three-pass frame (key 1 56.9 -> 55.3 ms,
 * from inside the disk 57.5 -> 55.7; 6 and 7 waves: < 1 %; a rank's share, whose pass 2 already runs under the other chain's
 * march, does not move: profiles/r05_eval_waves_ab.txt).  The in-line kernels, which share the code, gain nothing from more
 * waves (round 3) and keep 5. */
#ifndef RRT_EVAL_WAVES
#define RRT_EVAL_WAVES 8
#endif
/* The cursor a replay's pass 2 hands its blocks out from: the counter slot of a second chain, at kCounterStride behind the
 * launch's own counters.  The march cache runs one chain, so the slot is free there, and zero_words clears it at every fill.
 * It is 0 whenever a replay's pass 2 starts: pass 3 of the same launch puts it back.  (Reached from a.ctr and not through a
 * field of KeepArgs: a larger KeepArgs moves the hidden kernel arguments of every instance, KEEP or not, and with them the
 * encodings of kernels this does not concern.) */
__device__ __forceinline__ unsigned* replay_cursor(const FrameArgs& a) {
    return reinterpret_cast<unsigned*>(reinterpret_cast<uint8_t*>(a.ctr) + kCounterStride);
}

/* A replay's row: row k (input mask `mask`, not empty) of retained block b holds sample records; what the row loop of
 * eval_sample_rows below does with such a row -- same loads, same eval_sample_record, same stores, same out-mask rule.  A function
 * of its own, and that loop left as it stands, because folding the two into one text moves registers in the non-KEEP instances
 * (tools/kernel_bytes.py; so did round 10's attempt). */
template <int MEDIA>
__device__ __forceinline__ void replay_row(const FrameArgs& a, const KeepArgs& kp, unsigned b, unsigned k, unsigned long long mask, int lane) {
    const uint8_t* blk = a.sample_blocks + (size_t)b * kBlockBytes;
    uint8_t* const oblk = kp.out_blocks + (size_t)b * kOutBlockBytes;
    const bool mine = (mask >> lane) & 1ull;
    const float* f = reinterpret_cast<const float*>(blk + k * kRowData) + lane;
    const float* e = reinterpret_cast<const float*>(oblk + kOutBlockEnv + k * kOutEnvData) + lane;
    bool has = false;
    float ex = 0.f, ey = 0.f, ez = 0.f, s = 1.0f;
    if (mine) {
        SampleRecord rec;
        rec.rc = f[0]; rec.y = f[64]; rec.azimuth = f[128]; rec.shift_g = f[192]; rec.r = f[256];
        rec.env_acc = e[0]; rec.env_dust = e[64];
        has = eval_sample_record<MEDIA>(rec, a.time, record_step(rec, kHNear, kHDisk, kHVac), a.lut_acc, a.lut_dust, a.dust_bands, ex, ey, ez, s);
    }
    const unsigned long long live = __ballot(has);
    float* g = reinterpret_cast<float*>(oblk + k * kOutRowData) + lane;
    if (has) { g[0] = ex; g[64] = ey; g[128] = ez; g[192] = s; }
    if (lane == (int)(__ffsll((long long)mask) - 1)) reinterpret_cast<unsigned long long*>(oblk + kOutBlockMasks)[k] = live;
}

template <int ARITH, int MEDIA, bool KEEP = false>
__global__ __launch_bounds__(256, RRT_EVAL_WAVES) void eval_sample_rows(const FrameArgs a, const KeepArgs kp) {
    const int lane = threadIdx.x & 63;
    const unsigned n_blk = KEEP && kp.replay ? min(kp.n_blocks, a.block_capacity) : min(a.ctr->next_block, a.block_capacity);
    if constexpr (KEEP) {
        if (kp.replay) {
            /* Round 11: a replay hands its rows out.  A wave takes kReplayChunk whole blocks at a time from one cursor (one lane's
             * atomic, the start broadcast: wave-uniform) until the cursor has passed n_blk, so a workgroup that starts late -- the
             * chip shares its slots with whatever else is resident -- or meets cheap rows takes fewer blocks instead of marching a
             * fixed 1/8192 of the pool alone at the end.  ONE cursor is enough because the cache's launches are chained
             * (MarchCacheObject::chained): no two replays' pass 2 ever run at once, on whatever streams; pass 3 of the same launch
             * puts the cursor back to 0.  A block's eight input masks are 64 contiguous bytes: lanes 0-7 read one each, the empty
             * rows' out-masks are cleared in one store, and only the non-empty rows are visited. */
            for (;;) {
                unsigned b0 = 0u;
                if (lane == 0) b0 = atomicAdd(replay_cursor(a), kReplayChunk);
                b0 = (unsigned)__builtin_amdgcn_readfirstlane((int)b0);
                if (b0 >= n_blk) break;
                const unsigned b1 = min(b0 + kReplayChunk, n_blk);
                for (unsigned b = b0; b < b1; ++b) {
                    unsigned long long m = 0ull;
                    if (lane < (int)kBlockRows) {
                        m = reinterpret_cast<const unsigned long long*>(a.sample_blocks + (size_t)b * kBlockBytes + kBlockTrailer)[lane];
                        if (m == 0ull)                                 /* the planes hold another frame's masks */
                            reinterpret_cast<unsigned long long*>(kp.out_blocks + (size_t)b * kOutBlockBytes + kOutBlockMasks)[lane] = 0ull;
                    }
                    unsigned rows = (unsigned)__ballot(m != 0ull);     /* bit k: row k has samples */
                    const unsigned m_lo = (unsigned)m, m_hi = (unsigned)(m >> 32);
                    while (rows != 0u) {
                        const unsigned k = (unsigned)__ffs((int)rows) - 1u;
                        rows &= rows - 1u;
                        const unsigned long long mask = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)m_lo, (int)k) |
                                                        ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)m_hi, (int)k) << 32);
                        replay_row<MEDIA>(a, kp, b, k, mask, lane);
                    }
                }
            }
            return;
        }
    }
    const unsigned total = n_blk * kBlockRows;
    const unsigned n_waves = gridDim.x * 4u;
    /* (Round 5 also tried this loop software-pipelined by hand -- the next row's planes and the mask after it in flight while a
     * row is evaluated -- and measured nothing, 58.2 against 58.6-59.0 ms on the key-1 frame: the head-of-row round trip is not
     * what keeps this kernel at 0.62-0.65 of the VALU issue rate; profiles/r05_eval_prefetch_ab.txt.) */
    unsigned pruned = 0u;                                              /* wave-uniform; the fill only */
    for (unsigned row = blockIdx.x * 4u + (threadIdx.x >> 6); row < total; row += n_waves) {
        uint8_t* blk = a.sample_blocks + (size_t)(row / kBlockRows) * kBlockBytes;
        const unsigned k = row % kBlockRows;
        unsigned long long* mask_p = reinterpret_cast<unsigned long long*>(blk + kBlockTrailer) + k;
        const unsigned long long mask = *mask_p;
        uint8_t* const oblk = KEEP ? kp.out_blocks + (size_t)(row / kBlockRows) * kOutBlockBytes : nullptr;
        unsigned long long* const omask_p = KEEP ? reinterpret_cast<unsigned long long*>(oblk + kOutBlockMasks) + k : nullptr;
        if (mask == 0ull) {                                           /* wave-uniform */
            if (KEEP && lane == 0) *omask_p = 0ull;                   /* the planes hold another frame's masks */
            continue;
        }
        const bool mine = (mask >> lane) & 1ull;
        float* f = reinterpret_cast<float*>(blk + k * kRowData) + lane;
        bool has = false;
        float ex = 0.f, ey = 0.f, ez = 0.f, s = 1.0f;
        if constexpr (KEEP) {                                          /* sample records (kOutBlockEnv) */
            float* e = reinterpret_cast<float*>(oblk + kOutBlockEnv + k * kOutEnvData) + lane;
            SampleRecord rec;
            if (!kp.replay) {                                          /* the fill: raw row -> record, in place */
                bool keep = false;
                if (mine) {
                    const v3 rel_p = mk(f[0], f[64], f[128]);
                    const v3 vel = mk(f[192], 0.0f, f[256]);          /* vel.y: see kRowPlanes */
                    float r2, r, yv;
                    march_radius<ARITH>(rel_p, r2, r, yv);
                    rec = sample_record(rel_p, r, vel, a.spin);
                    f[0] = rec.rc; f[64] = rec.y; f[128] = rec.azimuth; f[192] = rec.shift_g; f[256] = rec.r;
                    e[0] = rec.env_acc; e[64] = rec.env_dust;
                    keep = !record_prunable(rec);
                }
                const unsigned long long kept = __ballot(keep);
                if (kept != mask && lane == (int)(__ffsll((long long)mask) - 1)) *mask_p = kept;
                pruned += (unsigned)__popcll(mask ^ kept);
            } else if (mine) {                                         /* (a replay has left above: replay_row) */
                rec.rc = f[0]; rec.y = f[64]; rec.azimuth = f[128]; rec.shift_g = f[192]; rec.r = f[256];
                rec.env_acc = e[0]; rec.env_dust = e[64];
            }
            if (mine) has = eval_sample_record<MEDIA>(rec, a.time, record_step(rec, kHNear, kHDisk, kHVac), a.lut_acc, a.lut_dust,
                                                      a.dust_bands, ex, ey, ez, s);
        } else if (mine) {
            const v3 rel_p = mk(f[0], f[64], f[128]);
            const v3 vel = mk(f[192], 0.0f, f[256]);                  /* vel.y: see kRowPlanes */
            float r2, r, yv;
            march_radius<ARITH>(rel_p, r2, r, yv);
            const bool near_bh = r < 18.0f;
            const bool in_disk = fabsf(rel_p.y) < kDiskH * 5.0f && r < kDiskOut + 5.0f;
            const bool in_cloud = fabsf(rel_p.y) < kCloudH * 1.5f && r < kCloudOut;
            const float h = near_bh ? kHNear : (in_disk ? kHDisk : kHVac);
            float d_disk, d_cloud;
            media_densities<MEDIA>(rel_p, a.time, in_disk, in_cloud, a.lut_acc, a.lut_dust, a.dust_bands, nullptr, d_disk, d_cloud);
            has = sample_emission(d_disk, d_cloud, rel_p, r, vel, h, a.spin, ex, ey, ez, s);
        }
        /* Round 5: a sample raymarcher.cu:71 would not take is the identity of the accumulation -- the single kernel skips it,
         * and so does pass 3 now: such lanes leave the row's mask instead of storing (0, 0, 0, 1) (the march pools every sample
         * inside the radial gate and the slab: from inside the disk most of them are real, on the bench view most are not). */
        const unsigned long long live = __ballot(has);
        if (KEEP) {                                                    /* the row keeps its inputs and its mask */
            float* g = reinterpret_cast<float*>(oblk + k * kOutRowData) + lane;
            if (has) { g[0] = ex; g[64] = ey; g[128] = ez; g[192] = s; }
            if (lane == (int)(__ffsll((long long)mask) - 1)) *omask_p = live;
        } else {
            if (has) { f[0] = ex; f[64] = ey; f[128] = ez; f[192] = s; }
            if (live != mask && lane == (int)(__ffsll((long long)mask) - 1)) *mask_p = live;
        }
    }
    if (KEEP && pruned != 0u && lane == 0) atomicAdd(&a.ctr->pruned_lanes, pruned);      /* one per wave of the grid, at most */
}

/* ---- pass 3: composite each ray's samples in march order; shade the rays of wavefronts that have reached their end;
 *      LAST (the last round the host enqueued): rays still suspended are finished with the media sampled in line ---- */
template <bool SPIN, int ARITH, int MEDIA, bool LAST, bool KEEP = false>
__global__ __launch_bounds__(kWGThreads) void composite_and_shade(const FrameArgs a, const KeepArgs kp) {
    const bool replay = KEEP && kp.replay != 0;                             /* retained rows: one round, long finished */
    if constexpr (KEEP) {
        /* this launch's pass 2 has handed out all its blocks (stream order) and the cache's next launch waits for this kernel
         * (MarchCacheObject::chained): the hand-out cursor goes back to 0 here, one lane of one workgroup */
        if (replay && (blockIdx.x | blockIdx.y | threadIdx.x) == 0u) *replay_cursor(a) = 0u;
    }
    if (!replay && a.ctr->rounds_run != 0u && a.ctr->last_overflow == 0u) return;      /* a later round with nothing left: all leave */
    const unsigned long long t_start = a.tile_cost ? __builtin_readcyclecounter() : 0ull;
    int x, y, out_row;
    if (!lane_pixel(a, x, y, out_row)) return;
    const int lane = threadIdx.x & 63;
    const unsigned wid = wave_slot(a);
    const unsigned state = replay ? 1u : a.hdr[wid].state;
    if (state != 1u && state != 2u) return;                        /* shaded in an earlier round */
    const size_t li = (size_t)wid * 64 + lane;
    Radiance acc = {0.f, 0.f, 0.f, 1.0f};
    if (a.hdr[wid].flags & 1u) {                                   /* the radiance composited in earlier rounds */
        acc.r = a.finals[7 * a.n_lanes + li]; acc.g = a.finals[8 * a.n_lanes + li];
        acc.b = a.finals[9 * a.n_lanes + li]; acc.t = a.finals[10 * a.n_lanes + li];
    }
    unsigned run_start = a.hdr[wid].first_block, run_len = 1;
    const unsigned n_runs = min(a.hdr[wid].n_runs, kMaxRunsWalked);
    for (unsigned rn = 0; rn < n_runs; ++rn) {
        const unsigned* link = reinterpret_cast<const unsigned*>(a.sample_blocks + (size_t)run_start * kBlockBytes +
                                                                 kBlockTrailer + kBlockRows * 8);
        const unsigned next_start = link[0], next_len = link[1];
        if (run_len > kMaxRun || run_start + run_len > a.block_capacity) break;    /* never walk outside the pool */
        /* Blocks of a run are consecutive, so several can be in flight at once: the walk is bound by load
         * latency (a heavy wave has ~250 blocks), not by arithmetic.  kNB blocks' loads are issued together,
         * then their rows are accumulated in order. */
        constexpr unsigned kNB = 4;
        for (unsigned b = 0; b < run_len; b += kNB) {
            float e[kNB][kBlockRows][4];
            unsigned long long m[kNB][kBlockRows];
            /* unconditional, address-independent loads (rows a lane does not own are read and ignored): conditional loads
             * serialise into one memory round trip per row -- also when the condition is wave-uniform: skipping the rows whose
             * mask pass 2 has emptied cost this pass 30-150 % (round 5, profiles/r05_pass_counters.txt) for 25 % fewer bytes */
#pragma unroll
            for (unsigned j = 0; j < kNB; ++j) {
                const size_t bi = run_start + (b + j < run_len ? b + j : b);
                const uint8_t* blk = KEEP ? kp.out_blocks + bi * kOutBlockBytes : a.sample_blocks + bi * kBlockBytes;
                const unsigned long long* masks = reinterpret_cast<const unsigned long long*>(blk + (KEEP ? kOutBlockMasks : kBlockTrailer));
#pragma unroll
                for (unsigned k = 0; k < kBlockRows; ++k) {
                    m[j][k] = masks[k];
                    const float* f = reinterpret_cast<const float*>(blk + k * (KEEP ? kOutRowData : kRowData)) + lane;
                    e[j][k][0] = f[0]; e[j][k][1] = f[64]; e[j][k][2] = f[128]; e[j][k][3] = f[192];
                }
            }
#pragma unroll
            for (unsigned j = 0; j < kNB; ++j) {
                const bool live = b + j < run_len;                 /* wave-uniform */
#pragma unroll
                for (unsigned k = 0; k < kBlockRows; ++k)
                    if (live && ((m[j][k] >> lane) & 1ull))
                        accumulate_emission(acc, e[j][k][0], e[j][k][1], e[j][k][2], e[j][k][3]);
            }
        }
        run_start = next_start; run_len = next_len;
    }
    const int leader = __ffsll((long long)__ballot(1)) - 1;
    if (!LAST && state == 2u) {
        /* the wave is suspended: keep what has been composited; the next round's march resumes its rays */
        a.finals[7 * a.n_lanes + li] = acc.r; a.finals[8 * a.n_lanes + li] = acc.g;
        a.finals[9 * a.n_lanes + li] = acc.b; a.finals[10 * a.n_lanes + li] = acc.t;
        if (lane == leader) a.hdr[wid].flags = 1u;
        if (a.tile_cost) add_tile_cost(a, t_start);
        return;
    }
    float uvx, uvy;
    v3 p, vel;
    primary_ray(a, x, y, uvx, uvy, p, vel);
    vel = mk(a.finals[li], a.finals[a.n_lanes + li], a.finals[2 * a.n_lanes + li]);
    const unsigned code = reinterpret_cast<const unsigned*>(a.finals)[3 * a.n_lanes + li];
    bool hit = (code >> 31) != 0;
    int steps = (int)(code & 0x3fffffffu);
    if (LAST && state == 2u && (code & 0x40000000u)) {
        /* the pool ran out under this ray at step `steps` and no round is left: carry on from its saved pre-step state
         * with the media sampled in line -- the samples composited above come first, exactly as in the single kernel */
        p = mk(a.finals[4 * a.n_lanes + li], a.finals[5 * a.n_lanes + li], a.finals[6 * a.n_lanes + li]);
        march_inline<SPIN, MEDIA, ARITH>(a, p, vel, acc, hit, steps, nullptr);
    }
    if (hit) acc.t = 0.0f;                                         /* raymarcher.cu:49 */
    shade_and_store<false>(a, x, y, out_row, uvx, uvy, hit, p, vel, acc, steps);
    if (!replay && lane == leader) a.hdr[wid].state = 3u;
#ifndef RRT_WAVE_TIMELINE
    if (a.tile_cost) add_tile_cost(a, t_start);
#endif
}

/* ---- coarse cost probe (round 4): one march-only ray per cell of stride_x x stride_y pixels of the launch's row map.
 * No media evaluation, no shading: the geodesic with the march's own step rule, counting steps and the steps that would
 * need an accretion / a dust sample.  cost = w_step steps + w_acc n_acc + w_dust n_dust, in the unit of the measured tile
 * costs (wave clocks / 16: a 1000-step wave at full occupancy ~ 1.7e5), so that the same radix sort orders both.  Used
 * (i) to dispatch the FIRST frame of a geometry longest-first (rrt_tile_order has no history yet) and (ii) on the host, to
 * weigh row tiles before they are dealt to the GPUs (rrt_probe_tile_costs -> rrt_tile_map_balance).  The weights are a
 * least-squares fit of this model to measured wave-tile costs of six 4K views (tools/probe_fit.py,
 * profiles/r04_probe_cost_fit.txt). */
struct ProbeArgs {
    unsigned* cell_cost;       /* cells_y x cells_x */
    int cells_x, cells_y, stride_x, stride_y;
    float w_step, w_acc, w_dust;
    float ring_steps;          /* max_steps: what a wave on the critical curve marches */
};
#ifndef RRT_PROBE_W_STEP
#define RRT_PROBE_W_STEP 180.0f
#define RRT_PROBE_W_ACC 730.0f
#define RRT_PROBE_W_DUST 630.0f
#endif
constexpr int kProbeStride = 16;

/* The probe is latency-bound, not throughput-bound: a few hundred wavefronts on a chip with 8 192 wave slots, each a
 * serial march -- and a lone wavefront retires a dependent instruction every ~10 clocks (profiles/r04_wave_timeline_default.txt),
 * so a faithful 1000-step march took 1.6 ms however few rays there were.  It therefore marches COARSELY: kProbeStepScale times the
 * reference's step in every zone (0.3 / 0.09 / 0.03 -> 1.2 / 0.36 / 0.12; classic RK4 is still well inside its accuracy range for
 * a cost estimate) in the fast arithmetic (FMA, v_rsq): ~0.15 ms.  Every probe step stands for kProbeStepScale real ones. */
constexpr int kProbeStepScale = 4;
template <bool SPIN>
__global__ __launch_bounds__(64) void probe_costs(const FrameArgs a, const ProbeArgs q) {
    const int lane = threadIdx.x & 63;
    const int cx = blockIdx.x * 8 + (lane & 7), cy = blockIdx.y * 8 + (lane >> 3);
    if (cx >= q.cells_x || cy >= q.cells_y) return;
    /* the cell's representative pixel: its centre, in the LOCAL rows of the launch (a shard probes its own tiles only) */
    int lr = cy * q.stride_y + q.stride_y / 2, y = 0, out_row = 0;
    if (lr >= a.rows.n_local_rows) lr = a.rows.n_local_rows - 1;
    if (!map_row(a.rows, a.height, lr, y, out_row) && !map_row(a.rows, a.height, cy * q.stride_y, y, out_row)) {
        q.cell_cost[cy * q.cells_x + cx] = 0u;
        return;
    }
    const int xc = cx * q.stride_x + q.stride_x / 2;
    const int x = xc < a.width ? xc : a.width - 1;
    float uvx, uvy;
    v3 p, vel;
    primary_ray(a, x, y, uvx, uvy, p, vel);
    const int max_probe = (a.max_steps + kProbeStepScale - 1) / kProbeStepScale;
    int steps = max_probe;
    unsigned n_acc = 0, n_dust = 0;
    bool captured = false;
    for (int k = 0; k < max_probe; ++k) {
        const v3 rel_p = p;
        const float r2 = dot_fma(rel_p, rel_p);
        const float yv = __builtin_amdgcn_rsqf(r2);
        const float r = r2 * yv;
        if (!(r >= kEventHorizon * 1.01f)) { steps = k; captured = true; break; }              /* horizon (or NaN) */
        const bool near_bh = r < 18.0f;
        const bool in_disk = fabsf(rel_p.y) < kDiskH * 5.0f && r < kDiskOut + 5.0f;
        const bool in_cloud = fabsf(rel_p.y) < kCloudH * 1.5f && r < kCloudOut;
        const float h = (float)kProbeStepScale * (near_bh ? kHNear : (in_disk ? kHDisk : kHVac));
        integrate_rk4_fast<SPIN>(p, vel, h, 0.5f * h, h * (1.0f / 6.0f), a.drag_c, r2, yv);
        if (in_disk || in_cloud) {
            const float rc2 = rel_p.x * rel_p.x + rel_p.z * rel_p.z;
            if (rc2 >= kIsco * kIsco && rc2 <= kDiskOut * kDiskOut) {
                /* the slab early-out of disk_point(): y^2 rc > 135 ends both densities twelve instructions in */
                if (rel_p.y * rel_p.y * rel_p.y * rel_p.y * rc2 <= 135.0f * 135.0f) { n_acc += in_disk; n_dust += in_cloud; }
            }
        }
        if (r > 250.0f && dot(rel_p, vel) > 0.0f) { steps = k + 1; break; }
    }
    const float c = (float)kProbeStepScale * (q.w_step * (float)steps + q.w_acc * (float)n_acc + q.w_dust * (float)n_dust);
    /* bit 0: the ray ended on the horizon.  Cells whose neighbours disagree about that hold the CRITICAL CURVE (the edge
     * of the shadow), whose rays orbit until MAX_STEPS: a ring a pixel or two wide that a sample every 16 pixels mostly
     * misses, and the longest waves of the frame (probe_to_tiles prices those cells at max_steps). */
    const unsigned ci = c >= (float)kTileCostMax ? kTileCostMax : (unsigned)c;
    q.cell_cost[cy * q.cells_x + cx] = (ci & ~1u) | (captured ? 1u : 0u);
}
/* every wave tile (tiles_x x tiles_y of kWGPixX x kWGPixY pixels) takes the cost of the probe cell it lies in */
__global__ __launch_bounds__(256) void probe_to_tiles(unsigned* tile_cost, unsigned tiles_x, unsigned tiles_y, ProbeArgs q) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= tiles_x * tiles_y) return;
    const unsigned rb = t / tiles_x, col = t - rb * tiles_x;
    int cx = (int)(col * kWGPixX) / q.stride_x, cy = (int)(rb * kWGPixY) / q.stride_y;
    cx = cx < q.cells_x ? cx : q.cells_x - 1; cy = cy < q.cells_y ? cy : q.cells_y - 1;
    const unsigned own = q.cell_cost[cy * q.cells_x + cx];
    unsigned cost = own;
    /* 3 x 3 neighbourhood: the largest estimate (thin structures between samples), and -- where captured and escaping
     * samples meet -- the cost of a wave that marches to max_steps */
    bool mixed = false;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int nx = cx + dx, ny = cy + dy;
            if (nx < 0 || ny < 0 || nx >= q.cells_x || ny >= q.cells_y) continue;
            const unsigned c = q.cell_cost[ny * q.cells_x + nx];
            mixed = mixed || ((c ^ own) & 1u);
            cost = c > cost ? c : cost;
        }
    if (mixed) {
        const float ring = q.w_step * q.ring_steps;
        const unsigned rc = ring >= (float)kTileCostMax ? kTileCostMax : (unsigned)ring;
        cost = rc > cost ? rc : cost;
    }
    tile_cost[t] = cost;
}

/* one wavefront sleeps for `ticks` of the 100 MHz counter and reports both counters' deltas (rrt_clock_probe) */
__global__ __launch_bounds__(64) void clock_probe_kernel(unsigned long long* out, unsigned long long ticks) {
    const unsigned long long c0 = __builtin_readcyclecounter(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long r1 = r0;
    for (unsigned it = 0; it < (1u << 24) && r1 - r0 < ticks; ++it) {       /* bounded: ~1.3 us per turn */
        __builtin_amdgcn_s_sleep(127);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long c1 = __builtin_readcyclecounter();
    if (threadIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

/* scatter one shard's tile buffer into the full bottom-up frame */
__global__ __launch_bounds__(256) void assemble_tiles_kernel(uchar4* frame, const uchar4* tiles, int width,
                                                            int height, RowMap m) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= width) return;
    for (int lr = blockIdx.y; lr < m.n_local_rows; lr += gridDim.y) {        /* gridDim.y is capped at kMaxGridY */
        int y, out_row;
        if (map_row(m, height, lr, y, out_row))
            frame[(size_t)(height - 1 - y) * width + x] = tiles[(size_t)out_row * width + x];
    }
}

/* all shards in one launch: `tiles` holds n_shards buffers, `shard_stride` pixels apart */
__global__ __launch_bounds__(256) void assemble_all_kernel(uchar4* frame, const uchar4* tiles, size_t shard_stride,
                                                          int width, int height, int tile_rows, int n_shards) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= width) return;
    for (int y = blockIdx.y; y < height; y += gridDim.y) {                   /* image row; gridDim.y capped */
        const int t = y / tile_rows, rr = y - t * tile_rows;
        const int shard = t % n_shards, k = t / n_shards;
        const int rows_k = min(tile_rows, height - t * tile_rows);
        const size_t src_row = (size_t)k * tile_rows + (rows_k - 1 - rr);
        frame[(size_t)(height - 1 - y) * width + x] = tiles[shard * shard_stride + src_row * width + x];
    }
}

/* all shards of an explicit tile map (rrt_tile_map) in one launch */
__global__ __launch_bounds__(256) void assemble_map_kernel(uchar4* frame, const uchar4* tiles, size_t shard_stride, int width,
                                                          int height, int tile_rows, const int* shard_of_tile, const int* k_of_tile) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= width) return;
    for (int y = blockIdx.y; y < height; y += gridDim.y) {
        const int t = y / tile_rows, rr = y - t * tile_rows;
        const int rows_k = min(tile_rows, height - t * tile_rows);
        const size_t src_row = (size_t)k_of_tile[t] * tile_rows + (rows_k - 1 - rr);
        frame[(size_t)(height - 1 - y) * width + x] = tiles[shard_of_tile[t] * shard_stride + src_row * width + x];
    }
}

#endif  /* RRT_KERNELS_H */
