/*
 * rrt.h -- C ABI of librrt_hip.so, the MI355X (gfx950) implementation of the
 * per-pixel geodesic ray-march hot path of levi2234/RelativisticRayTracer.
 *
 * This is the drop-in boundary.  The one entry point of the reference's path is
 *
 *     void launch_raymarch(uchar4* d_out, int w, int h, float time,
 *                          CameraState cam, cudaTextureObject_t skyboxTex,
 *                          CameraEffects effects);
 *                                   -- reference include/raymarcher.h:19,
 *                                      defined src/raymarcher.cu:176-180,
 *                                      called from src/main.cpp:467
 *
 * `include/raymarcher.h` of this repo re-declares it source-compatibly (C++);
 * librrt_hip.so exports it as a real C++ symbol, under the reference's own
 * mangled name too, over rrt_launch_raymarch() below; everything here is
 * plain C: pointers, ints, floats and PODs -- no HIP or torch types.
 *
 * Conventions
 *   - every function returns an rrt_status (0 = RRT_OK); nothing throws;
 *   - `d_*` pointers are DEVICE pointers owned by the caller;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream);
 *     launches are asynchronous exactly like the reference's (raymarcher.cu:179);
 *   - the library keeps no per-call state and allocates nothing in a launch,
 *     so launches may be captured into a hipGraph (what a launch needs beyond its arguments -- a pool, noise tables, a
 *     tile-order object -- are caller-owned objects created beforehand; the one exception is documented at
 *     rrt_tile_order: its FIRST launch of a larger geometry sizes its buffers, and captured launches ignore it).
 */
#ifndef RRT_H
#define RRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRT_ABI_VERSION 5      /* 5: RRT_ARITH_FMAD, rrt_params.nudge_ulps / .nudge_seed, rrt_params_init (an rrt_params of ABI 4's
                                     48 bytes is still accepted: the new fields read as 0);
                                  4: rrt_params.struct_size (leading), .pool_rounds, .pass_chains, rrt_tile_map_*, rrt_probe_tile_costs,
                                     rrt_clock_probe; 3: rrt_params.tile_order, rrt_tile_order_* */

typedef enum {
    RRT_OK = 0,
    RRT_ERR_INVALID_ARGUMENT = 1,
    RRT_ERR_NO_DEVICE = 2,
    RRT_ERR_HIP = 3,          /* a HIP runtime call failed; see rrt_last_hip_error() */
    RRT_ERR_BAD_HANDLE = 4,
    RRT_ERR_OUT_OF_MEMORY = 5,
    RRT_ERR_ABI_MISMATCH = 6  /* an rrt_params whose struct_size is not this library's: built against another include/rrt.h */
} rrt_status;

/* Camera basis handed to the kernel.  Layout == reference `struct CameraState`
 * (include/raymarcher.h:11-16): four packed float3, 48 bytes. */
typedef struct rrt_camera {
    float pos[3];
    float forward[3];
    float right[3];
    float up[3];
} rrt_camera;

/* Per-pixel camera effects.  Layout == reference `struct CameraEffects`
 * (include/camera_effects/camera_settings.h:4-17): 36 bytes, bools padded to
 * 4-byte slots (offsets 0,4,8,12,16,20,24,28,32). */
typedef struct rrt_effects {
    uint8_t use_bloom;       uint8_t _pad0[3];
    float bloom_threshold;
    float bloom_intensity;
    uint8_t use_vignette;    uint8_t _pad1[3];
    float vignette_intensity;
    uint8_t use_chromatic_aberration; uint8_t _pad2[3];
    float ca_amount;
    uint8_t use_lens_distortion;      uint8_t _pad3[3];
    float distortion_amount;
} rrt_effects;

/* Scene / quality parameters.  Defaults == the reference's compile-time
 * constants (include/config.h:18-48); `spin` replaces the SPIN_A macro
 * (config.h:21) so that Kerr a=0.9 / 0.99 are run-time settings. */
typedef struct rrt_params {
    uint32_t struct_size;    /* sizeof(rrt_params) of the header the caller was compiled against; rrt_params_default()
                                fills it in.  Every entry point that takes an rrt_params accepts this header's size and
                                ABI 4's 48 bytes (a prefix: the fields behind it read as their defaults) and refuses any
                                other value with RRT_ERR_ABI_MISMATCH (objects built against the ABI <= 3 header, whose
                                struct began with `spin`, must be recompiled)                                */
    float spin;              /* SPIN_A            config.h:21  default 0.0  */
    int32_t max_steps;       /* MAX_STEPS         config.h:48  default 2000 */
    int32_t volumetrics;     /* 1 = full disk + dust (reference behaviour);
                                0 = "skybox only": both densities read 0,
                                zone-dependent step sizes unchanged        */
    int32_t sky_frac_bits;   /* bilinear weight bits of the sky sampler:
                                8 = CUDA-texture-like (default), 0 = exact  */
    int32_t arith_mode;      /* RRT_ARITH_STRICT (default): every operation rounded as the
                                reference source writes it -- the bit-parity path.
                                RRT_ARITH_FMAD: the geodesic integrator with multiply-adds FUSED and
                                division / square root still correctly rounded -- the arithmetic class
                                of the reference's own build (nvcc defaults: -fmad=true, IEEE div/sqrt);
                                media, sky and post-FX code unchanged.  Within the 1e-4 tolerance of the
                                strict frame on every pixel whose strict value is itself stable under a
                                few-ulp nudge of its primary ray (tests/test_gpu_tolerance.py).
                                RRT_ARITH_FAST: fused multiply-adds and 1-ulp reciprocal
                                square roots, no correctly rounded divide; informational.       */
    int32_t workspace;       /* 0 (default): single kernel, media sampled in line by the marching
                                lane.  An rrt_workspace id: three-pass path -- the march only
                                records in-medium sample points, which the whole chip then evaluates
                                and a last pass composites in march order.  Same bytes out; removes
                                the per-wavefront long pole of disk-grazing rays, which is what
                                strong scaling over GPUs needs.           */
    int32_t path_policy;     /* with a workspace: RRT_PATH_AUTO (default) takes the three-pass path for
                                launches of <= 1.5 M rays (where it is faster) and the single kernel
                                otherwise; RRT_PATH_SINGLE / RRT_PATH_THREE_PASS force one             */
    int32_t noise_table;     /* 0 (default): every noise3D hashes its eight lattice corners arithmetically.
                                An rrt_noise_table id: the low octaves of the disk / dust noise read the corner
                                hashes from a precomputed lattice table whenever the 64 rays of a wavefront
                                share a few lattice cells (4K / 8K frames: most of them) -- same bits, about
                                half the media cost.  A launch whose `time` lies outside
                                the table's window [t0, t1] (rrt_noise_table_window) hashes arithmetically.  */
    int32_t tile_order;      /* 0 (default): wave tiles are dispatched in the static order (row blocks from the middle
                                of the frame outwards).  An rrt_tile_order id: the launch records what every wave tile
                                cost and the next launch of the same geometry through that object dispatches
                                longest-first -- same pixels; removes the drain of views whose long rays are not in the
                                middle (a 4K frame from inside the disk: 53 -> 46 ms), nothing to gain on the
                                reference's default view.  With no history for the launch's geometry the order comes
                                from a coarse march-only probe of the same view (one ray per 16x16 pixels, run on the
                                launch's stream right before it).  Both paths; a launch that is being captured into a
                                hipGraph renders in the static order and leaves the object alone.              */
    int32_t pool_rounds;     /* three-pass path: the workspace pool is reused in ROUNDS -- march until the pool is full,
                                evaluate and composite what was pooled, resume the suspended rays -- so that any pool
                                serves any view.  0 (default): automatic -- as many rounds as the workspace's previous
                                launch needed, plus one, at least 2; n > 0: exactly up to n rounds.  Rays still
                                suspended after the last round finish with the media sampled in line (same bytes).   */
    int32_t pass_chains;     /* three-pass path: 0 (default) = automatic -- a launch of >= 2 048 wavefronts is cut in two
                                along its dispatch order and the halves run their march -> evaluate -> composite chains
                                side by side (the workspace's own second stream), so that one half's evaluation fills the
                                other half's march tail; 1 = one chain; 2 = two whenever possible.  Same bytes.  A caller that
                                keeps SEVERAL launches in flight on streams of its own (frames of an animation) should ask for
                                1: the other frames already fill a launch's tails, and the extra streams only get in each
                                other's way (a rank's share of a 4K frame, three in flight: 6.8 instead of 7.4 ms).  With four
                                or more in flight RRT_PATH_SINGLE is usually faster still -- unless the view has a wavefront
                                that takes longer than the frames in flight together.                   */
    int32_t nudge_ulps;      /* conditioning probe (ABI 5).  0 (default): primary rays exactly as raymarcher.cu:27-34 forms
                                them.  K > 0: every component of every pixel's normalised primary direction is moved by a
                                pseudo-random whole number of ulps in [-K, K] (a hash of pixel and nudge_seed; the oracle has
                                the same function).  Rendering a frame under a few such nudges shows which pixels the
                                reference's own arithmetic does not determine to the tolerance -- near-critical rays, zone
                                and density gates about to flip: how the within-tolerance arithmetic modes are accounted for. */
    uint32_t nudge_seed;
} rrt_params;

#define RRT_PATH_AUTO 0
#define RRT_PATH_SINGLE 1
#define RRT_PATH_THREE_PASS 2

#define RRT_ARITH_STRICT 0
#define RRT_ARITH_FAST 1
#define RRT_ARITH_FMAD 2

/* Opaque sky-texture handle; stands in for cudaTextureObject_t
 * (`unsigned long long`, reference src/main.cpp:231-263). */
typedef unsigned long long rrt_sky_t;

/* Optional per-ray outputs of rrt_launch_raymarch_ex (device pointers, any may
 * be NULL).  Indexing: `ldr`/`hdr` like the RGBA8 frame (bottom-up rows,
 * raymarcher.cu:168); the others top-down, y*width + x. */
typedef struct rrt_debug_outputs {
    float* d_ldr;            /* 4 floats/pixel: tone-mapped r,g,b before the u8 cast, 1 */
    float* d_hdr;            /* 4 floats/pixel: final_hdr after post-FX, 1              */
    int32_t* d_steps;        /* RK4 steps taken                                         */
    int32_t* d_hit;          /* 1 = ray ended on the horizon                            */
    float* d_pos;            /* 3 floats/pixel: final position                          */
    float* d_vel;            /* 3 floats/pixel: final velocity                          */
    float* d_rad;            /* 4 floats/pixel: intensity r,g,b and transmittance       */
    unsigned* d_lut_oob;     /* 1 counter: noise-table reads whose index had to be clamped
                                (must stay 0: the table box covers every reachable cell)  */
} rrt_debug_outputs;

/* ---- library ---- */
int rrt_abi_version(void);
const char* rrt_status_string(int status);
const char* rrt_last_hip_error(void);          /* thread-local text of the last HIP failure */
int rrt_device_count(int* count);
int rrt_path_auto_max_rays(void);             /* RRT_PATH_AUTO takes the three-pass path for launches of at most this many rays (1 500 000) */
/* config.h defaults into the first `size` bytes of an rrt_params and struct_size = size.  Call it through the macro below, so
 * that `size` is the sizeof of the header the CALLER was compiled against: the library then knows which fields the caller
 * has.  Accepted sizes: this header's, and ABI 4's 48 bytes (fields the caller does not have read as their defaults); any
 * other size is RRT_ERR_ABI_MISMATCH here and at every entry point that takes an rrt_params. */
int rrt_params_init(void* prm, uint32_t size);
#define rrt_params_default(p) rrt_params_init((p), (uint32_t)sizeof(rrt_params))
/* (the library also keeps the exports older headers mapped the name to: rrt_params_default_v4 fills ABI 4's 48 bytes -- such a
 * binary keeps working --, rrt_params_default the 36-byte ABI <= 3 layout, whose binaries are refused at their first launch) */
int rrt_effects_default(rrt_effects* fx);      /* camera_settings.h:5-16 defaults          */

/* ---- sky texture: replaces loadSkybox()'s cudaMallocArray + texture object,
 *      reference src/main.cpp:246-263.  RGBA8, row 0 = top of the panorama. ---- */
int rrt_sky_create(const uint8_t* rgba8_host, int width, int height, rrt_sky_t* out);
int rrt_sky_create_from_device(const void* d_rgba8, int width, int height, rrt_sky_t* out); /* borrows */
int rrt_sky_destroy(rrt_sky_t sky);

/* ---- workspace of the three-pass path (rrt_params.workspace): a caller-owned HBM pool, so that a
 *      launch still allocates nothing.  One workspace serves one stream at a time (it owns a second stream of its
 *      own for the second chain, rrt_params.pass_chains; forked from and joined to the caller's by events).  ~1.5 KB per
 *      wave-step that touches the media (handed out in blocks of 8 rows, runs of up to 8 blocks); the 4K bench frame
 *      pools 2.6 GB, an eighth of it 0.3 GB, an eighth of a 4K view from inside the disk 1.9 GB.  The pool is reused in
 *      ROUNDS (rrt_params.pool_rounds): the wavefronts it runs out under are suspended and resumed once the pooled
 *      samples have been evaluated and composited, so any pool serves any view; only rays still suspended after the last
 *      enqueued round are finished by the in-line code (same result either way; one round is the fast case). ---- */
int rrt_workspace_create(size_t bytes, int* out_id);
int rrt_workspace_destroy(int id);
/* after a launch has completed: rows used and wavefronts that fell back (synchronous read) */
int rrt_workspace_stats(int id, unsigned* rows_used, unsigned* overflow_waves);
/* rounds of the last launch (rrt_params.pool_rounds): enqueued, with work for the march, rows of the fullest round, and
 * an upper bound of the pool's rows.  rrt_workspace_stats: rows_used = all rounds together, overflow_waves = wavefronts
 * still suspended after the last round (finished in line). */
int rrt_workspace_rounds(int id, unsigned* rounds_enqueued, unsigned* rounds_with_work, unsigned* peak_rows, unsigned* pool_rows);
/* inspection: copy `bytes` of the pool starting at `offset` to host memory (synchronous) */
int rrt_workspace_read(int id, size_t offset, size_t bytes, void* host_dst);

/* ---- cost-ordered dispatch (rrt_params.tile_order; no counterpart in the reference, whose launch is one fixed grid,
 *      src/raymarcher.cu:176-180).  The object holds, per 8x8-pixel wave tile, the shader clocks the last launch
 *      through it took, and the permutation (sorted on the device right after that launch, on its stream) the next
 *      launch with the same width / height / row map reads.  A launch with another geometry renders in the static order
 *      and starts over.  Launches through one object are serialised on the device, also across streams: give every frame
 *      that should overlap another its own object (the headless drivers: one per slot).  Frames of an animation change
 *      little from one to the next, which is what makes the previous frame's costs a good order for this one.  With NO
 *      history (first launch, new geometry) the order comes from a coarse probe of the view itself: one march-only ray per
 *      16x16 pixels on the launch's stream (~1/250 of the frame's work), costed by a fitted model -- a still image from
 *      inside the disk gets most of the gain too; rrt_tile_order_set_seeding(id, 0) switches that off.  The first
 *      launch of a (larger) geometry allocates the object's buffers -- a synchronising call.  A launch that is being
 *      CAPTURED into a hipGraph ignores the object (static order, nothing recorded): a replayed graph can then never read
 *      a permutation that a later live launch is rewriting.  Works on both paths (single kernel and three-pass). ---- */
int rrt_tile_order_create(int* out_id);
/* Must be called with the device that owns the object CURRENT (the one that was current at create): under another device it
 * returns RRT_ERR_BAD_HANDLE and frees NOTHING -- the handle stays valid and the call can be repeated from the right device
 * (rrt_tile_map_destroy: the same rule).  A caller that ignores the status there leaks the object's device buffers. */
int rrt_tile_order_destroy(int id);
int rrt_tile_order_set_seeding(int id, int on);
int rrt_tile_order_seeded(int id, unsigned long long* seeded_launches);      /* launches ordered by the probe */
/* counters; with perm_host / cost_host (either may be NULL; `capacity` elements each) also, after waiting for the
 * object's last launch, the order the next matching launch will use and the costs the last one recorded */
int rrt_tile_order_info(int id, unsigned long long* launches, unsigned long long* ordered_launches, unsigned* n_tiles,
                        unsigned* perm_host, unsigned* cost_host, unsigned capacity);

/* ---- lattice-hash tables for the volumetric noise (rrt_params.noise_table): hash31 (math_utils.h:91-96) of
 *      every lattice point the low-octave noise3D calls of getAccretionDensity / getDustCloudDensity
 *      (densities.h:54, :95-128) can reach for t0 <= time <= t1, computed once on the device by the same
 *      arithmetic (a few milliseconds).  Caller-owned like the sky and tied to the device it was created on; any
 *      number of launches / streams of that device may read one table concurrently.  A launch whose `time` lies
 *      outside the window renders with the arithmetic kernels: same bytes, slower.
 *      Size: 0.49 GB for [0, 32 s] at full coverage.  A single dense box does not stay bounded as the window slides along
 *      the reference's unbounded simTime (main.cpp:515): the dust coordinates shear with time * (10/rc)^1.5
 *      (densities.h:88-93), so its z extent grows like 0.75 t0 + (t1 - t0); far along the clock the fine dust families
 *      therefore move to the BANDED layout (below), which keeps a 10 s window at t = 500 s at full coverage inside 2 GiB.
 *      Two more knobs: the window and the coverage -- which call families are table-served; the finest ones dominate the volume:
 *          RRT_TABLE_FULL      all table-served families
 *          RRT_TABLE_COARSE    without the 4.41 and 4.0 cells-per-unit dust families (about 1/9 of the dust box)
 *          RRT_TABLE_COARSEST  also without the 2.1 dust family and the finest accretion octave
 *      and rrt_noise_table_fit_window(), the policy the headless drivers use: longest window from t_from, richest
 *      coverage, within a byte budget (*bytes_out == 0: nothing fits, render without a table).
 *      rrt_noise_table_plan*() is host arithmetic only and returns the same RRT_ERR_INVALID_ARGUMENT as create for a
 *      box that cannot be addressed (>= 2^28 lattice points). ---- */
enum { RRT_TABLE_FULL = 0, RRT_TABLE_COARSE = 1, RRT_TABLE_COARSEST = 2,
       /* LAYOUT of the dust families (ABI 5), ORed into `coverage` to force one; neither = automatic.  DENSE: one box for all
        * of them -- what every window near the origin of the clock gets.  BANDED: the three fine families (ridge octaves 1 and
        * 2, the detail octave -- the ones that make the dense box unaddressable minutes into the clock) in one small box per
        * band of the angular rate omega = (10/rc)^1.5, picked per sample from its own radius: the shear of densities.h:88-93
        * only costs every band ITS OWN z range.  [495, 505 s] at full coverage: not addressable dense, ~1.5 GB banded.
        * Same bytes.  Automatic: dense unless it is unaddressable, or over 768 MB and larger than the banded plan.
        * rrt_noise_table_window() reports the layout a table got in this bit of its `coverage`. */
       RRT_TABLE_BANDED = 16, RRT_TABLE_DENSE = 32 };
int rrt_noise_table_create(float t_max, int* out_id);                                  /* = window [0, t_max], full coverage */
int rrt_noise_table_create_window(float t0, float t1, int coverage, int* out_id);
int rrt_noise_table_destroy(int id);
int rrt_noise_table_info(int id, float* t_max, size_t* bytes, int* boxes12);   /* boxes: x0,y0,z0,nx,ny,nz of the accretion and dust boxes */
int rrt_noise_table_window(int id, float* t0, float* t1, int* coverage, int* device);
int rrt_noise_table_plan(float t_max, size_t* bytes, int* boxes12);
int rrt_noise_table_plan_window(float t0, float t1, int coverage, size_t* bytes, int* boxes12);
/* the layout such a table gets (host arithmetic): *banded = 0 / 1; for a banded one the number of omega bands, the rule
 * band = clamp((int)((omega - w_min) * w_scale)), the box (x0, y0, z0, nx, ny, nz) of every (family, band) -- family 0 / 1 / 2
 * = ridge octave 1 / ridge octave 2 / detail octave, band_boxes[(family * cap_bands + band) * 6 ...], cap_bands >= n_bands
 * (64 always is) -- and of the four accretion octaves (acc_octave_boxes[24]).  Either array may be NULL. */
int rrt_noise_table_plan_layout(float t0, float t1, int coverage, int* banded, int* n_bands, float* w_min, float* w_scale,
                                int32_t* band_boxes, int cap_bands, int32_t* acc_octave_boxes);
int rrt_noise_table_fit_window(float t_from, float t_until, size_t budget_bytes, float* t1_out, int* coverage_out, size_t* bytes_out);

/* Handles and devices: a sky, workspace or noise table belongs to the HIP device that was current when it was
 * created (a borrowed sky: the device that owns the pointer), and a launch or copy that names it under another
 * current device returns RRT_ERR_BAD_HANDLE.  (Tests drive those checks without a second GPU through
 * rrt_debug_fake_device, include/rrt_test.h.) */

/* The shader clock the chip HOLDS, measured on the device: one wavefront sleeps for `duration_us` (<= 2 000 000) on
 * `stream` and reads the shader-clock counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) at both ends;
 * d_counters2[0] / d_counters2[1] * 0.1 = GHz.  Launched on a second stream beside the frames of a measurement it says what
 * clock the roofline's peak should be priced at (bench.py: roofline.clock_ghz). */
int rrt_clock_probe(unsigned long long* d_counters2, unsigned duration_us, void* stream);

/* ---- parameters of the reference-signature entry point launch_raymarch() (include/raymarcher.h), which has
 *      no argument for them: spin, max_steps, volumetrics, a workspace, a noise table ...  NULL restores the
 *      config.h defaults.  Nothing is allocated on the caller's behalf: objects named here are the caller's. ---- */
int rrt_set_launch_defaults(const rrt_params* prm);
/* ---- ... or, in ONE call, let the library own them (round 6).  For a host that makes only the drop-in edits and keeps calling
 *      launch_raymarch(): rrt_launch_auto_resources(1, base, table_budget_bytes, pool_bytes) creates ON THE CURRENT DEVICE a pool
 *      (pool_bytes; 0: none), a tile order and -- lazily, at the first launch -- lattice-hash tables over a window of `time` that fits
 *      table_budget_bytes (0: none), and every launch_raymarch() under that device then runs with `base` (NULL: config.h; its
 *      spin, max_steps, arith_mode ... are kept, its object fields replaced) + those objects: same bytes, the full speed of the
 *      path.  THE DOCUMENTED EXCEPTION to "a launch allocates nothing": the launch_raymarch() call whose `time` has left the table's
 *      window (the reference's simTime grows without bound, main.cpp:515) waits for the device, destroys the table and builds the
 *      next window (milliseconds) before it launches.  Calls under another current device use the plain defaults above.
 *      rrt_launch_auto_resources(0, NULL, 0, 0), from the same device, destroys everything.  Explicit rrt_launch_raymarch*()
 *      calls are never affected. ---- */
int rrt_launch_auto_resources(int on, const rrt_params* base, size_t table_budget_bytes, size_t pool_bytes);
int rrt_launch_auto_resources_info(int* on, int* table_builds, float* table_t0, float* table_t1, size_t* table_bytes);   /* any pointer may be NULL */
int rrt_get_launch_defaults_sized(void* out, uint32_t size);        /* through the macro: size = the caller's sizeof(rrt_params) */
#define rrt_get_launch_defaults(out) rrt_get_launch_defaults_sized((out), (uint32_t)sizeof(rrt_params))
/* launch_raymarch() with plain C types (what both C++ symbols of that name forward to): cam12 = pos, forward,
 * right, up; effects36 = the 36 bytes of struct CameraEffects (== rrt_effects); null stream, asynchronous. */
int rrt_launch_raymarch_compat(void* d_out_rgba8, int width, int height, float time, const float* cam12,
                               rrt_sky_t sky, const void* effects36);

/* ---- the hot path.  Replaces launch_raymarch, reference include/raymarcher.h:19 /
 *      src/raymarcher.cu:176-180.  Writes width*height RGBA8 pixels, alpha 255,
 *      bottom-up rows, to d_out_rgba8.  prm == NULL -> config.h defaults.
 *      Size limits (RRT_ERR_INVALID_ARGUMENT beyond them): width*height < 2^31 pixels, height <= 524 280
 *      (65 535 row-blocks of 8 rows, HIP's gridDim.y; the reference's 16x16 launch stops at 1 048 560). ---- */
int rrt_launch_raymarch(void* d_out_rgba8, int width, int height, float time,
                        const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                        const rrt_params* prm, void* stream);

/* Row-range variant for sharding the image plane (no counterpart in the
 * reference, which is single-GPU): renders image rows y0 <= y < y1 (y as in
 * raymarcher.cu:17, i.e. before the bottom-up flip) of the full width x height
 * frame.  d_out_rows receives (y1-y0)*width pixels; local row k holds image
 * row y1-1-k, so concatenating the shards in DESCENDING y order reproduces the
 * full bottom-up frame. */
int rrt_launch_raymarch_rows(void* d_out_rows, int width, int height, int y0, int y1, float time,
                             const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                             const rrt_params* prm, void* stream);

/* Interleaved row-tile variant: tile t = image rows [t*tile_rows, (t+1)*tile_rows)
 * belongs to shard (t mod n_shards).  Renders all tiles of `shard` into
 * d_out_tiles, tile-major in increasing t, each tile stored bottom-up like
 * rrt_launch_raymarch_rows.  rrt_tile_shard_rows() gives the buffer's rows (x width x 4 bytes). */
int rrt_launch_raymarch_tiles(void* d_out_tiles, int width, int height, int tile_rows,
                              int shard, int n_shards, float time,
                              const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                              const rrt_params* prm, void* stream);
int rrt_tile_shard_rows(int height, int tile_rows, int shard, int n_shards, int* rows);
/* Scatter one shard's tile buffer into a full bottom-up frame (device to device). */
int rrt_assemble_tiles(void* d_frame_rgba8, const void* d_tiles, int width, int height,
                       int tile_rows, int shard, int n_shards, void* stream);

/* Same for ALL shards in one launch: shard s's buffer starts at d_tiles_all + s*shard_stride_bytes
 * (the layout a gather into one allocation produces). */
int rrt_assemble_all_tiles(void* d_frame_rgba8, const void* d_tiles_all, size_t shard_stride_bytes,
                           int width, int height, int tile_rows, int n_shards, void* stream);

/* ---- cost-weighted tile -> shard assignment ("cost-model-weighted assignment"; the reference is
 *      single-GPU).  The rows through the hole and the disk cost several times the sky rows; t mod n_shards evens that
 *      out to ~9 % at 8 shards of a 4K frame, a map dealt by COST to ~1 %.  rrt_probe_tile_costs() estimates every row
 *      tile's cost from a coarse march-only probe of the view (deterministic: every rank computes the same numbers from
 *      the same camera, so no exchange is needed), rrt_tile_map_balance() deals the tiles longest-first to the least
 *      loaded shard (host arithmetic), rrt_tile_map_create() makes the assignment a device-resident object, and the
 *      two entry points below are rrt_launch_raymarch_tiles / rrt_assemble_all_tiles for such a map.  Buffer layout:
 *      a shard's tiles in increasing t, tile-major, each tile bottom-up. ---- */
int rrt_tile_map_create(int height, int tile_rows, int n_shards, const int32_t* shard_of_tile, int* out_id);
int rrt_tile_map_destroy(int id);
int rrt_tile_map_shard_rows(int id, int shard, int* rows, int* max_rows);      /* rows of `shard`'s buffer; of the largest */
int rrt_tile_map_balance(int n_tiles, const float* tile_cost, int n_shards, int max_tiles_per_shard, int32_t* shard_of_tile_out);
int rrt_probe_tile_costs(int width, int height, int tile_rows, float time, const rrt_camera* cam, const rrt_effects* fx,
                         const rrt_params* prm, float* tile_cost_host, int n_tiles, void* stream);
int rrt_launch_raymarch_tilemap(void* d_out_tiles, int width, int height, int tile_map, int shard, float time,
                                const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                                const rrt_params* prm, void* stream);
int rrt_assemble_all_tilemap(void* d_frame_rgba8, const void* d_tiles_all, size_t shard_stride_bytes,
                             int width, int height, int tile_map, void* stream);

/* Full-frame launch that also fills per-ray debug outputs (parity tests). */
int rrt_launch_raymarch_ex(void* d_out_rgba8, int width, int height, float time,
                           const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                           const rrt_params* prm, const rrt_debug_outputs* dbg, void* stream);

/* ---- s x s supersampled (anti-aliased) frames, s = samples_per_axis in {1, 2, 4, 8}; no counterpart in the reference, which
 *      casts one ray per pixel at the pixel's corner (raymarcher.cu:20).  The frame is DEFINED by the 1x frame of
 *      (s*width) x (s*height):
 *        - output pixel (x, y) has sub-samples (i, j), 0 <= i, j < s; sub-sample (i, j) is rendered exactly like pixel
 *          (s*x + i, s*y + j) of the (s*width) x (s*height) frame -- primary ray, lens distortion, the nudge hash
 *          (rrt_params.nudge_ulps) on those coordinates, march, sky, bloom and the vignette at that sub-sample's uv.  The grid is
 *          corner-aligned: it tiles the pixel's footprint [x, x+1) x [y, y+1), so the image sits (s-1)/(2s) px right of and
 *          below the 1x frame's.  (float)(s*w)/(float)(s*h) == (float)w/(float)h: the aspect ratio is unchanged;
 *        - the pixel's HDR value is the mean of its s^2 sub-samples' post-FX HDR (what rrt_debug_outputs.d_hdr holds for them
 *          in the big frame), summed in THIS order: a pairwise tree over i within each sub-row j in natural order (s = 4:
 *          ((h0 + h1) + (h2 + h3))), then the same tree over the s row sums; then multiplied by 1/(s*s), which is exact;
 *        - that mean is tone-mapped once as raymarcher.cu:164-173 does and stored as RGBA8, bottom-up rows.
 *      s = 1 gives the bytes of rrt_launch_raymarch.  d_hdr_rgba32f (may be NULL): the mean HDR, 4 floats per pixel (alpha 1),
 *      indexed like the RGBA8 frame -- linear frames for compositing.
 *      rrt_params: spin, max_steps, volumetrics, sky_frac_bits, arith_mode, noise_table, nudge_ulps / nudge_seed are honoured;
 *      workspace, path_policy, pool_rounds, pass_chains and tile_order are IGNORED -- a supersampled launch is always the single
 *      kernel in the static dispatch order.  Size limits (RRT_ERR_INVALID_ARGUMENT): those of rrt_launch_raymarch for width x
 *      height, and for the virtual frame (s*width)*(s*height) < 2^31, s*height <= 524 280.  No memset, no synchronisation: a
 *      launch can be captured into a hipGraph. ---- */
int rrt_launch_raymarch_ss(void* d_out_rgba8, float* d_hdr_rgba32f /* may be NULL */, int width, int height, int samples_per_axis,
                           float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream);
/* The same frame's row tiles of `shard` (tile t = OUTPUT rows [t*tile_rows, (t+1)*tile_rows) belongs to shard t mod n_shards), in
 * exactly the buffer layout of rrt_launch_raymarch_tiles: rrt_tile_shard_rows and rrt_assemble_(all_)tiles serve it unchanged. */
int rrt_launch_raymarch_ss_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard, int n_shards,
                                 float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream);

/* ---- motion-blurred frames: K = n_times in {1, 2, 4, 8, 16} shutter-time sub-frames, each s x s supersampled (s in {1, 2, 4, 8});
 *      no counterpart in the reference, whose every frame is one instant.  times[k] and cams[k] (k < n_times) are HOST arrays, read
 *      during the call.  The frame is DEFINED by rrt_launch_raymarch_ss:
 *        - sub-frame k's sum T_k is exactly the sum rrt_launch_raymarch_ss(width, height, s, times[k], &cams[k], ...) forms before it
 *          scales: the pairwise sub-row / row-sum tree over the post-FX HDR of the (s*width) x (s*height) frame rendered at
 *          (times[k], cams[k]) -- same nudge hash, lens, bloom, vignette and CA;
 *        - the pixel's HDR value is tree(T_0 ... T_{K-1}) * (1 / (s*s*K)), tree the same pairwise tree in natural k order
 *          (((T0 + T1) + (T2 + T3)) ...), the scale a power of two (exact); tone-mapped once, stored as RGBA8, bottom-up rows.
 *      Hence K = 1 gives the bytes of rrt_launch_raymarch_ss, K equal (time, camera) pairs the bytes of K = 1, and s = 1, K = 1 the
 *      bytes of rrt_launch_raymarch.  d_hdr_rgba32f (may be NULL): the mean HDR as in rrt_launch_raymarch_ss.
 *      The noise table (rrt_params.noise_table) is used only if EVERY times[k] lies in its window; otherwise every sub-frame hashes
 *      arithmetically (same bytes).  Params honoured and ignored as in rrt_launch_raymarch_ss: a blurred launch is always the single
 *      kernel in the static order.  RRT_ERR_INVALID_ARGUMENT, before any device call: everything rrt_launch_raymarch_ss refuses,
 *      n_times outside the set, a NULL times or cams, a non-finite time.  No memset, no synchronisation: a launch can be captured
 *      into a hipGraph. ---- */
int rrt_launch_raymarch_mb(void* d_out_rgba8, float* d_hdr_rgba32f /* may be NULL */, int width, int height, int samples_per_axis,
                           int n_times, const float* times, const rrt_camera* cams, rrt_sky_t sky, const rrt_effects* fx,
                           const rrt_params* prm, void* stream);
/* The same frame's row tiles of `shard`, in the buffer layout of rrt_launch_raymarch_ss_tiles (rrt_assemble_(all_)tiles serve it). */
int rrt_launch_raymarch_mb_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard, int n_shards,
                                 int n_times, const float* times, const rrt_camera* cams, rrt_sky_t sky, const rrt_effects* fx,
                                 const rrt_params* prm, void* stream);

/* ---- HDR glow: a soft-knee bright pass spread by L separable Gaussian lobes and added back onto a frame's HDR, tone-mapped; no
 *      counterpart in the reference, whose "bloom" (rrt_effects.use_bloom, post_processing.h:27-31) only brightens a pixel above a
 *      threshold and never reaches its neighbours.  That effect is unchanged and runs inside the march, before the glow.
 *      H is the w x h float4 frame rrt_launch_raymarch_ss / _mb write to d_hdr_rgba32f (bottom-up rows; rgb read).  Every
 *      operation is binary32, uncontracted, no flush to zero:
 *        1. bright pass: luma = (r*0.2126f + g*0.7152f) + b*0.0722f; luma > T: f = (luma - T) / luma, B = (r*f, g*f, b*f);
 *           otherwise B = 0 (a soft knee);
 *        2. lobe l < L: sigma_l = ((double)radius * height) * 2^l output pixels (radius is a fraction of the frame height),
 *           R_l = ceil(3 sigma_l), taps w_l[k + R_l] = exp(-k^2 / (2 sigma_l^2)) / sum_j exp(-j^2 / (2 sigma_l^2)) for
 *           |k| <= R_l, in double with the sum over ascending j, rounded to float (rrt_glow_weights returns them);
 *        3. per lobe a horizontal pass over B, then a vertical pass over its result, giving V_l: acc = 0.0f, then for
 *           k = -R_l ... R_l ascending acc = acc + w_l[k + R_l] * X[clamp(i + k)], i the column, then the STORED row index
 *           (bottom-up), clamped to the frame's edge;
 *        4. G = V_0, G = G + V_l for l = 1 ... L-1; s = intensity / (float)L; out = H + G * s per channel, tone-mapped as
 *           raymarcher.cu:164-173 and stored as RGBA8 in H's layout.
 *      So intensity = 0, or a threshold above every luma, gives the bytes the _ss / _mb launch wrote with H. */
typedef struct rrt_glow {
    uint32_t struct_size;    /* sizeof(rrt_glow): rrt_glow_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    float radius;            /* sigma_0 as a fraction of the frame height, > 0 and finite */
    int32_t lobes;           /* L in {1, 2, 3, 4} */
    float threshold;         /* T >= 0 and finite */
    float intensity;         /* >= 0 and finite */
} rrt_glow;
/* radius 0.004, lobes 4, threshold 1.0, intensity 0.25: a look, not a measurement */
int rrt_glow_default(rrt_glow* g);
/* lobe `lobe`'s taps for a frame `height` rows high: R_l in *radius_out (may be NULL) and, if out is not NULL, its 2 R_l + 1
 * weights (cap >= 2 R_l + 1).  Host only. */
int rrt_glow_weights(const rrt_glow* g, int height, int lobe, float* out, int cap, int* radius_out);
/* the bytes of the caller-owned scratch rrt_launch_glow needs for a width x height frame.  Host only. */
int rrt_glow_scratch_bytes(int width, int height, const rrt_glow* g, size_t* bytes);
/* The glowed RGBA8 frame of H into d_out_rgba8 (width*height*4 bytes; it may not overlap H or the scratch).  The library
 * allocates nothing: d_scratch (>= rrt_glow_scratch_bytes) belongs to the caller; no memset, no synchronisation, so _ss / _mb
 * followed by this launch can be captured into a hipGraph.  RRT_ERR_INVALID_ARGUMENT, before any device call: NULL pointers,
 * d_hdr_rgba32f or d_scratch not 16-byte aligned, width or height <= 0, width*height >= 2^31, lobes outside {1 ... 4}, a radius
 * <= 0, a threshold or intensity < 0, any of them not finite, a widest R_{L-1} > 1024, scratch_bytes below the query's;
 * RRT_ERR_ABI_MISMATCH for another struct_size.  Full frames only: no _tiles form. */
int rrt_launch_glow(void* d_out_rgba8, const float* d_hdr_rgba32f, int width, int height, const rrt_glow* g, void* d_scratch,
                    size_t scratch_bytes, void* stream);

/* ---- panoramas: 360-degree equirectangular and angular-fisheye (dome master) frames; no counterpart in the reference, whose one
 *      camera is the pinhole of raymarcher.cu:20-34.  The frame is DEFINED as rrt_launch_raymarch_ss's: sub-sample (i, j) of output
 *      pixel (x, y) is pixel (s*x + i, s*y + j) of the W x H = (s*width) x (s*height) panorama, the pixel's HDR is the same pairwise
 *      sub-row / row-sum tree times 1/(s*s), tone-mapped once, bottom-up rows; d_hdr_rgba32f (may be NULL) receives the mean HDR.
 *      The primary ray of virtual pixel (x, y), with fw, rt, up, pos from cam, every operation binary32, uncontracted, division and
 *      square root correctly rounded, the same in all three arithmetic modes (the mode changes only the march):
 *        - half-angles in radians, on the host: a_h = (float)((double)fov_deg * 3.14159265358979323846 / 360.0), a_v the same of
 *          vfov_deg, a = a_h;
 *        - EQUIRECT: lon = (((float)x + 0.5f) / (float)W * 2.0f - 1.0f) * a_h, lat = (((float)y + 0.5f) / (float)H * 2.0f - 1.0f) * a_v;
 *          (s_lat, c_lat) and (s_lon, c_lon) from rrt_sincosf (csrc/rrt_math.h);
 *          D = fw*(c_lat*c_lon) + (rt*(c_lat*s_lon) + up*s_lat), per component in that association.  The centre column looks
 *          along fw, +x turns toward rt, +y toward up, as in the pinhole frame;
 *        - FISHEYE (angular, equidistant): u = (2.0f*((float)x + 0.5f) - (float)W) / (float)H, v = (2.0f*((float)y + 0.5f) - (float)H)
 *          / (float)H, r2 = u*u + v*v; r2 > 1.0f: the sub-sample is OUTSIDE the disc.  Otherwise r = sqrt(r2), (s_t, c_t) =
 *          rrt_sincosf(r * a), k = r > 0 ? s_t / r : 0.0f, D = fw*c_t + (rt*(u*k) + up*(v*k));
 *        - vel = normalize(D) (raymarcher.cu's: 1e-6f guard), then the nudge hash (rrt_params.nudge_ulps) on the virtual (x, y)
 *          exactly as the pinhole's; the march starts at pos.
 *      An outside sub-sample's post-FX HDR is exactly (0, 0, 0): no march, no sky, no bloom; it still enters its pixel's tree, which
 *      antialiases the disc's rim.  Bloom and chromatic aberration act per ray and are honoured; use_lens_distortion and use_vignette
 *      are IGNORED (both are defined on the pinhole's uv).  rrt_params honoured and ignored as in rrt_launch_raymarch_ss (noise table
 *      included): a panorama is always the single kernel in the static order.  kind RRT_PROJ_PINHOLE makes the call
 *      rrt_launch_raymarch_ss (same bytes; spans ignored).  RRT_ERR_INVALID_ARGUMENT, before any device call: everything
 *      rrt_launch_raymarch_ss refuses, a NULL proj, an unknown kind, a span outside its range or not finite; RRT_ERR_ABI_MISMATCH for
 *      another struct_size.  No memset, no synchronisation: a launch can be captured into a hipGraph. ---- */
#define RRT_PROJ_PINHOLE 0      /* the reference's camera: the call IS rrt_launch_raymarch_ss, same bytes */
#define RRT_PROJ_EQUIRECT 1
#define RRT_PROJ_FISHEYE 2
typedef struct rrt_projection {
    uint32_t struct_size;   /* sizeof(rrt_projection): rrt_projection_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    int32_t kind;           /* RRT_PROJ_* */
    float fov_deg;          /* equirect: horizontal span, (0, 360], default 360; fisheye: aperture, (0, 360], default 180; pinhole: ignored (0) */
    float vfov_deg;         /* equirect: vertical span, (0, 180], default 180; fisheye and pinhole: ignored (0) */
} rrt_projection;
int rrt_projection_default(int kind, rrt_projection* p);
/* Host only: the unit direction vel of virtual pixel (x, y) of a width x height frame, before any nudge, from the same source the
 * kernel runs; *inside_out (may be NULL) = 0 and a zero dir_out for a fisheye sub-sample outside the disc, 1 otherwise.
 * RRT_PROJ_PINHOLE: raymarcher.cu:20-34's direction without the lens.  Maps a pixel to a sky direction (overlays).
 * RRT_ERR_INVALID_ARGUMENT: the projection's refusals, NULL cam or dir_out, width or height <= 0, (x, y) outside the frame. */
int rrt_projection_ray(const rrt_projection* p, int width, int height, int x, int y, const rrt_camera* cam,
                       float dir_out[3], int* inside_out);
int rrt_launch_raymarch_pano(void* d_out_rgba8, float* d_hdr_rgba32f /* may be NULL */, int width, int height,
                             int samples_per_axis, const rrt_projection* proj, float time, const rrt_camera* cam,
                             rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream);
/* The same primary rays on the device, for GPU-side overlays and compositing: every pixel (x, y) of a width x height frame as a
 * float4 (vel before any nudge, 1 inside / 0 outside the fisheye disc) -- the bits rrt_projection_ray returns for it -- in the
 * frame's layout (bottom-up rows: pixel (x, y) at index (height - 1 - y) * width + x).  A supersampled frame's sub-samples are the
 * pixels of the (s*width) x (s*height) map.  RRT_ERR_INVALID_ARGUMENT, before any device call: the projection's refusals, NULL
 * d_dir_rgba32f or cam, d_dir_rgba32f not 16-byte aligned, width or height <= 0, width*height >= 2^31.  Graph-capturable. */
int rrt_launch_projection_map(void* d_dir_rgba32f, int width, int height, const rrt_projection* proj, const rrt_camera* cam,
                              void* stream);
/* The same frame's row tiles of `shard`, in the buffer layout of rrt_launch_raymarch_ss_tiles (rrt_assemble_(all_)tiles serve it). */
int rrt_launch_raymarch_pano_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows,
                                   int shard, int n_shards, const rrt_projection* proj, float time,
                                   const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                                   const rrt_params* prm, void* stream);

/* ---- adaptive supersampling: the 1x frame, with only the pixels that alias replaced by their s x s supersampled values; no
 *      counterpart in the reference.  An s x s frame costs s^2 frames, and almost all of it lands on pixels that do not alias; the
 *      aliasing sits on thin curves (photon ring, shadow edge, the disk's rim, ridge noise, stars).  For a width x height frame,
 *      s = samples_per_axis in {1, 2, 4, 8} and a threshold T in [0, 255] the frame is DEFINED by two frames of the same arguments:
 *        1. base: base8 and baseH are the RGBA8 and mean-HDR frames of rrt_launch_raymarch_ss(..., s = 1, ...) -- with a proj
 *           whose kind is not RRT_PROJ_PINHOLE, of rrt_launch_raymarch_pano(..., s = 1, ...);
 *        2. mask: on the STORED base8 in integer arithmetic, alpha ignored: pixel p is REFINED iff for one of its four edge
 *           neighbours q (left, right, up, down; coordinates clamped at the frame's edge, NO horizontal wrap, equirect frames
 *           included) max over c in {r, g, b} of |base8[p][c] - base8[q][c]| > T.  The rule is symmetric, so both sides of an edge are
 *           refined; T = 255 refines nothing;
 *        3. frame: a refined pixel's bytes and HDR are exactly those of the same pixel in the s x s frame of the same launch
 *           arguments (rrt_launch_raymarch_ss, or _pano): the same virtual grid, the nudge hash on virtual coordinates, the same
 *           pairwise tree, 1/(s*s) and one tone map.  Every other pixel keeps base8 and baseH.  out = where(mask, ss, base), byte
 *           for byte and bit for bit; s = 1 is the base frame at any T.
 *      The refined pixels carry the supersampled frame's (s-1)/(2s) px corner-aligned offset (rrt_launch_raymarch_ss) and the others
 *      do not: the two grids differ by less than half a pixel, which is invisible where the picture is flat -- and the picture is
 *      flat, to T, wherever a pixel is not refined.
 *      The launch is base pass -> zero -> mask -> refine on the caller's stream: the mask pass compacts the refined pixels' frame
 *      indices into the caller's scratch (ballot / popcount per wavefront, one atomic add per wavefront), the refine pass packs
 *      them into full wavefronts -- a wave is an 8x8 tile of virtual samples, (8/s)^2 pixels -- and overwrites d_out_rgba8 and
 *      d_hdr_rgba32f in place.  The host never learns the count: no synchronisation, no allocation, no memset; a launch can be
 *      captured into a hipGraph as a linear chain.
 *      d_scratch: rrt_adaptive_scratch_bytes(width, height) bytes or more, 16-byte aligned, the caller's.  Layout once the launch
 *      has run: the uint32 at offset 0 is the count of refined pixels; from offset 16 on, that many uint32 frame indices (stored row
 *      * width + x: the RGBA8 frame's own pixel index) in unspecified order.  A caller reads the count with its own 4-byte copy.
 *      rrt_params honoured and ignored as in rrt_launch_raymarch_ss: single kernel, static order, no march cache.
 *      RRT_ERR_INVALID_ARGUMENT, before any device call: everything rrt_launch_raymarch_ss (proj NULL) or rrt_launch_raymarch_pano
 *      (proj given) refuses for the s x s frame, a NULL ad, d_scratch or d_out_rgba8, a threshold outside [0, 255], a scratch that is
 *      too small or not 16-byte aligned; RRT_ERR_ABI_MISMATCH for another struct_size.  Full frames only: no _tiles form (the mask
 *      needs the neighbouring rows across tile seams). ---- */
typedef struct rrt_adaptive {
    uint32_t struct_size;    /* sizeof(rrt_adaptive): rrt_adaptive_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    int32_t threshold;       /* T in [0, 255], in steps of the stored 8-bit channels */
} rrt_adaptive;
/* threshold 8: a look, not a measurement */
int rrt_adaptive_default(rrt_adaptive* ad);
/* the bytes of the caller-owned scratch rrt_launch_raymarch_adaptive needs for a width x height frame: 16 + 4 width height, rounded
 * up to 16.  Host only.  RRT_ERR_INVALID_ARGUMENT: NULL bytes, width or height <= 0, width*height >= 2^31. */
int rrt_adaptive_scratch_bytes(int width, int height, size_t* bytes);
/* Host only: the mask of a stored RGBA8 frame in HOST memory, from the source the mask pass runs: mask_out[i] = 1 if pixel i is
 * refined, else 0, in the frame's layout; *count_out (may be NULL) their number.  The launch's refusals of ad, NULL rgba8_host or
 * mask_out, the frame sizes rrt_adaptive_scratch_bytes refuses. */
int rrt_adaptive_mask(const uint8_t* rgba8_host, int width, int height, const rrt_adaptive* ad, uint8_t* mask_out, uint32_t* count_out);
int rrt_launch_raymarch_adaptive(void* d_out_rgba8, float* d_hdr_rgba32f /* may be NULL */, int width, int height,
                                 int samples_per_axis, const rrt_projection* proj /* NULL = pinhole */, const rrt_adaptive* ad,
                                 float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm,
                                 void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- stereo frames: omni-directional stereo (ODS) equirect pairs for headsets and off-axis pinhole pairs for 3D displays; no
 *      counterpart in the reference.  width and height are PER EYE; the frame written is one RGBA8 composite of both eyes:
 *        - RRT_STEREO_TOP_BOTTOM: width x 2 height; as displayed the left eye is on top, so with the usual bottom-up rows buffer
 *          rows 0 ... height-1 hold the RIGHT eye and rows height ... 2 height-1 the left;
 *        - RRT_STEREO_SIDE_BY_SIDE: 2 width x height, the left eye in columns 0 ... width-1.
 *      Each eye's half is DEFINED as the mono frame of width x height -- rrt_launch_raymarch_ss's for RRT_PROJ_PINHOLE,
 *      rrt_launch_raymarch_pano's for RRT_PROJ_EQUIRECT: the same virtual (s*width) x (s*height) grid, pairwise tree, 1/(s*s) and one
 *      tone map; the EYE-LOCAL virtual pixel (x, y) feeds everything that depends on the pixel (projection, lens, vignette uv, the
 *      nudge hash).  Only the primary ray changes: its origin and, for the pinhole, a shift of u.  Every operation binary32,
 *      uncontracted, in the association written, the same in all three arithmetic modes; fw, rt, up, pos from cam:
 *        - on the host: hb = (float)(0.5 * (double)base); e = -1 for the left eye, +1 for the right;
 *        - EQUIRECT (ODS): the direction is rrt_launch_raymarch_pano's, bit for bit (lat, s_lon, c_lon its own values).  from and to
 *          in radians, on the host: (float)((double)deg * 3.14159265358979323846 / 180.0).  a = fabsf(lat); f = 1 if a <= from, else
 *          0 if a >= to, else (to - a) / (to - from); k = f * hb, negated for the left eye.  R_i = rt_i * c_lon - fw_i * s_lon (the
 *          column's horizontal right-hand vector); origin_i = pos_i + R_i * k: every column looks from its own point on a circle of
 *          radius hb, tangent to its viewing direction.  Lens and vignette are ignored, as in rrt_launch_raymarch_pano;
 *        - PINHOLE (off-axis): origin_i = pos_i + rt_i * k with k = e*hb; the direction is the pinhole's primary ray on the eye's
 *          frame (raymarcher.cu:20-34, the lens included) with u_coord = u_coord - c between u_coord *= aspect and forming D;
 *          c = k / convergence, per eye on the host, 0 when convergence == 0 (parallel axes).  The eyes' rays cross convergence
 *          units in front of the camera: the zero-parallax plane;
 *        - zero rule: k == 0 (either sign) leaves the origin at pos with no addition, c == 0 leaves u_coord untouched.  So base = 0
 *          gives each half the bytes of the mono frame, even for a signed-zero pos.
 *      Bloom and chromatic aberration act per ray.  rrt_params honoured and ignored as in rrt_launch_raymarch_ss: a stereo launch is
 *      always the single kernel in the static order.  d_hdr_rgba32f (may be NULL): the mean HDR in the composite's layout.
 *      RRT_ERR_INVALID_ARGUMENT, before any device call: everything rrt_launch_raymarch_ss refuses for the COMPOSITE frame (its
 *      virtual frame: (s*W)*(s*H) < 2^31, s*H <= 524 280 for W x H the composite), a NULL proj or st, the projection's refusals, a
 *      fisheye (no stereo domes), an unknown layout, a negative or non-finite base or convergence, merge angles not
 *      0 <= from <= to <= 90; RRT_ERR_ABI_MISMATCH for another struct_size of either struct.  No memset, no synchronisation: a
 *      launch can be captured into a hipGraph. ---- */
#define RRT_STEREO_TOP_BOTTOM 1     /* width x 2 height, left eye on top as displayed (buffer rows height ... 2 height-1) */
#define RRT_STEREO_SIDE_BY_SIDE 2   /* 2 width x height, left eye on the left */
#define RRT_EYE_LEFT 0
#define RRT_EYE_RIGHT 1
typedef struct rrt_stereo {
    uint32_t struct_size;        /* sizeof(rrt_stereo): rrt_stereo_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    int32_t layout;              /* RRT_STEREO_* */
    float base;                  /* interaxial distance in scene units, >= 0 and finite */
    float convergence;           /* pinhole: zero-parallax distance along forward, >= 0 (0 = parallel axes); equirect: finite >= 0, ignored */
    float pole_merge_from_deg;   /* equirect: 0 <= from <= to <= 90; the eye separation fades linearly to 0 between the two */
    float pole_merge_to_deg;     /*   latitudes (90, 90 = no fade); pinhole: checked, ignored */
} rrt_stereo;
/* base 1.0, convergence 0, pole merge 90 / 90: a look, not a measurement */
int rrt_stereo_default(int layout, rrt_stereo* st);
/* Host only: the primary ray of eye `eye`'s virtual pixel (x, y) of a width x height eye frame, before any nudge, from the source
 * the kernel runs: origin_out, the unit direction dir_out, *inside_out (may be NULL) = 1.  The pinhole's direction is without the
 * lens, as rrt_projection_ray's.  RRT_ERR_INVALID_ARGUMENT: the launch's refusals of proj and st, NULL cam, origin_out or dir_out,
 * width or height <= 0, (x, y) outside the eye's frame, eye not RRT_EYE_*. */
int rrt_stereo_ray(const rrt_projection* p, const rrt_stereo* st, int width, int height, int eye, int x, int y,
                   const rrt_camera* cam, float origin_out[3], float dir_out[3], int* inside_out);
int rrt_launch_raymarch_stereo(void* d_out_rgba8, float* d_hdr_rgba32f /* may be NULL */, int width, int height,
                               int samples_per_axis, const rrt_projection* proj, const rrt_stereo* st, float time,
                               const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream);
/* The composite's row tiles of `shard` (tile t = the composite's OUTPUT rows [t*tile_rows, (t+1)*tile_rows)), in the buffer layout
 * of rrt_launch_raymarch_ss_tiles: rrt_tile_shard_rows and rrt_assemble_(all_)tiles serve it unchanged, given the composite's
 * width and height. */
int rrt_launch_raymarch_stereo_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows,
                                     int shard, int n_shards, const rrt_projection* proj, const rrt_stereo* st, float time,
                                     const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm,
                                     void* stream);

/* ---- depth of field: K = n_samples in {1, 2, 4, 8, 16} rays per sub-sample through points of a thin lens focused at `focus`, each
 *      s x s supersampled (s in {1, 2, 4, 8}); no counterpart in the reference, whose camera is a pinhole.  times[k], cams[k] and
 *      the lens point (lx, ly) = (lens_xy[2k], lens_xy[2k+1]) of sample k (k < n_samples) are HOST arrays, read during the call; a
 *      lens point is in scene units along cams[k].right and cams[k].up.  Every sample carries its own time and camera, so ONE
 *      launch gives a frame that is defocused and motion-blurred from the same K rays.  The frame is DEFINED by
 *      rrt_launch_raymarch_ss and rrt_launch_raymarch_mb:
 *        - sample k's ray for virtual pixel (x, y) of the (s*width) x (s*height) frame; every operation binary32, uncontracted, in
 *          the association written, the same in all three arithmetic modes; fw, rt, up, pos from cams[k]:
 *          on the host cx = lx / focus and cy = ly / focus.  The direction is the pinhole's primary ray (raymarcher.cu:20-34, the
 *          lens distortion included) with u_coord = u_coord - cx and v_coord = v_coord - cy between u_coord *= aspect and forming
 *          D = fw + (rt*u + up*v); then normalize, then the nudge hash on the virtual (x, y), as in rrt_launch_raymarch_ss.  The
 *          vignette reads the uv primary_ray returns (after the lens distortion, before the shift), as the stereo pinhole does.
 *          The origin is org = pos; if lx != 0: org_i = org_i + rt_i * lx; if ly != 0: org_i = org_i + up_i * ly.  In flat space
 *          the rays of all lens points through one pixel meet on the plane `focus` along forward: the plane in focus;
 *        - zero rule: a zero cx or cy (either sign) leaves its coordinate untouched, a zero lx or ly adds nothing;
 *        - T_k is the sum rrt_launch_raymarch_ss forms over that sample's (s*width) x (s*height) frame before it scales;
 *        - the pixel's HDR value is tree(T_0 ... T_{K-1}) * (1 / (s*s*K)), rrt_launch_raymarch_mb's pairwise tree in natural k
 *          order; tone-mapped once, stored as RGBA8, bottom-up rows.  d_hdr_rgba32f (may be NULL) as in rrt_launch_raymarch_ss.
 *      Hence: all lens points (0, 0) give the bytes and HDR bits of rrt_launch_raymarch_mb for the same times and cams at any
 *      focus > 0; K = 1 with a zero lens point is rrt_launch_raymarch_ss, with s = 1 as well rrt_launch_raymarch; K = 1 with the
 *      lens point (+-lx, 0) and focus Z is the right / left half of rrt_launch_raymarch_stereo's pinhole frame with base 2 lx (exact)
 *      and convergence Z; K equal samples are K = 1.
 *      The noise table is used only if EVERY times[k] lies in its window.  rrt_params honoured and ignored as in
 *      rrt_launch_raymarch_mb: the launch is the single kernel in the static order, and never reads or fills the march cache.
 *      RRT_ERR_INVALID_ARGUMENT, before any device call: everything rrt_launch_raymarch_mb refuses, a NULL lens_xy, a non-finite
 *      lens coordinate, a focus that is not finite or <= 0.  No memset, no allocation, no synchronisation: a launch can be captured
 *      into a hipGraph. ---- */
int rrt_launch_raymarch_dof(void* d_out_rgba8, float* d_hdr_rgba32f /* may be NULL */, int width, int height, int samples_per_axis,
                            int n_samples, const float* times, const rrt_camera* cams, const float* lens_xy /* 2 n_samples */,
                            float focus, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream);
/* The same frame's row tiles of `shard`, in the buffer layout of rrt_launch_raymarch_mb_tiles (rrt_assemble_(all_)tiles serve it). */
int rrt_launch_raymarch_dof_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard, int n_shards,
                                  int n_samples, const float* times, const rrt_camera* cams, const float* lens_xy /* 2 n_samples */,
                                  float focus, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream);
/* Host only: the primary ray of virtual pixel (x, y) of a width x height frame through the lens point (lx, ly), before any nudge
 * and without the lens distortion (as rrt_stereo_ray's pinhole), from the source the kernel runs: origin_out and the unit
 * direction dir_out.  RRT_ERR_INVALID_ARGUMENT: NULL cam, origin_out or dir_out, width or height <= 0, (x, y) outside the frame, a
 * non-finite lx or ly, a focus that is not finite or <= 0. */
int rrt_lens_ray(int width, int height, int x, int y, const rrt_camera* cam, float lx, float ly, float focus, float origin_out[3],
                 float dir_out[3]);
/* Host only, a helper and no part of any bit contract: n_samples lens points on a disc of radius `aperture`.  n_samples = 1 gives
 * (0, 0); otherwise Vogel's spiral in double, r = aperture * sqrt((k + 0.5) / n_samples), theta = rotation_rad + k pi (3 - sqrt 5),
 * (r cos theta, r sin theta) rounded to float.  RRT_ERR_INVALID_ARGUMENT: NULL xy_out, a negative or non-finite aperture, a
 * non-finite rotation, n_samples outside {1, 2, 4, 8, 16}. */
int rrt_lens_points(float aperture, int n_samples, float rotation_rad, float* xy_out /* 2 n_samples */);

/* ---- exposure control: a frame's linear HDR scaled by 2^ev before the tone map, ev given by the caller (manual) or metered from the
 *      frame and adapted over time on the device (auto); no counterpart in the reference, whose every frame is tone-mapped at the
 *      fixed EXPOSURE = 0.8f (raymarcher.cu:164-166).  That constant stays inside the tone map; this pass scales what goes into it.
 *      H is the w x h float4 frame the _ss / _mb / _dof / _pano / _stereo / _adaptive launches write to d_hdr_rgba32f (any layout:
 *      the pass works per pixel and meters the whole buffer).  The pass writes the scaled HDR (rrt_launch_glow's input), the
 *      tone-mapped RGBA8 frame, or both.  Every step is integer, binary32 or binary64 arithmetic in the order written, uncontracted:
 *        1. luma and bin: luma = (r*0.2126f + g*0.7152f) + b*0.0722f (the glow's); u = the bits of luma; the pixel is METERED iff
 *           0 < u < 0x7f800000, i.e. luma is positive and finite, subnormals included.  Zero (the hole's shadow, sub-samples outside a
 *           fisheye disc), negative, NaN and infinite lumas are not metered.  bin = clamp((int)(u >> 20) - 888, 0, 255): the float's 8
 *           exponent bits and top 3 mantissa bits, 256 bins over the 32 octaves [2^-16, 2^16), 8 per octave, linear inside an octave
 *           (888 = (127 - 16) * 8); darker and brighter lumas fall into bins 0 and 255.  c_b is the count of bin b: exact integers,
 *           whatever order the pixels are counted in;
 *        2. bin centres, in double on the host (rrt_exposure_bin_ev returns them; the device is handed the table):
 *           L_b = (e - 127) + log2(1 + (j + 0.5) / 8) with e = (b + 888) >> 3 and j = (b + 888) & 7;
 *        3. resolve: N = sum c_b (uint64); lo = N * low_permille / 1000 and hi = N * high_permille / 1000 (integer floor); remove lo
 *           counts from the lowest bins upwards and hi from the highest downwards, cutting bins partially: the retained counts are r_b,
 *           M = sum r_b >= 1; m = (sum over ascending b, from 0.0, of (double)r_b * L_b) / (double)M in binary64;
 *           target = clamp((float)(log2_key - m) + ev, min_ev, max_ev) with log2_key = log2((double)key) from the host, the sum in
 *           binary32, clamp(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x);
 *        4. state (caller-owned device memory, carried from frame to frame: S.ev, S.frames): if N == 0, S.ev is unchanged -- except
 *           on the first frame (S.frames == 0), where it becomes clamp(ev, min_ev, max_ev); else if S.frames == 0, S.ev = target; else
 *           alpha = target > S.ev ? adapt_up : adapt_down and S.ev = S.ev + (target - S.ev) * alpha in binary32, the multiply and
 *           then the add.  Then S.frames += 1 (it stops at 2^32 - 1);
 *        5. scale = rrt_expf(S.ev * 0.693147182f), the portable exp of csrc/rrt_math.h.  In manual mode there is no metering and no
 *           state: the host computes scale from the settings' ev with the same function.  rrt_expf(0) == 1.0f: EV 0 is the identity;
 *        6. apply: out.rgb = H.rgb * scale, out.a = H.a; the bytes are that value tone-mapped as raymarcher.cu:164-173 and stored
 *           as RGBA8 at H's pixel index.
 *      So manual EV 0 gives the bytes the launch that wrote H stored, and H's bits.
 *      Auto mode is zero -> meter -> resolve -> apply on the caller's stream, a linear chain; manual mode the apply pass alone.  No
 *      synchronisation, no allocation, no memset: a launch can be captured into a hipGraph, and a replay advances the state.
 *      d_scratch: rrt_exposure_scratch_bytes() bytes or more, 16-byte aligned, the caller's; rrt_launch_exposure_reset must have run
 *      on it once before the first auto launch (it zeroes the state and loads the table of L_b), and starts a sequence over.  Layout:
 *        offset RRT_EXPOSURE_HIST_OFFSET (0):      uint32 c_b[256], the last launch's histogram
 *        offset RRT_EXPOSURE_STATE_OFFSET (1024):  float S.ev; uint32 S.frames; float scale; float target; uint64 N; double m;
 *                                                  32 reserved bytes -- target, N and m are the last launch's (target and m read 0
 *                                                  when N == 0); a caller reads S.ev with its own 4-byte copy
 *        offset RRT_EXPOSURE_TABLE_OFFSET (1088):  double L_b[256] ---- */
#define RRT_EXPOSURE_MANUAL 0
#define RRT_EXPOSURE_AUTO 1
#define RRT_EXPOSURE_HIST_OFFSET 0
#define RRT_EXPOSURE_STATE_OFFSET 1024
#define RRT_EXPOSURE_TABLE_OFFSET 1088
typedef struct rrt_exposure {
    uint32_t struct_size;    /* sizeof(rrt_exposure): rrt_exposure_default sets it; any other value is RRT_ERR_ABI_MISMATCH */
    int32_t mode;            /* RRT_EXPOSURE_* */
    float ev;                /* manual: the EV; auto: the compensation added to the metered EV.  Finite */
    float key;               /* auto: the luminance the retained pixels' log-average is brought to, > 0 and finite */
    int32_t low_permille;    /* auto: the darkest and the brightest share of the metered pixels left out of the average, in 1/1000; */
    int32_t high_permille;   /*   each >= 0, their sum < 1000 */
    float min_ev, max_ev;    /* auto: the target's range, min_ev <= max_ev, both finite */
    float adapt_up;          /* auto: the share of the way to a HIGHER target (a darker frame) taken per frame, in (0, 1] */
    float adapt_down;        /* auto: the same towards a lower target (a brighter frame); rrt_exposure_adapt makes them from seconds */
} rrt_exposure;
/* manual, ev 0, key 0.5, 400 / 20 per mille, ev in [-8, 8], both adapt factors 1 (no smoothing): a look, not a measurement.  The low
 * cut is large because most of a typical frame is dark sky, which would otherwise pull the exposure up until the disk clips. */
int rrt_exposure_default(rrt_exposure* e);
/* bin `bin`'s centre L_b in log2 units, 0 <= bin < 256.  Host only. */
int rrt_exposure_bin_ev(int bin, double* ev_out);
/* the adapt factor of a time constant: *alpha_out = (float)(1 - exp(-dt / tau)), in double, for a frame interval dt and a time
 * constant tau in the same unit; tau == 0 gives 1.  Host only.  RRT_ERR_INVALID_ARGUMENT: a negative or non-finite dt or tau. */
int rrt_exposure_adapt(double dt, double tau, float* alpha_out);
/* the bytes of the caller-owned scratch of an auto launch (the layout above; it does not depend on the frame).  Host only. */
int rrt_exposure_scratch_bytes(size_t* bytes);
/* Host only: the histogram c_b of a w x h float4 frame in HOST memory, from the source the meter pass runs.
 * RRT_ERR_INVALID_ARGUMENT: NULL pointers, width or height <= 0, width*height >= 2^31. */
int rrt_exposure_meter_host(const float* hdr_rgba32f_host, int width, int height, uint32_t* hist_out /* 256 */);
/* zeroes the scratch's histogram and state and loads the table (one kernel).  RRT_ERR_INVALID_ARGUMENT, before any device call: a
 * NULL or not 16-byte aligned d_scratch, scratch_bytes below the query's. */
int rrt_launch_exposure_reset(void* d_scratch, size_t scratch_bytes, void* stream);
/* The exposed frame of d_hdr_in (width*height float4): its RGBA8 into d_out_rgba8 (may be NULL), its scaled HDR into d_hdr_out (may
 * be NULL; may be d_hdr_in itself: in place).  Manual mode accepts a NULL d_scratch.  RRT_ERR_INVALID_ARGUMENT, before any device
 * call: a NULL e or d_hdr_in, both outputs NULL, d_hdr_in or d_hdr_out not 16-byte aligned, d_out_rgba8 not 4-byte aligned, a
 * d_hdr_out that overlaps d_hdr_in without being equal to it, width or height <= 0, width*height >= 2^31, a setting outside the
 * range the struct states, and in auto mode a NULL, misaligned or too small d_scratch; RRT_ERR_ABI_MISMATCH for another
 * struct_size.  Full frames only: no _tiles form (the meter needs the whole frame). */
int rrt_launch_exposure(void* d_out_rgba8 /* may be NULL */, float* d_hdr_out /* may be NULL */, const float* d_hdr_in, int width,
                        int height, const rrt_exposure* e, void* d_scratch, size_t scratch_bytes, void* stream);

/* ---- which path a rank's share takes while several frames of a sequence are in flight (host only; no GPU call) ----
 * New in this repo (the reference renders one frame at a time on one GPU: src/main.cpp:505-529).  A launch of <= 1.5 M rays
 * with a pool can take the three-pass path (RRT_PATH_AUTO) or the single kernel (RRT_PATH_SINGLE); under frames in flight the
 * single kernel is 3-10 % faster unless the share holds a wavefront that outlasts them (then 20 % slower).  The object cuts the
 * sequence into windows, tries the other path for a few frames at a window's start, compares SUSTAINED frame times (the mean
 * interval between the ends of consecutive frames' renders on the rank) and keeps the faster; frames_in_flight single-kernel
 * frames in a row that take > 1.5 x the three-pass mean end the experiment at once (csrc/rrt_path_chooser.cpp).  The bytes do not
 * depend on it.
 *   id = create(frames_in_flight, window_frames (0: 48));  per frame k = 1, 2, ...: policy(id, k, &p) -> rrt_params.path_policy;
 *   later, when frame k's times are known: report(id, k, ms). */
typedef struct rrt_path_chooser_stats {
    int32_t incumbent;                 /* RRT_PATH_AUTO / RRT_PATH_SINGLE: what the current window renders with outside its trial */
    int32_t windows, trials, trials_aborted, switches, outliers;
    int32_t frames[2];                 /* frames handed to [0] the automatic (three-pass) path, [1] the single kernel */
    float last_three_pass_mean_ms;
} rrt_path_chooser_stats;
int rrt_path_chooser_create(int frames_in_flight, int window_frames, int* out_id);
int rrt_path_chooser_destroy(int id);
int rrt_path_chooser_policy(int id, int frame, int* policy_out);
int rrt_path_chooser_report(int id, int frame, float sustained_ms);
int rrt_path_chooser_get_stats(int id, rrt_path_chooser_stats* out);


/* ---- march cache: retained geodesics of a still camera ("Retained geodesics") ----
 * rrt_launch_raymarch, _rows and _tiles WITHOUT an rrt_params.workspace keep state per device: about 90 % of a frame is the
 * march of the geodesics, and the march does not depend on `time`, the sky, the noise table or the effects applied after it.
 * The library remembers the last launch's key per device (camera block, size, row selection, spin, volumetrics, max_steps,
 * nudge, arith_mode, the lens distortion).  A launch with another key runs exactly as before.  The second
 * consecutive launch of a key runs the three passes and keeps pass 1's output (a "fill"); the third and later ones run only the
 * media evaluation and the composite on the retained rows (a "hit") -- same bytes as the uncached launch, always.  Not cached:
 * launches with a workspace, an rrt_tile_order or an rrt_tile_map, with path_policy RRT_PATH_SINGLE, without volumetrics, with
 * debug outputs, launches being captured into a graph, and the _ss / _mb / _pano / _stereo launches.
 * Memory: allocated at the first fill, kept until released; bounded by max_bytes -- default the smaller of 8 GiB and a quarter of
 * the device memory free at the first use.  A frame that does not fit stays on the uncached path (no error; `why` says so).
 * RRT_MARCH_CACHE=0 in the environment switches it off for every device. */
typedef struct rrt_march_cache_info {
    uint64_t fills, hits;              /* launches that filled the cache / were served from it */
    uint64_t drops;                    /* keys given up after a fill had been made or started for them */
    uint64_t misses;                   /* launches whose key differed from the previous one's (uncached path, key remembered) */
    uint64_t uncacheable;              /* launches of a repeated key that stayed on the uncached path */
    uint64_t bytes, max_bytes;         /* device memory held / the budget (0: off) */
    uint64_t blocks_used, blocks_capacity;   /* of the current key's fill, in pool blocks */
    int32_t state;                     /* 0 none, 1 key seen once, 2 fill not yet verified, 3 refill at a larger capacity next, 4 ready, 5 uncacheable */
    int32_t why;                       /* state 5: 1 the budget is too small, 2 the pool overflowed twice, 3 allocation failed */
} rrt_march_cache_info;
/* device < 0: the calling thread's current device.  configure: max_bytes 0 = off; forgets the key, frees memory above the budget */
int rrt_march_cache_configure(int device, size_t max_bytes);
int rrt_march_cache_stats(int device, rrt_march_cache_info* out);
/* waits for the launches through the cache, frees everything, forgets the key; counters and budget stay.  Nothing is freed
 * at process exit or library unload: call this first if that matters */
int rrt_march_cache_release(int device);

/* ---- host-side camera helpers (host C++ in the reference too) ---- */
/* CameraController::getCUDAStateFrom, src/main.cpp:141-167 (degrees; note its 3.14159f) */
int rrt_camera_from_angles(const float pos[3], float yaw_deg, float pitch_deg, rrt_camera* out);
/* catmull_rom / lerp_angle, src/camera_paths.cpp:6-29 */
int rrt_catmull_rom(const float p0[3], const float p1[3], const float p2[3], const float p3[3], float t, float out[3]);
int rrt_lerp_angle(float a, float b, float t, float* out);
/* the three built-in keyframe paths, src/camera_paths.cpp:31-73 (0 "Gargantua Fly-By",
 * 1 "Event Horizon Focus", 2 "Horizon Skimmer"); keyframes are 6 floats: time, x, y, z, yaw, pitch */
int rrt_path_count(void);
int rrt_path_info(int path, const char** name, int* n_keys, float* t_end);
int rrt_path_keyframes(int path, float* out6, int cap_keys);
/* PathController::getInterpolatedState, src/main.cpp:176-203 */
int rrt_path_camera_at(int path, float path_time, rrt_camera* out);
/* recording clock of the main loop, src/main.cpp:511-516: times seen by 1-based frame k */
int rrt_recording_clock(int frame_k, int fps, float* sim_time, float* path_time);
/* the shutter of a motion-blurred frame k (rrt_launch_raymarch_mb; no counterpart in the reference), in binary32:
 * (S, P) = rrt_recording_clock(frame_k, fps), d = shutter * (1.0f / fps), u_m = ((float)(n_times - m) - 0.5f) / (float)n_times,
 * sim_times[m] = S - d * u_m and path_times[m] = P - d * u_m for m < n_times: the midpoints of n_times equal slices of the
 * trailing interval (S - d, S], increasing.  shutter in [0, 1] (0: every sub-time is the frame's own), n_times in
 * {1, 2, 4, 8, 16}; either output may be NULL. */
int rrt_motion_clock(int frame_k, int fps, float shutter, int n_times, float* sim_times, float* path_times);

#ifdef __cplusplus
}
#endif
#endif /* RRT_H */
