/*
 * rrt_hip.hip -- the HIP translation unit of librrt_hip.so: host side of the render path and its C ABI (include/rrt.h).
 *
 * Replaces the reference's only CUDA translation unit, src/raymarcher.cu (raymarch_kernel :15-174 and launch_raymarch
 * :176-180).  Built with
 *   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize -mllvm -enable-post-misched=false
 *         -mllvm -amdgpu-sched-strategy=max-ilp -fPIC
 * (relativisticraytracer_amd/build.py).  gfx950 only: no other target, no CUDA dual path.
 *
 * Sections (round 5: one 3 100-line file became four)
 *   rrt_kernels.h      the kernels and the structures they share with the host (included below: a kernel and its launch
 *                      site share a translation unit); rrt_glow.h, rrt_exposure.h: the two post passes' kernels
 *   this file          host helpers (the five handle tables, path choice and launch logic, the march cache's device object, what
 *                      the entry points share) in ONE anonymous namespace, then the C ABI in ONE extern "C" block, grouped by
 *                      object in the order include/rrt.h declares them; the C++ launch_raymarch at the end
 *   rrt_handles.h      HandleTable: the registry behind every kind of handle, and the list of what the entry points do
 *                      differently on purpose (host only, no HIP)
 *   rrt_noise_plan.h   NoiseTableObject and the noise tables' planning; rrt_tile_objects.h: TileMapObject, TileOrderObject
 *   rrt_march_cache.h  the march cache's key, policy state machine and capacity rule (host only, no HIP)
 *   rrt_camera.cpp     camera basis / path playback / recording clock (plain C++)
 *   rrt_test_hooks.h   rrt_unit_*, rrt_selfcheck_*, rrt_debug_fake_device -- compiled only with -DRRT_TEST_HOOKS, i.e. into
 *                      librrt_hip_test.so; the product library exports none of them
 */
#include <hip/hip_runtime.h>

#include <atomic>
#include <memory>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>
#include <algorithm>
#include <type_traits>

#include "../../include/rrt.h"
#ifdef RRT_TEST_HOOKS
#include "../../include/rrt_test.h"
#include "../../include/rrt_test_records.h"     /* the sample-record hooks: one exported table, no function export */
#endif
#include "rrt_device.h"
#include "rrt_tile_sort.h"              /* the native radix sort behind rrt_tile_order */
#include "rrt_march_cache.h"            /* the march cache's key, policy and capacity rule (host only) */
#include "rrt_handles.h"                /* HandleTable (host only) */

namespace {

using namespace rrt;
using rrt_handles::HandleTable;

thread_local char g_hip_err[256] = "";

int hip_fail(hipError_t e, const char* what) {
    snprintf(g_hip_err, sizeof(g_hip_err), "%s: %s", what, hipGetErrorString(e));
    return RRT_ERR_HIP;
}
#define RRT_HIP(call)                                       \
    do {                                                    \
        hipError_t e_ = (call);                             \
        if (e_ != hipSuccess) return hip_fail(e_, #call);   \
    } while (0)

/* is `st` being captured into a graph?  The null stream never is; an error from the query reads as "no" and is cleared */
bool stream_is_capturing(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (st != nullptr && hipStreamIsCapturing(st, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
    return cap != hipStreamCaptureStatusNone;
}

/* ------------------------------------------------------------------ handles (the tables: rrt_handles.h)
 * Every handle records the HIP device it was created on, and every entry point that would dereference its
 * allocation from a kernel or a copy compares that with the calling thread's current device: a sky, workspace or
 * noise table used under another hipSetDevice() is RRT_ERR_BAD_HANDLE, not a wild device pointer inside a kernel
 * (the one-process N-GPU driver and the process-global launch defaults make that mistake easy).
 * rrt_debug_fake_device() (librrt_hip_test.so) lets a CPU-only test drive those checks. */
#ifdef RRT_TEST_HOOKS            /* librrt_hip_test.so only */
std::atomic<int> g_fake_device{-1};
bool test_hooks_enabled() {       /* decided once, from the environment the process was started with */
    static const bool on = [] { const char* e = getenv("RRT_ENABLE_TEST_HOOKS"); return e && e[0] == '1'; }();
    return on;
}
int faked_device() { return g_fake_device.load(std::memory_order_relaxed); }
#else
constexpr int faked_device() { return -1; }
#endif
int current_device() {
    const int fake = faked_device();
    if (fake >= 0) return fake;
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); return -1; }
    return d;
}
/* -1 on either side (no HIP device could be asked) does not fail a launch by itself */
bool on_current_device(int object_device) {
    if (object_device < 0) return true;
    const int d = current_device();
    return d < 0 || d == object_device;
}

struct SkyObject {
    uint8_t* d_texels;
    int w, h;
    bool owned;
    int device;
};

/* ------------------------------------------------------------------ device code (kernels, kernel arguments, pool layout) */
#include "rrt_kernels.h"
#include "rrt_glow.h"                   /* the glow's kernels (rrt_launch_glow) */
#include "rrt_exposure.h"               /* exposure control: the bin rule and the resolve walk (host and device), its kernels */

struct WorkspaceObject {
    uint8_t* d_base; size_t bytes; int device;
    DeferCounters* h_stats;      /* pinned host copy (one per chain) of the counters its last launch left (asynchronous, behind that launch) */
    hipStream_t side;            /* the second chain's stream (round 4), with the two events that fork it from and join it to the caller's */
    hipEvent_t forked, joined;
};

/* ------------------------------------------------------------------ lattice-hash tables: NoiseTableObject + planning */
#include "rrt_noise_plan.h"

/* ------------------------------------------------------------------ TileMapObject (rrt_tile_map), TileOrderObject (rrt_tile_order) */
#include "rrt_tile_objects.h"

/* ------------------------------------------------------------------ the five handle tables
 * Process-lifetime objects; an element's destructor never calls HIP (device memory is freed by the destroy entry points only:
 * what is still registered at exit goes with the process).  rrt_sky_t ids start at "RT" << 48 | 1, the int ids at 1. */
HandleTable<rrt_sky_t, SkyObject> g_skies(0x5254000000000001ull);
HandleTable<int, WorkspaceObject> g_workspaces(1);
HandleTable<int, NoiseTableObject> g_noise_tables(1);
HandleTable<int, std::shared_ptr<TileMapObject>> g_tile_maps(1);
HandleTable<int, std::shared_ptr<TileOrderObject>> g_tile_orders(1);

template <class T> int device_of(const T& object) { return object.device; }
template <class T> int device_of(const std::shared_ptr<T>& object) { return object->device; }
/* the object behind `id`, for a caller that will dereference its device memory: unknown, or made under another device than the
 * calling thread's current one, is RRT_ERR_BAD_HANDLE */
template <class Id, class T>
int lookup_here(HandleTable<Id, T>& table, std::common_type_t<Id> id, T& out) {
    return table.get(id, out) && on_current_device(device_of(out)) ? RRT_OK : RRT_ERR_BAD_HANDLE;
}
/* take()'s predicate of the two kinds that are destroyed under their own device only */
template <class T>
bool made_here(const std::shared_ptr<T>& object) { return on_current_device(object->device); }

#ifdef RRT_TEST_HOOKS
#define RRT_TEST_HOOKS_PART 1
#include "rrt_test_hooks.h"
#undef RRT_TEST_HOOKS_PART
#endif

/* ------------------------------------------------------------------ host helpers */
/* an rrt_params built against another header is refused before any field of it is believed -- except ABI 4's 48-byte
 * layout, a strict prefix of this one: its caller simply has no nudge fields (they read as 0) */
constexpr uint32_t kParamsSizeAbi4 = 48;
static_assert(sizeof(rrt_params) == 56 && offsetof(rrt_params, nudge_ulps) == kParamsSizeAbi4, "rrt_params layout (ABI 5)");
int check_params_abi(const rrt_params* prm) {
    if (prm && prm->struct_size != (uint32_t)sizeof(rrt_params) && prm->struct_size != kParamsSizeAbi4) {
        snprintf(g_hip_err, sizeof(g_hip_err), "rrt_params.struct_size %u, this library's is %zu (ABI %d; ABI 4's %u is accepted too): recompile against include/rrt.h",
                 prm->struct_size, sizeof(rrt_params), RRT_ABI_VERSION, kParamsSizeAbi4);
        return RRT_ERR_ABI_MISMATCH;
    }
    return RRT_OK;
}
/* the caller's struct (NULL: config.h defaults) as this library's layout; check_params_abi() has passed */
void load_params(const rrt_params* in, rrt_params& out) {
    rrt_params_init(&out, (uint32_t)sizeof(out));
    if (in) memcpy(&out, in, in->struct_size < sizeof(out) ? in->struct_size : sizeof(out));
    out.struct_size = (uint32_t)sizeof(out);
}
int check_params_values(const rrt_params* prm_in) {
    rrt_params full;
    load_params(prm_in, full);
    const rrt_params* prm = &full;
    if (prm->max_steps < 0 || prm->sky_frac_bits < 0 || prm->sky_frac_bits > 16) return RRT_ERR_INVALID_ARGUMENT;
    if (!(prm->spin == prm->spin)) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->arith_mode != RRT_ARITH_STRICT && prm->arith_mode != RRT_ARITH_FAST && prm->arith_mode != RRT_ARITH_FMAD) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->workspace < 0) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->path_policy < RRT_PATH_AUTO || prm->path_policy > RRT_PATH_THREE_PASS) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->noise_table < 0 || prm->tile_order < 0) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->pool_rounds < 0 || prm->pool_rounds > 64) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->pass_chains < 0 || prm->pass_chains > kMaxChains) return RRT_ERR_INVALID_ARGUMENT;
    if (prm->nudge_ulps < 0 || prm->nudge_ulps > 4096) return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}
int check_common(const void* out, int width, int height, const rrt_camera* cam, const rrt_effects* fx,
                 const rrt_params* prm) {
    if (!out || !cam || !fx || width <= 0 || height <= 0) return RRT_ERR_INVALID_ARGUMENT;
    if ((long long)width * height > (1ll << 31) - 1) return RRT_ERR_INVALID_ARGUMENT;
    if (height > kMaxGridY * kWGPixY) return RRT_ERR_INVALID_ARGUMENT;             /* 524 280 rows */
    if (prm) {
        const int rc = check_params_abi(prm);
        if (rc != RRT_OK) return rc;
        return check_params_values(prm);
    }
    return RRT_OK;
}

struct LaunchOpts { int media; int arith; int workspace, policy, pool_rounds, pass_chains; };

int fill_args(FrameArgs& a, LaunchOpts& o, void* out, int width, int height, float time, const rrt_camera* cam,
              rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm_in) {
    rrt_params prm;
    load_params(prm_in, prm);
    SkyObject so;
    if (lookup_here(g_skies, sky, so)) return RRT_ERR_BAD_HANDLE;
    const SkyObject* s = &so;
    a.out = static_cast<uchar4*>(out);
    a.width = width; a.height = height; a.time = time; a.cam = *cam;
    a.sky.texels = s->d_texels; a.sky.w = s->w; a.sky.h = s->h; a.sky.frac_bits = prm.sky_frac_bits;
    a.use_bloom = fx->use_bloom != 0; a.use_vignette = fx->use_vignette != 0;
    a.use_ca = fx->use_chromatic_aberration != 0; a.use_lens = fx->use_lens_distortion != 0;
    a.bloom_threshold = fx->bloom_threshold; a.bloom_intensity = fx->bloom_intensity;
    a.vignette_intensity = fx->vignette_intensity; a.ca_amount = fx->ca_amount;
    a.distortion_amount = fx->distortion_amount;
    a.spin = prm.spin;
    a.drag_c = (2.0f * prm.spin) * 2.0f;            /* 2.0f * SPIN_A * EVENT_HORIZON, geodesics.h:41 */
    a.max_steps = prm.max_steps;
    a.nudge_ulps = prm.nudge_ulps; a.nudge_seed = prm.nudge_seed;
    memset(&a.dbg, 0, sizeof(a.dbg));
    a.tile_perm = nullptr; a.tile_cost = nullptr; a.tile_order_id = prm.tile_order;
    a.grid_rows = 0; a.grid_row_base = 0; a.grid_row_stride = 1;
    if (prm.tile_order != 0) {                      /* whatever path the launch takes: a stale or foreign id is an error */
        std::shared_ptr<TileOrderObject> to;
        if (lookup_here(g_tile_orders, prm.tile_order, to)) return RRT_ERR_BAD_HANDLE;
    }
    o.media = prm.volumetrics != 0 ? 1 : 0;
    memset(&a.lut_acc, 0, sizeof(a.lut_acc)); memset(&a.lut_dust, 0, sizeof(a.lut_dust)); memset(&a.dust_bands, 0, sizeof(a.dust_bands));
    if (prm.noise_table != 0) {
        NoiseTableObject nt;
        if (lookup_here(g_noise_tables, prm.noise_table, nt)) return RRT_ERR_BAD_HANDLE;
        /* the boxes were sized for t0 <= time <= t1; any other time runs the arithmetic kernels (same bytes) */
        if (o.media && time >= nt.t0 && time <= nt.t1) {
            o.media = nt.banded ? 3 : 2;
            a.lut_acc = make_lut(nt.d_cells, nt.acc, nt.acc_families);
            a.lut_dust = make_lut(nt.d_cells + dust_cell0(nt), nt.dust, nt.dust_families);
            a.dust_bands = make_bands(nt);
        }
    }
    o.arith = prm.arith_mode;
    o.workspace = prm.workspace;
    o.policy = prm.path_policy;
    o.pool_rounds = prm.pool_rounds;
    o.pass_chains = prm.pass_chains;
    a.ctr = nullptr; a.hdr = nullptr; a.finals = nullptr; a.n_lanes = 0; a.sample_blocks = nullptr; a.block_capacity = 0;
    return RRT_OK;
}

/* Largest max_steps the three-pass bookkeeping can represent: the step count shares a word with the hit /
 * resume flags (30 bits), and pass 3 walks at most kMaxRunsWalked runs of a wave, whose lengths double up to
 * kMaxRun blocks of kBlockRows rows -- a wave can pool one row per step, so it must not need more runs than
 * that.  Launches with more steps take the single kernel (same bytes). */
constexpr long long kThreePassMaxSteps = (long long)(kMaxRunsWalked - 8) * kMaxRun * kBlockRows;   /* ~262 k */
static_assert(kThreePassMaxSteps < (1ll << 30), "step count must fit beside the two flag bits");
constexpr int kFinalPlanes = 11;      /* per ray: vel xyz, code, pos xyz, radiance rgbt */
constexpr int kMaxPoolRounds = 64;

/* Where the three-pass bookkeeping of a launch over `grid` sits in its memory: the chains' counters at byte 0, the wave headers
 * at off_hdr, `final_planes` float planes of n_lanes rays at off_fin, the sample blocks from off_rows on (all multiples of 256) */
struct PoolLayout {
    size_t n_waves, n_lanes, off_hdr, off_fin, off_rows;
    static size_t align(size_t v) { return (v + 255) & ~(size_t)255; }
    /* how many blocks of `block_bytes` fit in `bytes` (the block index shares its word with flags) */
    static size_t blocks_in(size_t bytes, size_t block_bytes) { return std::min<size_t>(bytes / block_bytes, 0x0fffffffu); }
};
PoolLayout pool_layout(dim3 grid, int final_planes) {
    static_assert(kMaxChains * kCounterStride <= 256, "the chains' counters sit in front of the wave headers");
    PoolLayout l;
    l.n_waves = (size_t)grid.x * grid.y * kWGWaves;
    l.n_lanes = l.n_waves * 64;
    l.off_hdr = 256;
    l.off_fin = PoolLayout::align(l.off_hdr + l.n_waves * sizeof(WaveHdr));
    l.off_rows = PoolLayout::align(l.off_fin + l.n_lanes * 4 * final_planes);
    return l;
}

/* How many rounds to enqueue (rrt_params.pool_rounds == 0).  The host cannot ask the device without stalling the
 * stream, so it reads the statistics the workspace's PREVIOUS launch left in pinned host memory (an asynchronous copy
 * behind its last kernel; possibly a frame stale, which is all an animation needs): as many rounds as that launch had
 * work for -- PLUS ONE spare unless its fullest round left a fifth of the pool free (a view that changes finds room; an idle
 * round costs four near-empty launches: every wave leaves on one scalar load) --, twice as many plus one if rays were still
 * suspended at its end.  Rays the enqueued
 * rounds do not finish take the in-line route: the bytes never depend on the guess. */
int auto_pool_rounds(const volatile DeferCounters* h, unsigned capacity) {
    if (!h) return 2;
    const unsigned run = h->rounds_run, work = h->rounds_with_work, left = h->suspended_left, peak = h->peak_blocks;
    if (run == 0u) return 2;                                    /* no history */
    int r = (int)(work > 0u ? work : 1u);
    /* round 5: no spare round while the pool has room to spare -- the previous launch finished everything and its fullest
     * round used at most 80 % of this launch's pool: a view that changes from one frame to the next does not outgrow that, and
     * the idle round's four near-empty launches are ~1 % of a rank's share of a frame.  (If it ever does overflow, those rays
     * finish in line -- same bytes -- and the next launch sees suspended_left != 0.) */
    if (left == 0u && (unsigned long long)peak * 5ull <= (unsigned long long)capacity * 4ull) return r > kMaxPoolRounds ? kMaxPoolRounds : r;
    r = left != 0u ? 2 * r + 1 : r + 1;
    return r > kMaxPoolRounds ? kMaxPoolRounds : r;
}

/* The template instances of a launch: f(SPIN, MEDIA, ARITH) with the three as std::integral_constants.  MEDIA0: `media == 0`
 * (no volumetrics) is an instance of its own -- the single kernels; the three-pass chain has no such instance (a launch
 * without volumetrics never takes it) and dispatches with MEDIA0 = false */
template <bool MEDIA0 = true, class F>
void dispatch_kernel(bool spin, int media, int arith, F&& f) {
    const auto by_arith = [&](auto S, auto M) {
        if (arith == kArithFast) f(S, M, std::integral_constant<int, kArithFast>{});
        else if (arith == kArithFmad) f(S, M, std::integral_constant<int, kArithFmad>{});
        else f(S, M, std::integral_constant<int, kArithStrict>{});
    };
    const auto by_media = [&](auto S) {
        if (media == 3) by_arith(S, std::integral_constant<int, 3>{});
        else if (media == 2) by_arith(S, std::integral_constant<int, 2>{});
        else if (!MEDIA0 || media == 1) by_arith(S, std::integral_constant<int, 1>{});
        else if constexpr (MEDIA0) by_arith(S, std::integral_constant<int, 0>{});
    };
    if (spin) by_media(std::true_type{}); else by_media(std::false_type{});
}

/* the rounds of one chain.  KEEP: the march cache's chain (rrt_march_cache.h) -- one round, pass 2's results in planes of their
 * own (kp); with kp.replay pass 1 and the round's close are left out.  (The kernels of passes 2 and 3 take a KeepArgs whether
 * or not they are KEEP instances: one signature per kernel; the workspace path passes an empty one, which its instances never
 * read.  march_defer has no MEDIA parameter: every MEDIA launches the same instance.) */
/* The grid of a replay's pass 2.  Its waves take blocks from a cursor (eval_sample_rows), so the grid need not equal the chip: it
 * is what the device holds of that instance at once -- the occupancy query times the CU count, asked once per device and instance
 * and kept in the device's MarchCacheObject.  `forced`: the test library's hook (rrt_test_records.replay_grid), 0 otherwise. */
struct ReplayGrid {
    unsigned blocks[3][4] = {};       /* [ARITH][MEDIA]; 0: not asked yet */
    unsigned forced = 0;
};
template <int ARITH, int MEDIA>
int replay_grid_blocks(ReplayGrid& g, unsigned& blocks) {
    static_assert(ARITH >= 0 && ARITH < 3 && MEDIA >= 0 && MEDIA < 4, "ReplayGrid::blocks is indexed by the instance");
    unsigned& slot = g.blocks[ARITH][MEDIA];
    if (slot == 0u) {
        int dev = 0, cus = 0, per_cu = 0;
        RRT_HIP(hipGetDevice(&dev));
        RRT_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
        RRT_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, eval_sample_rows<ARITH, MEDIA, true>, 256, 0));
        slot = (unsigned)std::max(cus, 1) * (unsigned)std::max(per_cu, 1);
    }
    blocks = g.forced != 0u ? g.forced : slot;
    return RRT_OK;
}

template <bool SPIN, int MEDIA, int ARITH, bool KEEP>
int enqueue_rounds(const FrameArgs& a, dim3 grid, dim3 block, int rounds, hipStream_t st, const KeepArgs kp, ReplayGrid* rg) {
    const bool replay = KEEP && kp.replay != 0;
    if (KEEP) rounds = 1;
    unsigned eval_blocks = 2048u;           /* 256 CUs x 8 workgroups: the static row stride of the fill and the workspace path */
    if constexpr (KEEP) {
        if (replay) { const int rc = replay_grid_blocks<ARITH, MEDIA>(*rg, eval_blocks); if (rc != RRT_OK) return rc; }
    }
    for (int r = 0; r < rounds; ++r) {
        const bool last = r == rounds - 1;
        if (!replay) {
            if (r == 0) hipLaunchKernelGGL((march_defer<SPIN, ARITH, false>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((march_defer<SPIN, ARITH, true>), grid, block, 0, st, a);
        }
        RRT_HIP(hipGetLastError());
        hipLaunchKernelGGL((eval_sample_rows<ARITH, MEDIA, KEEP>), dim3(eval_blocks), dim3(256), 0, st, a, kp);
        RRT_HIP(hipGetLastError());
        /* LAST = true for the last round enqueued; the cache's chain (KEEP) has one round, so only <LAST, KEEP> = <true, true> exists */
        if constexpr (KEEP) hipLaunchKernelGGL((composite_and_shade<SPIN, ARITH, MEDIA, true, true>), grid, block, 0, st, a, kp);
        else if (last) hipLaunchKernelGGL((composite_and_shade<SPIN, ARITH, MEDIA, true, false>), grid, block, 0, st, a, kp);
        else hipLaunchKernelGGL((composite_and_shade<SPIN, ARITH, MEDIA, false, false>), grid, block, 0, st, a, kp);
        RRT_HIP(hipGetLastError());
        if (replay) break;
        hipLaunchKernelGGL(pool_next_round, dim3(1), dim3(1), 0, st, a.ctr, a.block_capacity, last ? 1 : 0);
        RRT_HIP(hipGetLastError());
    }
    return RRT_OK;
}

/* one chain = march -> evaluate -> composite (in rounds) over dispatch rows [row0, row1) of the launch, in its own slice
 * of the pool, on its own stream; `keep`: the march cache's chain */
int enqueue_chain(FrameArgs a, int arith, int media, dim3 full_grid, int row0, int row_stride, int n_rows, int rounds, hipStream_t st,
                  const KeepArgs* keep = nullptr, ReplayGrid* replay_grid = nullptr) {
    if (n_rows <= 0) return RRT_OK;
    const dim3 block(kWGThreads), grid(full_grid.x, (unsigned)n_rows);
    a.grid_rows = (int)full_grid.y; a.grid_row_base = row0; a.grid_row_stride = row_stride;
    int rc = RRT_OK;
    dispatch_kernel<false>(a.spin != 0.0f, media, arith, [&](auto S, auto M, auto A) {
        rc = keep ? enqueue_rounds<S, M, A, true>(a, grid, block, 1, st, *keep, replay_grid)
                  : enqueue_rounds<S, M, A, false>(a, grid, block, rounds, st, KeepArgs{nullptr, 0u, 0}, nullptr);
    });
    return rc;
}

/* Three-pass launch through a workspace.  Returns RRT_OK after enqueuing, or -1 if the workspace cannot
 * hold this launch's bookkeeping plus a useful pool (the caller then uses the single-kernel path).
 *
 * TWO CHAINS (round 4).  A rank's share of a frame is a few rounds of wavefronts, and each of the three kernels ends in a
 * tail: a lone wavefront retires a dependent instruction every ~10 clocks, the SIMDs are only busy with 5-6 of them, so the
 * last-started waves of the march take a full 1.5 ms whatever else has finished, and the chip decays from full to empty
 * over that time (profiles/r04_wave_timeline_default.txt: 1.1 of the 5.4 ms of an eighth of the 4K bench frame).  The
 * launch is therefore cut in two along its dispatch order -- the first half of the dispatch rows (the frame's middle, or the
 * costliest tiles under rrt_tile_order) and the second -- and each half runs its own march -> evaluate -> composite chain
 * on its own stream with its own slice of the pool: the evaluation and compositing of one half fill the march tail of the
 * other.  Same kernels, same arithmetic, same bytes; an eighth of the bench frame 5.7 -> 5.2 ms, of the view from inside
 * the disk 12.4 -> 9.5 ms (profiles/r04_split_chain_probe.txt).  The side stream and its events belong to the workspace;
 * a launch that is being captured into a graph, or a small one, runs one chain. */
int launch_deferred(FrameArgs a, int arith, int media, const WorkspaceObject& ws, int pool_rounds, int chains_wanted, hipStream_t st) {
    dim3 grid((a.width + kWGPixX - 1) / kWGPixX, (a.rows.n_local_rows + kWGPixY - 1) / kWGPixY);
    const PoolLayout lay = pool_layout(grid, kFinalPlanes);
    const size_t n_waves = lay.n_waves, off_fin = lay.off_fin, off_rows = lay.off_rows;
    if (ws.bytes < off_rows + (size_t)1024 * kBlockBytes) return -1;
    const size_t cap = PoolLayout::blocks_in(ws.bytes - off_rows, kBlockBytes);
    a.hdr = reinterpret_cast<WaveHdr*>(ws.d_base + lay.off_hdr);
    a.finals = reinterpret_cast<float*>(ws.d_base + off_fin);
    a.n_lanes = lay.n_lanes;
    /* one chain or two */
    int chains = 1;
    if (chains_wanted != 1 && ws.side != nullptr && grid.y >= 8 && cap >= 4096 && n_waves >= (chains_wanted == 2 ? 2u : 2048u) &&
        !stream_is_capturing(st))
        chains = 2;
    hipLaunchKernelGGL(zero_words, dim3((unsigned)((off_fin / 16 + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<uint4*>(ws.d_base), off_fin / 16);        /* counters + wave headers (off_fin is a multiple of 256) */
    RRT_HIP(hipGetLastError());
    /* the pool's split: by what each chain pooled last time (the heavy half holds most of the media), 65 : 35 without history */
    size_t cap_of[kMaxChains] = {cap, 0};
    /* which dispatch rows a chain takes: the first and the second half of the static order (the frame's middle and the rest) --
     * or, when the order is by COST (rrt_tile_order), every other row each: the halves of a cost-sorted order are "all the
     * expensive tiles" and "all the cheap ones", which made the two chains worse than one (5.15 -> 5.45 ms on an
     * eighth of the bench frame), while even and odd rows of it carry the same cost */
    const bool deal_rows = chains == 2 && a.tile_perm != nullptr;
    int row_first[kMaxChains] = {0, deal_rows ? 1 : (int)grid.y / 2};
    int row_step = deal_rows ? 2 : 1;
    int row_count[kMaxChains] = {(int)grid.y, 0};
    if (chains == 2) {
        row_count[0] = deal_rows ? ((int)grid.y + 1) / 2 : (int)grid.y / 2;
        row_count[1] = (int)grid.y - row_count[0];
    }
    if (chains == 2) {
        double share = deal_rows ? 0.5 : 0.65;
        const volatile DeferCounters* h = ws.h_stats;
        if (h && h[0].rounds_run != 0u && h[1].rounds_run != 0u) {
            const double t0 = (double)h[0].total_blocks, t1 = (double)h[1].total_blocks;
            if (t0 + t1 > 0.0) share = t0 / (t0 + t1);
        }
        share = share < 0.3 ? 0.3 : (share > 0.85 ? 0.85 : share);
        cap_of[0] = (size_t)((double)cap * share);
        cap_of[1] = cap - cap_of[0];
    }
    if (chains == 2) {            /* fork: the side stream starts behind the memset, BEFORE anything of chain 0 is in the caller's stream */
        RRT_HIP(hipEventRecord(ws.forked, st));
        RRT_HIP(hipStreamWaitEvent(ws.side, ws.forked, 0));
    }
    size_t block0 = 0;
    for (int c = 0; c < chains; ++c) {
        FrameArgs b = a;
        b.ctr = reinterpret_cast<DeferCounters*>(ws.d_base + (size_t)c * kCounterStride);
        b.sample_blocks = ws.d_base + off_rows + block0 * kBlockBytes;
        b.block_capacity = (unsigned)cap_of[c];
        const int rounds = pool_rounds > 0 ? pool_rounds : auto_pool_rounds(ws.h_stats ? ws.h_stats + c : nullptr, b.block_capacity);
        const hipStream_t cs = c == 1 ? ws.side : st;
        const int rc = enqueue_chain(b, arith, media, grid, row_first[c], row_step, row_count[c], rounds, cs);
        if (rc != RRT_OK) return rc;
        /* what this chain needed, for the next launch's round count and pool split (and rrt_workspace_stats) */
        if (ws.h_stats) RRT_HIP(hipMemcpyAsync(ws.h_stats + c, b.ctr, sizeof(DeferCounters), hipMemcpyDeviceToHost, cs));
        if (c == 1) {                                          /* join */
            RRT_HIP(hipEventRecord(ws.joined, ws.side));
            RRT_HIP(hipStreamWaitEvent(st, ws.joined, 0));
        }
        block0 += cap_of[c];
    }
    if (chains == 1 && ws.h_stats) memset(const_cast<DeferCounters*>(ws.h_stats) + 1, 0, sizeof(DeferCounters));   /* no second chain this time */
    return RRT_OK;
}

/* When does the three-pass path pay?  It does ~8 % more work than the single kernel, but its longest
 * wavefront is a bare march (<= ~1.2 ms) instead of a march with every media sample in line (up to ~13 ms
 * on the bench view).  A launch only feels that pole once its own duration gets close to it, i.e. for
 * small launches -- one GPU's share of a frame that is spread over many GPUs.  Measured on the 4K bench
 * frame (profiles/README.md): 1/4 of the frame (2.07 M rays) 11.8 ms in line vs 12.6 ms three-pass;
 * 1/8 (1.04 M rays) 11.7 ms vs 6.8 ms. */
constexpr long long kThreePassMaxRays = 1500000;


/* ------------------------------------------------------------------ march cache: retained geodesics
 * One object per device, made at the first launch that could use it.  It owns the pool pass 1 fills for the most recent launch
 * key (rrt_march_cache.h: key, policy, capacity) and follows rrt_tile_order's rules for hidden state: one mutex per object held
 * while a launch is enqueued, launches through the object chained by an event (a replay on another stream never reads a
 * half-written fill), a launch that is being captured into a graph ignores it entirely, and so do debug launches. */
struct MarchCacheObject {
    std::mutex mu;
    int device = -1;
    rrt_mc::Policy pol;
    bool budget_known = false, configured = false;
    size_t max_bytes = 0;                  /* 0: off */
    uint8_t* d_base = nullptr; size_t bytes = 0;
    DeferCounters* h_stats = nullptr;      /* pinned: what the fill used, copied behind it */
    hipEvent_t chained = nullptr;
    unsigned long long launches = 0;
    /* layout of the current key's fill; off_out: pass 2's planes (KeepArgs), behind the sample blocks */
    PoolLayout lay{};
    size_t off_out = 0;
    unsigned cap_blocks = 0, used_blocks = 0;
    ReplayGrid replay_grid;                /* pass 2's grid on a replay, per instance */
};
struct MarchCacheRegistry {
    std::mutex mu;
    std::unordered_map<int, std::unique_ptr<MarchCacheObject>> by_device;
    static void free_device_memory(MarchCacheObject& c) {
        if (c.launches > 0 && c.chained) (void)hipEventSynchronize(c.chained);
        if (c.d_base) (void)hipFree(c.d_base);
        c.d_base = nullptr; c.bytes = 0; c.cap_blocks = 0;
        (void)hipGetLastError();
    }
    static void destroy(MarchCacheObject& c) {
        free_device_memory(c);
        if (c.h_stats) (void)hipHostFree(c.h_stats);
        if (c.chained) (void)hipEventDestroy(c.chained);
        c.h_stats = nullptr; c.chained = nullptr; c.launches = 0;
        (void)hipGetLastError();
    }
};
/* Never destroyed, and the handle tables hold nothing whose destructor touches HIP either: a static destructor would call into the HIP runtime at process exit
 * or library unload, when the runtime may already be gone.  rrt_march_cache_release() is the way to give the memory back; what
 * is still held at exit goes with the process. */
MarchCacheRegistry& march_caches() { static MarchCacheRegistry* const r = new MarchCacheRegistry; return *r; }
MarchCacheObject* march_cache_of(int device, bool create) {
    MarchCacheRegistry& r = march_caches();
    std::lock_guard<std::mutex> lk(r.mu);
    auto it = r.by_device.find(device);
    if (it != r.by_device.end()) return it->second.get();
    if (!create) return nullptr;
    auto c = std::make_unique<MarchCacheObject>();
    c->device = device;
    MarchCacheObject* p = c.get();
    r.by_device.emplace(device, std::move(c));
    return p;
}
/* RRT_MARCH_CACHE=0 in the environment switches every device's cache off, whatever rrt_march_cache_configure says */
bool march_cache_env_off() {
    static const bool off = [] { const char* e = getenv("RRT_MARCH_CACHE"); return e && e[0] == '0' && e[1] == 0; }();
    return off;
}
/* the byte budget, decided at first use: the smaller of 8 GiB and a quarter of the device memory free then */
size_t march_cache_budget(MarchCacheObject& c) {
    if (march_cache_env_off()) return 0;
    if (!c.budget_known) {
        if (!c.configured) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
            c.max_bytes = std::min<size_t>((size_t)8 << 30, free_b / 4);
        }
        c.budget_known = true;
    }
    return c.max_bytes;
}

/* THE KEY.  What pass 1 (march_defer) and the row bookkeeping read of a launch, proven from the source:
 *   lane_pixel / map_row / wave_slot / row_block   width, height, rows.{n_local_rows, y_base, tile_rows, shard, n_shards,
 *                                                  tile_of_local}, tile_perm, grid_rows / grid_row_base / grid_row_stride
 *   primary_ray                                    width, height, cam, use_lens, distortion_amount, nudge_ulps, nudge_seed
 *   the march loop                                 max_steps, drag_c (= 4 spin), SPIN = (spin != 0), ARITH
 *   pool bookkeeping                               ctr, hdr, finals, n_lanes, sample_blocks, block_capacity (the cache's own)
 *   tile_cost                                      written only (rrt_tile_order)
 * and nothing else: not `time` (media_densities is called by passes 2 and 3 only), not the sky, not the noise tables (MEDIA is
 * no template parameter of march_defer), not bloom / vignette / chromatic aberration.  Launches with an rrt_tile_map
 * (tile_of_local), an rrt_tile_order (tile_perm, tile_cost) or without volumetrics (no pass 1 exists) are not cached, so those
 * fields are not in the key; the cache runs ONE chain over the whole grid (grid_rows = 0), so the grid_row_* triple is constant.
 * max_steps above the three-pass bookkeeping's limit is not cached either.
 * The sample records the fill's pass 2 makes of the retained rows (rrt_device.h: SampleRecord) are functions of (rel_p, vel, spin,
 * ARITH) only -- pass 1's output and two fields of the key -- and of neither MEDIA, the tables, the sky nor the effects: no new field.
 * A field added to FrameArgs trips the assertion below: decide whether pass 1 reads it BEFORE changing the number. */
static_assert(sizeof(FrameArgs) == 416, "FrameArgs changed: does march_defer read the new field?  Then it belongs in rrt_mc::MarchKey (march_key)");
rrt_mc::MarchKey march_key(const FrameArgs& a, const LaunchOpts& o) {
    rrt_mc::MarchKey k;
    memset(&k, 0, sizeof(k));
    static_assert(sizeof(k.cam) == sizeof(a.cam), "rrt_camera is twelve floats");
    memcpy(k.cam, &a.cam, sizeof(k.cam));
    k.width = a.width; k.height = a.height;
    k.n_local_rows = a.rows.n_local_rows; k.y_base = a.rows.y_base; k.tile_rows = a.rows.tile_rows;
    k.shard = a.rows.shard; k.n_shards = a.rows.n_shards;
    memcpy(&k.spin, &a.spin, 4);
    k.max_steps = a.max_steps;
    k.nudge_ulps = a.nudge_ulps; k.nudge_seed = a.nudge_seed;
    k.arith_mode = o.arith;
    k.volumetrics = o.media != 0;
    k.use_lens = a.use_lens; memcpy(&k.distortion_amount, &a.distortion_amount, 4);
    rrt_mc::canonicalize(k);
    return k;
}

constexpr int kCacheFinalPlanes = 7;       /* vel xyz, code, pos xyz: one round, so no radiance is ever saved between rounds */
constexpr size_t kCacheBlockBytes = (size_t)kBlockBytes + kOutBlockBytes;

/* memory and layout for a fill of `grid` with (at least) the capacity rule's blocks; rrt_mc::kWhy* if there is none to be had */
int march_cache_reserve(MarchCacheObject& c, const FrameArgs& a, dim3 grid, bool grown) {
    const PoolLayout lay = pool_layout(grid, kCacheFinalPlanes);
    const size_t fixed = lay.off_rows + 256;
    const uint64_t rays = (uint64_t)a.width * (uint64_t)a.rows.n_local_rows;
    uint64_t blocks = rrt_mc::blocks_in_budget(rrt_mc::wanted_blocks(rays, kBlockBytes, grown), march_cache_budget(c), fixed, kCacheBlockBytes);
    if (blocks == 0) return rrt_mc::kWhyBudget;
    if (c.bytes > fixed) {                           /* memory an earlier key left: use all of it */
        const uint64_t have = PoolLayout::blocks_in(c.bytes - fixed, kCacheBlockBytes);
        if (have > blocks) blocks = have;
    }
    if (grown && blocks <= c.cap_blocks) return rrt_mc::kWhyOverflow;       /* the budget leaves nothing to grow into */
    const size_t need = fixed + (size_t)blocks * kCacheBlockBytes;
    if (!c.chained) {
        if (hipEventCreateWithFlags(&c.chained, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&c.h_stats), sizeof(DeferCounters), hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            MarchCacheRegistry::destroy(c);
            return rrt_mc::kWhyAlloc;
        }
        memset(c.h_stats, 0, sizeof(DeferCounters));
    }
    if (need > c.bytes) {
        MarchCacheRegistry::free_device_memory(c);          /* waits for the launches that still read it */
        if (hipMalloc(reinterpret_cast<void**>(&c.d_base), need) != hipSuccess) { (void)hipGetLastError(); c.d_base = nullptr; return rrt_mc::kWhyAlloc; }
        c.bytes = need;
    }
    c.lay = lay;
    c.cap_blocks = (unsigned)blocks;
    c.off_out = PoolLayout::align(lay.off_rows + (size_t)blocks * kBlockBytes);
    c.used_blocks = 0;
    return rrt_mc::kWhyNone;
}

/* a fill (march -> evaluate -> composite, pass 1 writing the cache) or a replay (evaluate -> composite on the retained rows):
 * one chain on the caller's stream.  Two chains were measured for a whole-frame replay and bought nothing (3.78 against 3.78 ms,
 * profiles/r07_march_cache_ab.txt): no second stream, no pool split. */
int march_cache_enqueue(MarchCacheObject& c, FrameArgs a, int arith, int media, dim3 grid, bool fill, hipStream_t st) {
    a.hdr = reinterpret_cast<WaveHdr*>(c.d_base + c.lay.off_hdr);
    a.finals = reinterpret_cast<float*>(c.d_base + c.lay.off_fin);
    a.n_lanes = c.lay.n_lanes;
    if (c.launches > 0) RRT_HIP(hipStreamWaitEvent(st, c.chained, 0));
    if (fill) {
        hipLaunchKernelGGL(zero_words, dim3((unsigned)((c.lay.off_fin / 16 + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<uint4*>(c.d_base), c.lay.off_fin / 16);
        RRT_HIP(hipGetLastError());
    }
    a.ctr = reinterpret_cast<DeferCounters*>(c.d_base);
    a.sample_blocks = c.d_base + c.lay.off_rows;
    a.block_capacity = c.cap_blocks;
    /* (the replay's hand-out cursor, rrt_kernels.h: replay_cursor, is the second counter slot of this header region: a.ctr is
     * the region's base on a fill and on a replay alike, the cache's one chain never uses that slot, zero_words above clears it
     * at every fill, and ONE cursor serves replays on any stream because c.chained serialises them) */
    const KeepArgs kp{c.d_base + c.off_out, fill ? 0u : c.used_blocks, fill ? 0 : 1};
    const int rc = enqueue_chain(a, arith, media, grid, 0, 1, (int)grid.y, 1, st, &kp, &c.replay_grid);
    if (rc != RRT_OK) return rc;
    if (fill) RRT_HIP(hipMemcpyAsync(c.h_stats, a.ctr, sizeof(DeferCounters), hipMemcpyDeviceToHost, st));
    RRT_HIP(hipEventRecord(c.chained, st));
    ++c.launches;
    return RRT_OK;
}

/* A launch without a workspace of its own asks its device's cache.  `launched`: the frame has been enqueued here; otherwise the
 * caller runs today's code, whether the key was only remembered, cannot be cached, or the cache is off. */
int march_cache_launch(const FrameArgs& a, const LaunchOpts& o, dim3 grid, hipStream_t st, bool& launched) {
    launched = false;
    if (march_cache_env_off() || faked_device() >= 0) return RRT_OK;
    if (stream_is_capturing(st)) return RRT_OK;                       /* a replayed graph must not read what a later launch rewrites */
    const int dev = current_device();
    if (dev < 0) return RRT_OK;
    MarchCacheObject* cp = march_cache_of(dev, true);
    std::lock_guard<std::mutex> lk(cp->mu);
    MarchCacheObject& c = *cp;
    if (march_cache_budget(c) == 0) return RRT_OK;
    const rrt_mc::MarchKey k = march_key(a, o);
    if (c.pol.pending_for(k)) {                   /* the third launch of a key: what did its fill use, did everything fit? */
        RRT_HIP(hipEventSynchronize(c.chained));
        const volatile DeferCounters* h = c.h_stats;
        c.used_blocks = h->peak_blocks;
        c.pol.fill_verified(h->rounds_run == 1u && h->suspended_left == 0u);
    }
    const rrt_mc::Action act = c.pol.next(k);
    if (act == rrt_mc::kFill) {
        const int why = march_cache_reserve(c, a, grid, c.pol.grown);
        if (why != rrt_mc::kWhyNone) c.pol.fill_failed(why);
    }
    /* a key that has been given up serves nothing: its memory goes back now, not when another key arrives */
    if (c.pol.state == rrt_mc::kOff && c.d_base) MarchCacheRegistry::free_device_memory(c);
    if (act == rrt_mc::kToday || c.pol.state == rrt_mc::kOff) return RRT_OK;
    const int rc = march_cache_enqueue(c, a, o.arith, o.media, grid, act == rrt_mc::kFill, st);
    if (rc != RRT_OK) { c.pol.reset(); return rc; }
    launched = true;
    return RRT_OK;
}

int march_cache_device(int device) { return device >= 0 ? device : current_device(); }
/* runs f with `device` current (the cache's memory is freed and allocated there) */
template <class F>
int on_device(int device, F&& f) {
    int prev = -1;
    if (faked_device() >= 0) return f();
    RRT_HIP(hipGetDevice(&prev));
    if (prev != device) RRT_HIP(hipSetDevice(device));
    const int rc = f();
    if (prev != device) (void)hipSetDevice(prev);
    return rc;
}

/* room for n tiles in a tile-order object (grows only; growing forgets the order) */
int tile_order_reserve(TileOrderObject& o, size_t n) {
    if (n <= o.n_cap) return RRT_OK;
    if (n > ((size_t)1 << 30)) return RRT_ERR_INVALID_ARGUMENT;
    RRT_HIP(hipDeviceSynchronize());                 /* launches through the object may still read the old buffers */
    unsigned** bufs[] = {&o.d_cost, &o.d_sorted, &o.d_iota, &o.d_perm[0], &o.d_perm[1]};
    for (unsigned** b : bufs) { if (*b) (void)hipFree(*b); *b = nullptr; }
    if (o.d_temp) (void)hipFree(o.d_temp);
    o.d_temp = nullptr; o.n_cap = 0; o.have = false;
    const size_t cap = n + n / 8;
    for (unsigned** b : bufs) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(b), cap * sizeof(unsigned));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(tile order)");
    }
    const size_t tb = (size_t)2 * 256 * rrt_sort::kMaxBlocks * sizeof(unsigned);      /* counters for any n (2 MB) */
    hipError_t e = hipMalloc(&o.d_temp, tb);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(tile order sort)");
    o.temp_bytes = tb;
    o.n_cap = cap;
    return RRT_OK;
}

/* enqueue the coarse probe of the launch `a` describes (its row map included) into `cells` */
int enqueue_probe(const FrameArgs& a, ProbeArgs& q, unsigned* cells, int stride_x, int stride_y, bool media, hipStream_t st) {
    q.cell_cost = cells;
    q.stride_x = stride_x; q.stride_y = stride_y;
    q.cells_x = (a.width + stride_x - 1) / stride_x;
    q.cells_y = (a.rows.n_local_rows + stride_y - 1) / stride_y;
    q.w_step = RRT_PROBE_W_STEP; q.w_acc = RRT_PROBE_W_ACC; q.w_dust = RRT_PROBE_W_DUST;
    q.ring_steps = (float)a.max_steps;
    if (!media) { q.w_acc = 0.0f; q.w_dust = 0.0f; }          /* volumetrics off: a sample costs nothing, the steps stay */
    if (const char* e = getenv("RRT_PROBE_WEIGHTS")) {          /* dev: tools/probe_fit.py reads the three counts one at a time */
        float w0, w1, w2;
        if (sscanf(e, "%f,%f,%f", &w0, &w1, &w2) == 3) { q.w_step = w0; q.w_acc = w1; q.w_dust = w2; }
    }
    const dim3 grid((q.cells_x + 7) / 8, (q.cells_y + 7) / 8);
    if (a.spin != 0.0f) hipLaunchKernelGGL((probe_costs<true>), grid, dim3(64), 0, st, a, q);
    else hipLaunchKernelGGL((probe_costs<false>), grid, dim3(64), 0, st, a, q);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

int launch(const FrameArgs& a, const LaunchOpts& o, bool debug, hipStream_t st) {
    dim3 block(kWGThreads);
    if (a.rows.n_local_rows == 0) return RRT_OK;
    const bool spin = a.spin != 0.0f;
    dim3 grid((a.width + kWGPixX - 1) / kWGPixX, (a.rows.n_local_rows + kWGPixY - 1) / kWGPixY);
    /* which path */
    WorkspaceObject ws{};
    bool deferred = false;
    if (o.workspace != 0) {
        if (lookup_here(g_workspaces, o.workspace, ws)) return RRT_ERR_BAD_HANDLE;
        const long long rays = (long long)a.width * a.rows.n_local_rows;
        const bool want = o.policy == RRT_PATH_THREE_PASS || (o.policy == RRT_PATH_AUTO && rays <= kThreePassMaxRays);
        deferred = o.media != 0 && !debug && want && a.max_steps <= kThreePassMaxSteps;
    }
    FrameArgs b = a;
    /* cost-ordered dispatch: read the order the previous launch through the object left (same geometry), or -- no history --
     * the order a coarse probe of this very view gives; record this launch's costs; sort them into the other buffer for the
     * next one.  A launch that is being captured into a graph renders in the static order and leaves the object alone: a
     * replayed graph must never read a permutation that a later live launch is rewriting. */
    std::shared_ptr<TileOrderObject> order;
    std::unique_lock<std::mutex> order_lock;
    const size_t n_tiles = (size_t)grid.x * grid.y;
    if (a.tile_order_id != 0 && !debug && kWGWaves == 1) {
        if (!stream_is_capturing(st)) {
            if (lookup_here(g_tile_orders, a.tile_order_id, order)) return RRT_ERR_BAD_HANDLE;
            order_lock = std::unique_lock<std::mutex>(order->mu);
            if (order->dead) return RRT_ERR_BAD_HANDLE;            /* destroyed while this thread waited for it */
            int rc = tile_order_reserve(*order, n_tiles);
            if (rc != RRT_OK) return rc;
            if (order->launches > 0) RRT_HIP(hipStreamWaitEvent(st, order->chained, 0));
            const bool same = order->have && order->grid_x == grid.x && order->grid_y == grid.y && order->width == a.width &&
                              order->height == a.height && same_row_map(order->rows, a.rows);
            if (!same && !order->no_seed) {
                /* first launch of this geometry: probe -> per-tile estimate -> order */
                ProbeArgs q;
                rc = enqueue_probe(a, q, order->d_sorted, kProbeStride, kProbeStride, o.media != 0, st);   /* d_sorted: scratch until the sort */
                if (rc != RRT_OK) return rc;
                hipLaunchKernelGGL(probe_to_tiles, dim3((unsigned)((n_tiles + 255) / 256)), dim3(256), 0, st, order->d_cost, grid.x, grid.y, q);
                RRT_HIP(hipGetLastError());
                const int next = order->cur ^ 1;
                RRT_HIP(rrt_sort::enqueue(order->d_cost, order->d_sorted, order->d_iota, static_cast<unsigned*>(order->d_temp),
                                          order->d_perm[next], n_tiles, grid.x, grid.y, kTileCostSortLo, st));
                order->cur = next;
                ++order->seeded;
            }
            const bool ordered = same || !order->no_seed;
            b.tile_perm = ordered ? order->d_perm[order->cur] : nullptr;
            b.tile_cost = order->d_cost;
            /* the one hipMemsetAsync on a launch path.  Safe where the workspace header's was not (zero_words, above): this
             * branch is only entered when `st` is NOT being captured -- a captured launch ignores the tile-order object -- so the
             * memset is never turned into a graph node that a replay would have to re-execute */
            RRT_HIP(hipMemsetAsync(order->d_cost, 0, n_tiles * sizeof(unsigned), st));
            if (same) ++order->ordered;
        }
    }
    bool launched = false;
    if (deferred) {
        const int rc = launch_deferred(b, o.arith, o.media, ws, o.pool_rounds, o.pass_chains, st);
        if (rc > 0) return rc;
        launched = rc == RRT_OK;
    }
    /* a launch that brings no workspace: its device's march cache may hold this key's geodesics (a still camera) */
    if (o.workspace == 0 && !debug && o.media != 0 && o.policy != RRT_PATH_SINGLE && a.tile_order_id == 0 &&
        a.rows.tile_of_local == nullptr && a.max_steps <= kThreePassMaxSteps) {
        const int rc = march_cache_launch(b, o, grid, st, launched);
        if (rc != RRT_OK) return rc;
    }
    if (!launched) {
        dispatch_kernel(spin, o.media, o.arith, [&](auto S, auto M, auto F) {
            if (debug) hipLaunchKernelGGL((raymarch_pixels<S, M, true, F>), grid, block, 0, st, b);
            else hipLaunchKernelGGL((raymarch_pixels<S, M, false, F>), grid, block, 0, st, b);
        });
        RRT_HIP(hipGetLastError());
    }
    if (order) {
        const int next = order->cur ^ 1;
        RRT_HIP(rrt_sort::enqueue(order->d_cost, order->d_sorted, order->d_iota, static_cast<unsigned*>(order->d_temp),
                                  order->d_perm[next], n_tiles, grid.x, grid.y, kTileCostSortLo, st));
        RRT_HIP(hipEventRecord(order->chained, st));
        order->cur = next; order->have = true; ++order->launches;
        order->grid_x = grid.x; order->grid_y = grid.y; order->width = a.width; order->height = a.height; order->rows = a.rows;
    }
    return RRT_OK;
}

/* the plain frame (rrt_launch_raymarch_rows, _ex, _tiles, _tilemap) once the entry point has made its own checks and built the
 * rows it renders; dbg: a debug launch (rrt_launch_raymarch_ex) */
int launch_frame(void* out, int width, int height, const RowMap& rows, float time, const rrt_camera* cam, rrt_sky_t sky,
                 const rrt_effects* fx, const rrt_params* prm, const rrt_debug_outputs* dbg, void* stream) {
    FrameArgs a;
    LaunchOpts o;
    const int rc = fill_args(a, o, out, width, height, time, cam, sky, fx, prm);
    if (rc) return rc;
    a.rows = rows;
    if (dbg) a.dbg = *dbg;
    return launch(a, o, dbg != nullptr, static_cast<hipStream_t>(stream));
}

/* ---- sampled launches (rrt_launch_raymarch_ss*, _mb*, _pano*, _stereo*): one kernel over the virtual (s w) x (s h) frame, static order */
bool valid_samples(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }

/* the checks of check_common plus the virtual (s w) x (s h) frame's limits; all before any device call */
int check_ss(const void* out, int width, int height, int s, const rrt_camera* cam, const rrt_effects* fx, const rrt_params* prm) {
    if (!valid_samples(s)) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = check_common(out, width, height, cam, fx, prm);
    if (rc != RRT_OK) return rc;
    if ((long long)s * width * ((long long)s * height) >= (1ll << 31)) return RRT_ERR_INVALID_ARGUMENT;
    if ((long long)s * height > (long long)kMaxGridY * kWGPixY) return RRT_ERR_INVALID_ARGUMENT;   /* 524 280 virtual rows */
    return RRT_OK;
}

/* The arguments and grid of a sampled launch: the virtual frame at times [t_lo, t_hi], `rows` in OUTPUT rows of the w x h frame
 * (grid.y == 0: nothing to launch).  The params that pick a path or an order (workspace, path_policy, pool_rounds, pass_chains,
 * tile_order) are dropped before fill_args looks at them: a sampled launch neither takes the three-pass path nor reads or records
 * a tile order.  The media mode is picked once for the interval: fill_args at both ends -- a table's window is an interval, so it
 * holds every time iff it holds both -- and the arithmetic kernels unless both found the table. */
int sampled_args(FrameArgs& a, LaunchOpts& o, dim3& grid, void* out, int width, int height, int s, const RowMap& rows, float t_lo,
                 float t_hi, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm_in) {
    rrt_params prm;
    load_params(prm_in, prm);
    prm.workspace = 0; prm.path_policy = RRT_PATH_AUTO; prm.pool_rounds = 0; prm.pass_chains = 0; prm.tile_order = 0;
    int rc = fill_args(a, o, out, s * width, s * height, t_lo, cam, sky, fx, &prm);
    if (rc) return rc;
    if (t_hi != t_lo) {
        FrameArgs a_hi;
        LaunchOpts o_hi;
        rc = fill_args(a_hi, o_hi, out, s * width, s * height, t_hi, cam, sky, fx, &prm);
        if (rc) return rc;
        if (o.media != o_hi.media) {                /* some time outside the window: every sub-frame hashes arithmetically */
            o.media = 1;
            memset(&a.lut_acc, 0, sizeof(a.lut_acc)); memset(&a.lut_dust, 0, sizeof(a.lut_dust)); memset(&a.dust_bands, 0, sizeof(a.dust_bands));
        }
    }
    a.rows = rows;
    grid = dim3((a.width + kWGPixX - 1) / kWGPixX, (s * rows.n_local_rows + kWGPixY - 1) / kWGPixY);
    return RRT_OK;
}

/* ---- motion-blurred launches (rrt_launch_raymarch_mb*): supersampled sub-frames at n_times (time, camera) pairs, one kernel */
bool valid_times(int n) { return n == 1 || n == 2 || n == 4 || n == 8 || n == 16; }
static_assert(kMaxTimes == 16, "valid_times and MotionArgs agree on the largest n_times");

/* the checks of check_ss plus the sub-frames' own; all before any device call */
int check_mb(const void* out, int width, int height, int s, int n_times, const float* times, const rrt_camera* cams,
             const rrt_effects* fx, const rrt_params* prm) {
    if (!valid_times(n_times) || !times || !cams) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = check_ss(out, width, height, s, cams, fx, prm);
    if (rc != RRT_OK) return rc;
    for (int k = 0; k < n_times; ++k)
        if (!std::isfinite(times[k])) return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}

/* launch_ss with n sub-frames, over the span of their times; with Launch = LensLaunch (rrt_launch_raymarch_dof*), each through its
 * own point (lens_xy[2k], lens_xy[2k + 1]) of a thin lens focused at `focus`.  A LensLaunch reads all 2n of lens_xy and divides by
 * focus: its callers have passed check_dof (lens_xy non-null and finite, focus > 0); a MotionLaunch looks at neither. */
template <class Launch = MotionLaunch>
int launch_mb(void* out, float4* hdr, int width, int height, int s, const RowMap& rows, int n, const float* times,
              const rrt_camera* cams, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm_in, hipStream_t st,
              const float* lens_xy = nullptr, float focus = 0.0f) {
    constexpr bool kLens = std::is_same<Launch, LensLaunch>::value;
    float t_lo = times[0], t_hi = times[0];
    Launch L;
    auto& m = L.m;
    for (int k = 0; k < kMaxTimes; ++k) {           /* the unused slots repeat the last sub-frame: no uninitialised kernel argument */
        const int j = k < n ? k : n - 1;
        m.time[k] = times[j];
        m.cam[k] = cams[j];
        if constexpr (kLens) {
            m.lx[k] = lens_xy[2 * j]; m.ly[k] = lens_xy[2 * j + 1];
            m.cx[k] = m.lx[k] / focus; m.cy[k] = m.ly[k] / focus;
        }
        if (times[j] < t_lo) t_lo = times[j];
        if (times[j] > t_hi) t_hi = times[j];
    }
    LaunchOpts o;
    dim3 grid;
    const int rc = sampled_args(L.a, o, grid, out, width, height, s, rows, t_lo, t_hi, &cams[0], sky, fx, prm_in);
    if (rc || grid.y == 0) return rc;
    L.s = s; L.n = n; L.hdr_out = hdr;
    dispatch_kernel(L.a.spin != 0.0f, o.media, o.arith, [&](auto S, auto M, auto F) {
        if constexpr (kLens) hipLaunchKernelGGL((lens_pixels<S, M, F>), grid, dim3(kWGThreads), 0, st, L);
        else hipLaunchKernelGGL((motion_pixels<S, M, F>), grid, dim3(kWGThreads), 0, st, L);
    });
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

/* ---- depth of field (rrt_launch_raymarch_dof*): launch_mb's sub-frames, each through its own point of a thin lens, one kernel */
/* the checks of check_mb plus the lens's own; all before any device call */
int check_dof(const void* out, int width, int height, int s, int n_samples, const float* times, const rrt_camera* cams,
              const float* lens_xy, float focus, const rrt_effects* fx, const rrt_params* prm) {
    if (!lens_xy || !std::isfinite(focus) || !(focus > 0.0f)) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = check_mb(out, width, height, s, n_samples, times, cams, fx, prm);
    if (rc != RRT_OK) return rc;
    for (int k = 0; k < 2 * n_samples; ++k)
        if (!std::isfinite(lens_xy[k])) return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}

/* ---- panoramas (rrt_launch_raymarch_pano*, rrt_projection_ray): supersampled frames with the projection's primary ray */
/* the projection's own refusals (include/rrt.h); a pinhole's spans are not looked at */
int check_projection(const rrt_projection* p) {
    if (!p) return RRT_ERR_INVALID_ARGUMENT;
    if (p->struct_size != (uint32_t)sizeof(rrt_projection)) return RRT_ERR_ABI_MISMATCH;
    const bool span_ok = std::isfinite(p->fov_deg) && p->fov_deg > 0.0f && p->fov_deg <= 360.0f;
    if (p->kind == RRT_PROJ_PINHOLE) return RRT_OK;
    if (p->kind == RRT_PROJ_FISHEYE) return span_ok ? RRT_OK : RRT_ERR_INVALID_ARGUMENT;
    if (p->kind == RRT_PROJ_EQUIRECT)
        return span_ok && std::isfinite(p->vfov_deg) && p->vfov_deg > 0.0f && p->vfov_deg <= 180.0f ? RRT_OK : RRT_ERR_INVALID_ARGUMENT;
    return RRT_ERR_INVALID_ARGUMENT;
}
/* the kernel's constants: half-spans in radians, rounded once from double */
ProjArgs proj_args(const rrt_projection& p) {
    ProjArgs pj;
    pj.kind = p.kind;
    pj.a_h = (float)((double)p.fov_deg * 3.14159265358979323846 / 360.0);
    pj.a_v = (float)((double)p.vfov_deg * 3.14159265358979323846 / 360.0);
    return pj;
}

int check_pano(const void* out, int width, int height, int s, const rrt_projection* proj, const rrt_camera* cam, const rrt_effects* fx,
               const rrt_params* prm) {
    const int rc = check_projection(proj);
    if (rc != RRT_OK) return rc;
    return check_ss(out, width, height, s, cam, fx, prm);
}

/* ---- stereo frames (rrt_launch_raymarch_stereo*, rrt_stereo_ray): both eyes' supersampled frames in one composite */
bool valid_layout(int layout) { return layout == RRT_STEREO_TOP_BOTTOM || layout == RRT_STEREO_SIDE_BY_SIDE; }

/* the refusals of the projection (no fisheye) and of the stereo settings (include/rrt.h) */
int check_stereo(const rrt_projection* p, const rrt_stereo* st) {
    int rc = check_projection(p);
    if (rc != RRT_OK) return rc;
    if (p->kind == RRT_PROJ_FISHEYE || !st) return RRT_ERR_INVALID_ARGUMENT;
    if (st->struct_size != (uint32_t)sizeof(rrt_stereo)) return RRT_ERR_ABI_MISMATCH;
    if (!valid_layout(st->layout)) return RRT_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(st->base) || !(st->base >= 0.0f) || !std::isfinite(st->convergence) || !(st->convergence >= 0.0f))
        return RRT_ERR_INVALID_ARGUMENT;
    const float from = st->pole_merge_from_deg, to = st->pole_merge_to_deg;
    if (!std::isfinite(from) || !std::isfinite(to) || !(from >= 0.0f) || !(from <= to) || !(to <= 90.0f)) return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}
/* the composite's output size of a width x height eye (false: it does not fit an int) */
bool composite_size(const rrt_stereo& st, int width, int height, int& cw, int& ch) {
    const long long w = (long long)width * (st.layout == RRT_STEREO_SIDE_BY_SIDE ? 2 : 1);
    const long long h = (long long)height * (st.layout == RRT_STEREO_TOP_BOTTOM ? 2 : 1);
    if (w > INT_MAX || h > INT_MAX) return false;
    cw = (int)w; ch = (int)h;
    return true;
}
/* the checks of check_stereo, then check_ss on the composite; all before any device call */
int check_stereo_launch(const void* out, int width, int height, int s, const rrt_projection* proj, const rrt_stereo* st,
                        const rrt_camera* cam, const rrt_effects* fx, const rrt_params* prm, int& cw, int& ch) {
    const int rc = check_stereo(proj, st);
    if (rc != RRT_OK) return rc;
    if (width <= 0 || height <= 0 || !composite_size(*st, width, height, cw, ch)) return RRT_ERR_INVALID_ARGUMENT;
    return check_ss(out, cw, ch, s, cam, fx, prm);
}
/* the kernel's constants of an eye's (s w) x (s h) virtual frame: hb, the merge latitudes and the pinhole's k and c per eye, all
 * rounded on the host (include/rrt.h) */
StereoArgs stereo_args(const rrt_stereo& st, int eye_w, int eye_h) {
    StereoArgs sa;
    sa.W = eye_w; sa.H = eye_h;
    sa.right_x = st.layout == RRT_STEREO_SIDE_BY_SIDE ? eye_w : 0;
    sa.right_y = st.layout == RRT_STEREO_TOP_BOTTOM ? eye_h : 0;
    sa.hb = (float)(0.5 * (double)st.base);
    sa.from = (float)((double)st.pole_merge_from_deg * 3.14159265358979323846 / 180.0);
    sa.to = (float)((double)st.pole_merge_to_deg * 3.14159265358979323846 / 180.0);
    sa.k_left = -sa.hb; sa.k_right = sa.hb;
    sa.c_left = st.convergence != 0.0f ? sa.k_left / st.convergence : 0.0f;
    sa.c_right = st.convergence != 0.0f ? sa.k_right / st.convergence : 0.0f;
    return sa;
}

/* A supersampled frame (proj NULL or a pinhole: supersample_pixels), a panorama (panorama_pixels: projection_dir instead of
 * primary_ray; the lens and the vignette are cleared, the contract ignores them), or -- stereo not NULL -- a stereo composite of
 * width x height eyes (stereo_pixels; `rows` in the composite's output rows; equirect clears the lens and the vignette too) */
int launch_ss(void* out, float4* hdr, int width, int height, int s, const RowMap& rows, const rrt_projection* proj, float time,
              const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm_in, hipStream_t st,
              const rrt_stereo* stereo = nullptr) {
    FrameArgs a;
    LaunchOpts o;
    dim3 grid;
    int cw = width, ch = height;
    if (stereo && !composite_size(*stereo, width, height, cw, ch)) return RRT_ERR_INVALID_ARGUMENT;
    const int rc = sampled_args(a, o, grid, out, cw, ch, s, rows, time, time, cam, sky, fx, prm_in);
    if (rc || grid.y == 0) return rc;
    const bool pano = proj && proj->kind != RRT_PROJ_PINHOLE;
    const ProjArgs pj = pano || stereo ? proj_args(*proj) : ProjArgs{};
    const StereoArgs sa = stereo ? stereo_args(*stereo, s * width, s * height) : StereoArgs{};
    if (pano) { a.use_lens = 0; a.use_vignette = 0; }
    dispatch_kernel(a.spin != 0.0f, o.media, o.arith, [&](auto S, auto M, auto F) {
        if (stereo) hipLaunchKernelGGL((stereo_pixels<S, M, F>), grid, dim3(kWGThreads), 0, st, a, s, hdr, pj, sa);
        else if (pano) hipLaunchKernelGGL((panorama_pixels<S, M, F>), grid, dim3(kWGThreads), 0, st, a, s, hdr, pj);
        else hipLaunchKernelGGL((supersample_pixels<S, M, F>), grid, dim3(kWGThreads), 0, st, a, s, hdr);
    });
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

int shard_rows(int height, int tile_rows, int shard, int n_shards) {
    int n_tiles = (height + tile_rows - 1) / tile_rows;
    int rows = 0;
    for (int t = shard; t < n_tiles; t += n_shards) rows += (t * tile_rows + tile_rows <= height) ? tile_rows : (height - t * tile_rows);
    return rows;
}
/* the whole frame, bottom-up */
RowMap frame_rows(int height) { return RowMap{height, 0, height, 0, 1, nullptr}; }
/* shard `shard` of n_shards: tiles of tile_rows rows, dealt round-robin */
int shard_map(int height, int tile_rows, int shard, int n_shards, RowMap& m) {
    if (tile_rows <= 0 || n_shards <= 0 || shard < 0 || shard >= n_shards) return RRT_ERR_INVALID_ARGUMENT;
    m = RowMap{shard_rows(height, tile_rows, shard, n_shards), 0, tile_rows, shard, n_shards, nullptr};
    return RRT_OK;
}

/* ---- adaptive supersampling (rrt_launch_raymarch_adaptive, rrt_adaptive_mask): the 1x frame, then only its aliasing pixels at s x s */
int check_adaptive(const rrt_adaptive* ad) {
    if (!ad) return RRT_ERR_INVALID_ARGUMENT;
    if (ad->struct_size != (uint32_t)sizeof(rrt_adaptive)) {
        snprintf(g_hip_err, sizeof(g_hip_err), "rrt_adaptive.struct_size %u, this library's is %zu: recompile against include/rrt.h",
                 ad->struct_size, sizeof(rrt_adaptive));
        return RRT_ERR_ABI_MISMATCH;
    }
    return ad->threshold >= 0 && ad->threshold <= 255 ? RRT_OK : RRT_ERR_INVALID_ARGUMENT;
}
bool adaptive_frame_ok(int width, int height) {
    return width > 0 && height > 0 && (int64_t)width * (int64_t)height < ((int64_t)1 << 31);
}

/* base pass -> zero -> mask -> refine, a linear chain on `st`: no synchronisation, allocation or memset (the counter is zeroed by
 * zero_words, like the workspace's header).  The refine pass overwrites out / hdr in place; stream order puts it behind the
 * mask pass, which is the last reader of the base bytes.  The host does not know the count: the refine grid covers width*height
 * list entries and the waves past the device-side count leave on one scalar load. */
int launch_adaptive(void* out, float4* hdr, int width, int height, int s, const rrt_projection* proj, const rrt_adaptive& ad,
                    float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm_in,
                    void* scratch, hipStream_t st) {
    FrameArgs a;
    LaunchOpts o;
    dim3 unused;
    /* the s x s virtual frame's arguments first: whatever _ss refuses for it fails here, before the base pass is enqueued
     * (launch_ss builds its own for s = 1) */
    int rc = sampled_args(a, o, unused, out, width, height, s, frame_rows(height), time, time, cam, sky, fx, prm_in);
    if (rc) return rc;
    if ((rc = launch_ss(out, hdr, width, height, 1, frame_rows(height), proj, time, cam, sky, fx, prm_in, st))) return rc;
    unsigned* count = static_cast<unsigned*>(scratch);
    unsigned* list = reinterpret_cast<unsigned*>(static_cast<uint8_t*>(scratch) + kAdaptiveListOffset);
    hipLaunchKernelGGL(zero_words, dim3(1), dim3(256), 0, st, static_cast<uint4*>(scratch), kAdaptiveListOffset / 16);
    const unsigned tiles = (unsigned)((width + kMaskTile - 1) / kMaskTile) * (unsigned)((height + kMaskTile - 1) / kMaskTile);
    hipLaunchKernelGGL(adaptive_mask, dim3((tiles + kMaskWaves - 1) / kMaskWaves), dim3(64 * kMaskWaves), 0, st,
                       static_cast<const uint8_t*>(out), width, height, ad.threshold, count, list);
    const bool pano = proj && proj->kind != RRT_PROJ_PINHOLE;
    const ProjArgs pj = pano ? proj_args(*proj) : ProjArgs{};
    if (pano) { a.use_lens = 0; a.use_vignette = 0; }
    const RefineArgs ra{count, list, hdr, s};
    const unsigned long long slots = (unsigned long long)((kTileW / s) * (kTileW / s)) * kWGWaves;       /* per workgroup */
    const unsigned long long groups = ((unsigned long long)width * height + slots - 1) / slots;
    const unsigned gx = (unsigned)std::min<unsigned long long>(groups, 1ull << 20);
    const dim3 grid(gx, (unsigned)((groups + gx - 1) / gx));
    dispatch_kernel(a.spin != 0.0f, o.media, o.arith, [&](auto S, auto M, auto F) {
        if (pano) hipLaunchKernelGGL((refine_pixels<S, M, F, kRayProjection>), grid, dim3(kWGThreads), 0, st, a, ra, pj);
        else hipLaunchKernelGGL((refine_pixels<S, M, F, kRayPinhole>), grid, dim3(kWGThreads), 0, st, a, ra, pj);
    });
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

/* ---- HDR glow (rrt_launch_glow): the lobes' taps in double, the checks, the three launches */
struct GlowPlan {
    int lobes, rmax, n_weights;
    int radius[kGlowMaxLobes], woff[kGlowMaxLobes];
    double sigma[kGlowMaxLobes];
};

/* the settings' checks and the lobes' sigma_l = (radius * height) * 2^l, R_l = ceil(3 sigma_l); all on the host */
int glow_plan(const rrt_glow* g, int height, GlowPlan& p) {
    if (!g) return RRT_ERR_INVALID_ARGUMENT;
    if (g->struct_size != (uint32_t)sizeof(rrt_glow)) {
        snprintf(g_hip_err, sizeof(g_hip_err), "rrt_glow.struct_size %u, this library's is %zu: recompile against include/rrt.h",
                 g->struct_size, sizeof(rrt_glow));
        return RRT_ERR_ABI_MISMATCH;
    }
    if (g->lobes < 1 || g->lobes > kGlowMaxLobes || height <= 0) return RRT_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(g->radius) || !(g->radius > 0.0f)) return RRT_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(g->threshold) || g->threshold < 0.0f) return RRT_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(g->intensity) || g->intensity < 0.0f) return RRT_ERR_INVALID_ARGUMENT;
    p.lobes = g->lobes;
    p.n_weights = 0;
    for (int l = 0; l < p.lobes; ++l) {
        const double sigma = ((double)g->radius * (double)height) * (double)(1 << l);
        const double r = std::ceil(3.0 * sigma);
        if (!(r <= (double)kGlowMaxRadius)) return RRT_ERR_INVALID_ARGUMENT;
        p.sigma[l] = sigma;
        p.radius[l] = (int)r;
        p.woff[l] = p.n_weights;
        p.n_weights += 2 * p.radius[l] + 1;
    }
    p.rmax = p.radius[p.lobes - 1];
    return RRT_OK;
}

/* w[k + R] = exp(-k^2 / (2 sigma^2)) / sum_j exp(-j^2 / (2 sigma^2)), in double (the sum over ascending j), rounded to float */
void glow_taps_host(double sigma, int r, float* out) {
    const double d = 2.0 * sigma * sigma;
    double sum = 0.0;
    for (int j = -r; j <= r; ++j) sum += std::exp(-(double)j * (double)j / d);
    for (int k = -r; k <= r; ++k) out[k + r] = (float)(std::exp(-(double)k * (double)k / d) / sum);
}

size_t glow_weight_bytes(const GlowPlan& p) { return ((size_t)p.n_weights * sizeof(float) + 15) & ~(size_t)15; }
size_t glow_scratch(const GlowPlan& p, int width, int height) {
    return glow_weight_bytes(p) + (size_t)p.lobes * (size_t)width * (size_t)height * sizeof(float4);
}
bool glow_frame_ok(int width, int height) {
    return width > 0 && height > 0 && (int64_t)width * (int64_t)height < ((int64_t)1 << 31);
}

int launch_glow(uchar4* out, const float4* hdr, int width, int height, const rrt_glow* g, const GlowPlan& p, void* scratch,
                hipStream_t st) {
    float* weights = static_cast<float*>(scratch);
    std::vector<float> taps(p.n_weights);
    for (int l = 0; l < p.lobes; ++l) glow_taps_host(p.sigma[l], p.radius[l], taps.data() + p.woff[l]);
    for (int off = 0; off < p.n_weights; off += kGlowWeightChunk) {
        GlowWeightChunk c;
        c.offset = off;
        c.count = std::min(kGlowWeightChunk, p.n_weights - off);
        memcpy(c.w, taps.data() + off, c.count * sizeof(float));
        memset(c.w + c.count, 0, (kGlowWeightChunk - c.count) * sizeof(float));
        hipLaunchKernelGGL(glow_load_weights, dim3(1), dim3(256), 0, st, weights, c);
    }
    GlowArgs a;
    memset(&a, 0, sizeof(a));
    a.hdr = hdr;
    a.planes = reinterpret_cast<float4*>(static_cast<uint8_t*>(scratch) + glow_weight_bytes(p));
    a.weights = weights;
    a.out = out;
    a.width = width; a.height = height; a.lobes = p.lobes; a.rmax = p.rmax;
    a.seg = glow_seg(p.rmax);
    for (int l = 0; l < p.lobes; ++l) { a.radius[l] = p.radius[l]; a.woff[l] = p.woff[l]; }
    a.threshold = g->threshold;
    a.scale = g->intensity / (float)p.lobes;
    const int n_seg = (width + a.seg - 1) / a.seg;
    hipLaunchKernelGGL((glow_hpass<kGlowM>), dim3(n_seg * height), dim3(kGlowHThreads), glow_hpass_lds(a.seg, p.rmax), st, a);
    const int n_yb = (height + kGlowVWaves * kGlowM - 1) / (kGlowVWaves * kGlowM), n_strips = (width + 63) / 64;
    hipLaunchKernelGGL((glow_vpass<kGlowM>), dim3(n_yb * n_strips), dim3(64, kGlowVWaves), 0, st, a);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

/* ---- exposure control (rrt_launch_exposure): the settings' checks, the bin centres, the launches */
static_assert(sizeof(rrt_exposure) == 40, "rrt_exposure layout");
static_assert(RRT_EXPOSURE_HIST_OFFSET == kExposureHistOffset && RRT_EXPOSURE_STATE_OFFSET == kExposureStateOffset &&
              RRT_EXPOSURE_TABLE_OFFSET == kExposureTableOffset, "the scratch layout include/rrt.h documents");
int check_exposure(const rrt_exposure* e) {
    if (!e) return RRT_ERR_INVALID_ARGUMENT;
    if (e->struct_size != (uint32_t)sizeof(rrt_exposure)) {
        snprintf(g_hip_err, sizeof(g_hip_err), "rrt_exposure.struct_size %u, this library's is %zu: recompile against include/rrt.h",
                 e->struct_size, sizeof(rrt_exposure));
        return RRT_ERR_ABI_MISMATCH;
    }
    if (e->mode != RRT_EXPOSURE_MANUAL && e->mode != RRT_EXPOSURE_AUTO) return RRT_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(e->ev) || !std::isfinite(e->key) || !(e->key > 0.0f)) return RRT_ERR_INVALID_ARGUMENT;
    if (e->low_permille < 0 || e->high_permille < 0 || (int64_t)e->low_permille + (int64_t)e->high_permille >= 1000)
        return RRT_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(e->min_ev) || !std::isfinite(e->max_ev) || !(e->min_ev <= e->max_ev)) return RRT_ERR_INVALID_ARGUMENT;
    if (!(e->adapt_up > 0.0f && e->adapt_up <= 1.0f) || !(e->adapt_down > 0.0f && e->adapt_down <= 1.0f)) return RRT_ERR_INVALID_ARGUMENT;
    return RRT_OK;
}
bool exposure_scratch_ok(const void* scratch, size_t bytes) {
    return scratch && !(reinterpret_cast<uintptr_t>(scratch) & 15) && bytes >= kExposureScratchBytes;
}

/* auto: zero -> meter -> resolve -> apply, a linear chain on `st` (the histogram is zeroed by zero_words, like the adaptive list's
 * counter: no memset node); manual: the apply pass alone, the scale computed here by the function the resolve pass runs */
int launch_exposure(uchar4* out8, float4* hdr_out, const float4* hdr_in, int width, int height, const rrt_exposure& e, void* scratch,
                    hipStream_t st) {
    const size_t n = (size_t)width * (size_t)height;
    const dim3 apply_grid((unsigned)((n + 255) / 256));
    if (e.mode == RRT_EXPOSURE_MANUAL) {
        hipLaunchKernelGGL(exposure_apply, apply_grid, dim3(256), 0, st, out8, hdr_out, hdr_in, n,
                           static_cast<const ExposureState*>(nullptr), rrt_expf(e.ev * 0.693147182f));
        RRT_HIP(hipGetLastError());
        return RRT_OK;
    }
    uint8_t* base = static_cast<uint8_t*>(scratch);
    unsigned* hist = reinterpret_cast<unsigned*>(base + kExposureHistOffset);
    ExposureState* state = reinterpret_cast<ExposureState*>(base + kExposureStateOffset);
    const double* table = reinterpret_cast<const double*>(base + kExposureTableOffset);
    ExposureMeter s;
    s.log2_key = std::log2((double)e.key);
    s.ev = e.ev; s.min_ev = e.min_ev; s.max_ev = e.max_ev; s.adapt_up = e.adapt_up; s.adapt_down = e.adapt_down;
    s.low_permille = e.low_permille; s.high_permille = e.high_permille;
    hipLaunchKernelGGL(zero_words, dim3(1), dim3(256), 0, st, reinterpret_cast<uint4*>(hist), kExposureBins * sizeof(uint32_t) / 16);
    hipLaunchKernelGGL(exposure_meter, dim3(exposure_meter_groups(n)), dim3(kMeterThreads), 0, st, hdr_in, n, hist);
    hipLaunchKernelGGL(exposure_resolve, dim3(1), dim3(64), 0, st, hist, state, table, s);
    hipLaunchKernelGGL(exposure_apply, apply_grid, dim3(256), 0, st, out8, hdr_out, hdr_in, n, state, 0.0f);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

/* ---- workspace counters (rrt_workspace_stats, _rounds) */
hipError_t read_chain_counters(const WorkspaceObject& w, DeferCounters* out) {
    uint8_t raw[kMaxChains * kCounterStride];
    const hipError_t e = hipMemcpy(raw, w.d_base, sizeof(raw), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (int k = 0; k < kMaxChains; ++k) memcpy(&out[k], raw + (size_t)k * kCounterStride, sizeof(DeferCounters));
    return hipSuccess;
}

/* rrt_launch_auto_resources (round 6): the objects the library owns on behalf of a host that only ever calls the
 * reference-signature launch_raymarch() */
struct AutoResources {
    bool on = false;
    int device = -1;
    int pool = 0, order = 0, table = 0;
    size_t table_budget = 0;
    float t0 = 0.0f, t1 = -1.0f;           /* the window the table (or the remembered "nothing fits") covers; empty at first */
    int table_builds = 0;
    rrt_params base;
};
std::mutex g_auto_mu;
AutoResources g_auto;

void auto_release_locked() {
    if (g_auto.table) rrt_noise_table_destroy(g_auto.table);
    if (g_auto.order) rrt_tile_order_destroy(g_auto.order);
    if (g_auto.pool) rrt_workspace_destroy(g_auto.pool);
    g_auto = AutoResources();
}

/* the parameters of one launch_raymarch() call under auto resources; slides the table's window when `time` has left it */
bool auto_params(float time, rrt_params& prm) {
    std::lock_guard<std::mutex> lk(g_auto_mu);
    if (!g_auto.on) return false;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != g_auto.device) return false;       /* another device is current: plain defaults */
    if (g_auto.table_budget > 0 && g_auto.base.volumetrics && !(time >= g_auto.t0 && time <= g_auto.t1)) {
        /* The one place a launch_raymarch() call waits for the device and allocates -- opted into by the caller: the frames that
         * may still read the old table drain, the next window is fitted to the budget and built (milliseconds). */
        (void)hipDeviceSynchronize();
        if (g_auto.table) { rrt_noise_table_destroy(g_auto.table); g_auto.table = 0; }
        float t1 = time; int cov = RRT_TABLE_FULL; size_t bytes = 0;
        rrt_noise_table_fit_window(time, time + 120.0f, g_auto.table_budget, &t1, &cov, &bytes);
        if (bytes != 0 && rrt_noise_table_create_window(time, t1, cov, &g_auto.table) == RRT_OK) ++g_auto.table_builds;
        else { g_auto.table = 0; if (bytes == 0) t1 = time + 5.0f; }                  /* nothing fits / no memory: look again after 5 s */
        g_auto.t0 = time; g_auto.t1 = t1;
    }
    prm = g_auto.base;
    prm.workspace = g_auto.pool; prm.tile_order = g_auto.order; prm.noise_table = g_auto.table;
    return true;
}

}  // namespace

/* ====================================================================== C ABI */
extern "C" {

int rrt_abi_version(void) { return RRT_ABI_VERSION; }

/* RRT_PATH_AUTO's threshold, for hosts that size their own policy on it (the drivers leave rrt_tile_order off for launches
 * that will take the three-pass path): one definition instead of a copy in every driver */
int rrt_path_auto_max_rays(void) { return (int)kThreePassMaxRays; }

const char* rrt_status_string(int s) {
    switch (s) {
        case RRT_OK: return "ok";
        case RRT_ERR_INVALID_ARGUMENT: return "invalid argument";
        case RRT_ERR_NO_DEVICE: return "no HIP device";
        case RRT_ERR_HIP: return "HIP runtime error";
        case RRT_ERR_BAD_HANDLE: return "bad handle (sky, workspace, noise table, tile order or tile map)";
        case RRT_ERR_OUT_OF_MEMORY: return "out of memory";
        case RRT_ERR_ABI_MISMATCH: return "rrt_params from another ABI version (recompile against include/rrt.h)";
        default: return "unknown status";
    }
}

const char* rrt_last_hip_error(void) { return g_hip_err; }

int rrt_device_count(int* count) {
    if (!count) return RRT_ERR_INVALID_ARGUMENT;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return RRT_ERR_NO_DEVICE; }
    *count = n;
    return n > 0 ? RRT_OK : RRT_ERR_NO_DEVICE;
}

int rrt_params_init(void* p, uint32_t size) {
    if (!p) return RRT_ERR_INVALID_ARGUMENT;
    if (size != (uint32_t)sizeof(rrt_params) && size != kParamsSizeAbi4) return RRT_ERR_ABI_MISMATCH;
    rrt_params d;
    memset(&d, 0, sizeof(d));
    d.spin = 0.0f;          /* SPIN_A    config.h:21 */
    d.max_steps = 2000;     /* MAX_STEPS config.h:48 */
    d.volumetrics = 1;
    d.sky_frac_bits = 8;
    d.struct_size = size;
    memcpy(p, &d, size);
    return RRT_OK;
}

/* what binaries built against the ABI 4 header call: that header's struct is the first 48 bytes of today's, and such a
 * struct is still accepted by every entry point (check_params_abi) */
int rrt_params_default_v4(void* abi4_48) { return rrt_params_init(abi4_48, kParamsSizeAbi4); }

/* The symbol binaries built against the ABI <= 3 header call: it fills the 36 bytes THEIR struct has -- spin, max_steps,
 * volumetrics, sky_frac_bits, arith_mode, workspace, path_policy, noise_table, tile_order -- and not a byte more, so such
 * a binary is refused at its first launch (RRT_ERR_ABI_MISMATCH: its first word is `spin`, not a struct size) instead of
 * having its stack overwritten here. */
#pragma push_macro("rrt_params_default")
#undef rrt_params_default
int rrt_params_default(void* legacy36) {
    if (!legacy36) return RRT_ERR_INVALID_ARGUMENT;
    int32_t w[9] = {0, 2000, 1, 8, 0, 0, 0, 0, 0};
    memcpy(legacy36, w, sizeof(w));
    return RRT_OK;
}
#pragma pop_macro("rrt_params_default")

int rrt_effects_default(rrt_effects* e) {    /* camera_settings.h:5-16 */
    if (!e) return RRT_ERR_INVALID_ARGUMENT;
    memset(e, 0, sizeof(*e));
    e->use_bloom = 1; e->bloom_threshold = 0.8f; e->bloom_intensity = 0.5f;
    e->use_vignette = 1; e->vignette_intensity = 0.4f;
    e->use_chromatic_aberration = 0; e->ca_amount = 0.005f;
    e->use_lens_distortion = 1; e->distortion_amount = 0.15f;
    return RRT_OK;
}

int rrt_sky_create(const uint8_t* rgba8_host, int width, int height, rrt_sky_t* out) {
    if (!rgba8_host || !out || width <= 0 || height <= 0) return RRT_ERR_INVALID_ARGUMENT;
    SkyObject s{nullptr, width, height, true, current_device()};
    size_t bytes = (size_t)width * height * 4;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&s.d_texels), bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(sky)");
    e = hipMemcpy(s.d_texels, rgba8_host, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(s.d_texels); return hip_fail(e, "hipMemcpy(sky)"); }
    *out = g_skies.insert(s);
    return RRT_OK;
}

int rrt_sky_create_from_device(const void* d_rgba8, int width, int height, rrt_sky_t* out) {
    if (!d_rgba8 || !out || width <= 0 || height <= 0) return RRT_ERR_INVALID_ARGUMENT;
    /* the device that owns the caller's allocation, if the runtime can tell; else the current one */
    int device = current_device();
    hipPointerAttribute_t attr;
    if (faked_device() < 0 && hipPointerGetAttributes(&attr, d_rgba8) == hipSuccess) device = attr.device;
    else (void)hipGetLastError();
    SkyObject s{const_cast<uint8_t*>(static_cast<const uint8_t*>(d_rgba8)), width, height, false, device};
    *out = g_skies.insert(s);
    return RRT_OK;
}

int rrt_sky_destroy(rrt_sky_t sky) {
    SkyObject s;
    if (g_skies.take(sky, s)) return RRT_ERR_BAD_HANDLE;
    if (s.owned) {
        hipError_t e = hipFree(s.d_texels);
        if (e != hipSuccess) return hip_fail(e, "hipFree(sky)");
    }
    return RRT_OK;
}

int rrt_workspace_create(size_t bytes, int* out) {
    if (!out || bytes < (size_t)1 << 20) return RRT_ERR_INVALID_ARGUMENT;
    WorkspaceObject w{nullptr, bytes, current_device(), nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&w.d_base), bytes);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(workspace)");
    e = hipHostMalloc(reinterpret_cast<void**>(&w.h_stats), kMaxChains * sizeof(DeferCounters), hipHostMallocDefault);
    if (e != hipSuccess) { (void)hipFree(w.d_base); return hip_fail(e, "hipHostMalloc(workspace statistics)"); }
    memset(w.h_stats, 0, kMaxChains * sizeof(DeferCounters));
    /* the second chain's stream and the fork / join events; without them launches run one chain.  Default priority on
     * purpose: a higher-priority stream is served STRICTLY first on this hardware -- the other queue did not start until the
     * whole high-priority chain had finished (kernel trace, profiles/README.md round 4): serial again, and slower */
    if (hipStreamCreateWithFlags(&w.side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&w.forked, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&w.joined, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        if (w.side) (void)hipStreamDestroy(w.side);
        if (w.forked) (void)hipEventDestroy(w.forked);
        w.side = nullptr; w.forked = nullptr; w.joined = nullptr;
    }
    *out = g_workspaces.insert(w);
    return RRT_OK;
}

int rrt_workspace_destroy(int id) {
    WorkspaceObject w;
    if (g_workspaces.take(id, w)) return RRT_ERR_BAD_HANDLE;
    if (w.side) { (void)hipStreamSynchronize(w.side); (void)hipStreamDestroy(w.side); }
    if (w.forked) (void)hipEventDestroy(w.forked);
    if (w.joined) (void)hipEventDestroy(w.joined);
    hipError_t e = hipFree(w.d_base);
    if (w.h_stats) (void)hipHostFree(w.h_stats);
    if (e != hipSuccess) return hip_fail(e, "hipFree(workspace)");
    return RRT_OK;
}

int rrt_workspace_stats(int id, unsigned* rows_used, unsigned* overflow_waves) {
    WorkspaceObject w;
    if (lookup_here(g_workspaces, id, w)) return RRT_ERR_BAD_HANDLE;
    DeferCounters c[kMaxChains];
    RRT_HIP(read_chain_counters(w, c));
    unsigned long long rows = 0; unsigned left = 0;
    for (int k = 0; k < kMaxChains; ++k) { rows += c[k].total_blocks * kBlockRows; left += c[k].suspended_left; }
    if (rows_used) *rows_used = rows > 0xffffffffull ? 0xffffffffu : (unsigned)rows;
    if (overflow_waves) *overflow_waves = left;
    return RRT_OK;
}

int rrt_workspace_rounds(int id, unsigned* rounds_enqueued, unsigned* rounds_with_work, unsigned* peak_rows, unsigned* pool_rows) {
    WorkspaceObject w;
    if (lookup_here(g_workspaces, id, w)) return RRT_ERR_BAD_HANDLE;
    DeferCounters c[kMaxChains];
    RRT_HIP(read_chain_counters(w, c));
    unsigned run = 0, work = 0, peak = 0;
    for (int k = 0; k < kMaxChains; ++k) {        /* rounds: of the chain that needed most; rows of the fullest round: both chains' */
        run = c[k].rounds_run > run ? c[k].rounds_run : run;
        work = c[k].rounds_with_work > work ? c[k].rounds_with_work : work;
        peak += c[k].peak_blocks;
    }
    if (rounds_enqueued) *rounds_enqueued = run;
    if (rounds_with_work) *rounds_with_work = work;
    if (peak_rows) *peak_rows = peak * kBlockRows;
    if (pool_rows) *pool_rows = (unsigned)((w.bytes / kBlockBytes) * kBlockRows);      /* upper bound: before the launch's bookkeeping */
    return RRT_OK;
}

int rrt_workspace_read(int id, size_t offset, size_t bytes, void* host_dst) {
    WorkspaceObject w;
    if (!g_workspaces.get(id, w)) return RRT_ERR_BAD_HANDLE;
    if (!host_dst || offset > w.bytes || bytes > w.bytes - offset) return RRT_ERR_INVALID_ARGUMENT;
    if (!on_current_device(w.device)) return RRT_ERR_BAD_HANDLE;
    RRT_HIP(hipMemcpy(host_dst, w.d_base + offset, bytes, hipMemcpyDeviceToHost));
    return RRT_OK;
}

int rrt_tile_order_create(int* out) {
    if (!out) return RRT_ERR_INVALID_ARGUMENT;
    auto o = std::make_shared<TileOrderObject>();
    o->device = current_device();
    o->d_cost = o->d_sorted = o->d_iota = o->d_perm[0] = o->d_perm[1] = nullptr;
    o->d_temp = nullptr; o->temp_bytes = 0; o->n_cap = 0; o->cur = 0; o->have = false;
    o->grid_x = o->grid_y = 0; o->width = o->height = 0; o->rows = RowMap{0, 0, 1, 0, 1, nullptr};
    o->launches = o->ordered = o->seeded = 0; o->no_seed = false; o->dead = false;
    RRT_HIP(hipEventCreateWithFlags(&o->chained, hipEventDisableTiming));
    *out = g_tile_orders.insert(o);
    return RRT_OK;
}

int rrt_tile_order_destroy(int id) {
    std::shared_ptr<TileOrderObject> o;
    if (g_tile_orders.take(id, o, made_here<TileOrderObject>)) return RRT_ERR_BAD_HANDLE;
    std::lock_guard<std::mutex> lk(o->mu);                          /* after any launch that holds the object */
    o->dead = true;
    if (o->launches > 0) (void)hipEventSynchronize(o->chained);     /* its last launch and sort have finished */
    unsigned* bufs[] = {o->d_cost, o->d_sorted, o->d_iota, o->d_perm[0], o->d_perm[1]};
    for (unsigned* b : bufs) if (b) (void)hipFree(b);
    if (o->d_temp) (void)hipFree(o->d_temp);
    (void)hipEventDestroy(o->chained);
    return RRT_OK;
}

int rrt_tile_order_set_seeding(int id, int on) {
    std::shared_ptr<TileOrderObject> o;
    if (!g_tile_orders.get(id, o)) return RRT_ERR_BAD_HANDLE;
    std::lock_guard<std::mutex> lk(o->mu);
    o->no_seed = on == 0;
    return RRT_OK;
}

/* launches whose order came from the coarse probe (no history for their geometry) */
int rrt_tile_order_seeded(int id, unsigned long long* seeded_launches) {
    std::shared_ptr<TileOrderObject> o;
    if (!g_tile_orders.get(id, o)) return RRT_ERR_BAD_HANDLE;
    if (!seeded_launches) return RRT_ERR_INVALID_ARGUMENT;
    std::lock_guard<std::mutex> lk(o->mu);
    *seeded_launches = o->seeded;
    return RRT_OK;
}

/* counters of an object, and (optionally, after waiting for its last launch) the order the NEXT matching launch will
 * use plus the costs the last one recorded: perm_host / cost_host may be NULL, capacity counts elements */
int rrt_tile_order_info(int id, unsigned long long* launches, unsigned long long* ordered_launches, unsigned* n_tiles,
                        unsigned* perm_host, unsigned* cost_host, unsigned capacity) {
    std::shared_ptr<TileOrderObject> op;
    if (!g_tile_orders.get(id, op)) return RRT_ERR_BAD_HANDLE;
    std::lock_guard<std::mutex> lk(op->mu);
    const TileOrderObject& o = *op;
    if (!on_current_device(o.device)) return RRT_ERR_BAD_HANDLE;
    const unsigned n = o.have ? o.grid_x * o.grid_y : 0u;
    if (launches) *launches = o.launches;
    if (ordered_launches) *ordered_launches = o.ordered;
    if (n_tiles) *n_tiles = n;
    if ((perm_host || cost_host) && n > 0) {
        if (capacity < n) return RRT_ERR_INVALID_ARGUMENT;
        RRT_HIP(hipEventSynchronize(o.chained));
        if (perm_host) RRT_HIP(hipMemcpy(perm_host, o.d_perm[o.cur], n * sizeof(unsigned), hipMemcpyDeviceToHost));
        if (cost_host) RRT_HIP(hipMemcpy(cost_host, o.d_cost, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    }
    return RRT_OK;
}

int rrt_noise_table_create(float t_max, int* out_id) {
    if (!(t_max >= 0.0f)) return RRT_ERR_INVALID_ARGUMENT;
    return rrt_noise_table_create_window(0.0f, t_max, RRT_TABLE_FULL, out_id);
}

int rrt_noise_table_create_window(float t0, float t1, int coverage, int* out_id) {
    if (!out_id) return RRT_ERR_INVALID_ARGUMENT;
    NoiseTableObject nt;
    const int rc = plan_table(t0, t1, coverage, nt);
    if (rc != RRT_OK) return rc;
    RRT_HIP(hipGetDevice(&nt.device));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&nt.d_cells), nt.bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); snprintf(g_hip_err, sizeof(g_hip_err), "hipMalloc(noise table, %zu bytes): %s", nt.bytes, hipGetErrorString(e)); return e == hipErrorOutOfMemory ? RRT_ERR_OUT_OF_MEMORY : RRT_ERR_HIP; }
    auto fill_box = [&](const LutBox& bx, size_t cell0) {
        const size_t n = (size_t)bx.nx * bx.ny * bx.nz;
        hipLaunchKernelGGL(build_noise_table, dim3((unsigned)std::min<size_t>(4096, (n + 255) / 256)), dim3(256), 0, nullptr, nt.d_cells + cell0, bx);
    };
    auto record = [&](const LutBox& bx, unsigned cell0) {
        const NoiseLut L = make_lut(nullptr, bx, 0u);
        rrt::BandLut r;
        memset(&r, 0, sizeof(r));
        r.cell0 = cell0; r.origin = L.origin; r.nx = L.nx; r.nxy = L.nxy; r.last = L.last;
        return r;
    };
    if (!nt.banded) fill_box(nt.acc, 0);
    fill_box(nt.dust, dust_cell0(nt));
    e = hipGetLastError();
    if (e == hipSuccess && nt.banded) {
        std::vector<rrt::BandLut> recs((size_t)rrt::kBandFamilies * nt.bands.n_bands + rrt::kLutAccOctaves);
        for (int o = 0; o < rrt::kLutAccOctaves; ++o) {
            fill_box(nt.bands.acc_box[o], nt.bands.acc_cell0[o]);
            recs[(size_t)rrt::kBandFamilies * nt.bands.n_bands + o] = record(nt.bands.acc_box[o], nt.bands.acc_cell0[o]);
        }
        for (int f = 0; f < rrt::kBandFamilies; ++f)
            for (int b = 0; b < nt.bands.n_bands; ++b) {
                fill_box(nt.bands.box[f][b], nt.bands.cell0[f][b]);
                recs[(size_t)f * nt.bands.n_bands + b] = record(nt.bands.box[f][b], nt.bands.cell0[f][b]);
            }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(reinterpret_cast<char*>(nt.d_cells) + nt.bands.entries_offset, recs.data(),
                                           recs.size() * sizeof(rrt::BandLut), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { (void)hipFree(nt.d_cells); return hip_fail(e, "build_noise_table"); }
    *out_id = g_noise_tables.insert(nt);
    return RRT_OK;
}

int rrt_noise_table_destroy(int id) {
    NoiseTableObject nt;
    if (g_noise_tables.take(id, nt)) return RRT_ERR_BAD_HANDLE;
    hipError_t e = hipFree(nt.d_cells);
    if (e != hipSuccess) return hip_fail(e, "hipFree(noise table)");
    return RRT_OK;
}

int rrt_noise_table_info(int id, float* t_max, size_t* bytes, int* boxes12) {
    NoiseTableObject nt;                       /* any device: nothing of the table's memory is read */
    if (!g_noise_tables.get(id, nt)) return RRT_ERR_BAD_HANDLE;
    if (t_max) *t_max = nt.t1;
    if (bytes) *bytes = nt.bytes;
    if (boxes12) { memcpy(boxes12, &nt.acc, sizeof(LutBox)); memcpy(boxes12 + 6, &nt.dust, sizeof(LutBox)); }
    return RRT_OK;
}

int rrt_noise_table_window(int id, float* t0, float* t1, int* coverage, int* device) {
    NoiseTableObject nt;
    if (!g_noise_tables.get(id, nt)) return RRT_ERR_BAD_HANDLE;
    if (t0) *t0 = nt.t0;
    if (t1) *t1 = nt.t1;
    if (coverage) *coverage = nt.coverage | (nt.banded ? RRT_TABLE_BANDED : 0);
    if (device) *device = nt.device;
    return RRT_OK;
}

int rrt_noise_table_plan(float t_max, size_t* bytes, int* boxes12) {
    if (!(t_max >= 0.0f)) return RRT_ERR_INVALID_ARGUMENT;
    return rrt_noise_table_plan_window(0.0f, t_max, RRT_TABLE_FULL, bytes, boxes12);
}

/* boxes only (host arithmetic, no device): what rrt_noise_table_create_window would allocate, with the same
 * RRT_ERR_INVALID_ARGUMENT for a box it would refuse */
int rrt_noise_table_plan_window(float t0, float t1, int coverage, size_t* bytes, int* boxes12) {
    NoiseTableObject nt;
    const int rc = plan_table(t0, t1, coverage, nt);
    if (bytes) *bytes = rc == RRT_OK ? nt.bytes : 0;
    if (rc != RRT_OK) return rc;
    if (boxes12) { memcpy(boxes12, &nt.acc, sizeof(LutBox)); memcpy(boxes12 + 6, &nt.dust, sizeof(LutBox)); }
    return RRT_OK;
}

int rrt_noise_table_plan_layout(float t0, float t1, int coverage, int* banded, int* n_bands, float* w_min, float* w_scale,
                                int32_t* band_boxes, int cap_bands, int32_t* acc_octave_boxes) {
    if (!banded || !n_bands) return RRT_ERR_INVALID_ARGUMENT;
    NoiseTableObject nt;
    const int rc = plan_table(t0, t1, coverage, nt);
    if (rc != RRT_OK) return rc;
    *banded = nt.banded ? 1 : 0;
    *n_bands = nt.banded ? nt.bands.n_bands : 0;
    if (w_min) *w_min = nt.bands.w_min;
    if (w_scale) *w_scale = nt.bands.w_scale;
    if (nt.banded && band_boxes) {
        if (cap_bands < nt.bands.n_bands) return RRT_ERR_INVALID_ARGUMENT;
        for (int f = 0; f < rrt::kBandFamilies; ++f)
            for (int b = 0; b < nt.bands.n_bands; ++b) {
                const LutBox& bx = nt.bands.box[f][b];
                const int v[6] = {bx.x0, bx.y0, bx.z0, bx.nx, bx.ny, bx.nz};
                memcpy(band_boxes + ((size_t)f * cap_bands + b) * 6, v, sizeof(v));
            }
    }
    if (nt.banded && acc_octave_boxes)
        for (int o = 0; o < rrt::kLutAccOctaves; ++o) {
            const LutBox& bx = nt.bands.acc_box[o];
            const int v[6] = {bx.x0, bx.y0, bx.z0, bx.nx, bx.ny, bx.nz};
            memcpy(acc_octave_boxes + (size_t)o * 6, v, sizeof(v));
        }
    return RRT_OK;
}

/* The window a frame driver should build next: the longest [t_from, t1], t1 <= t_until, at the richest coverage,
 * whose table fits `budget_bytes` -- the window is halved (down to 0.5 s) before the coverage is lowered, because a
 * rebuild costs milliseconds while a coarser table costs every frame.  RRT_OK with *bytes_out == 0 when nothing fits
 * (the driver then renders without a table: same bytes, slower). */
int rrt_noise_table_fit_window(float t_from, float t_until, size_t budget_bytes, float* t1_out, int* coverage_out, size_t* bytes_out) {
    if (!t1_out || !coverage_out || !bytes_out || !(t_from <= t_until)) return RRT_ERR_INVALID_ARGUMENT;
    *t1_out = t_from; *coverage_out = RRT_TABLE_FULL; *bytes_out = 0;
    for (int cov = RRT_TABLE_FULL; cov <= RRT_TABLE_COARSEST; ++cov) {
        float span = t_until - t_from;
        for (;;) {
            NoiseTableObject nt;
            const float t1 = t_from + span;
            if (plan_table(t_from, t1, cov, nt) == RRT_OK && nt.bytes <= budget_bytes) {
                *t1_out = t1; *coverage_out = cov; *bytes_out = nt.bytes;
                return RRT_OK;
            }
            if (span <= 0.5f) break;
            span = span * 0.5f < 0.5f ? 0.5f : span * 0.5f;
        }
    }
    return RRT_OK;
}

int rrt_clock_probe(unsigned long long* d_counters2, unsigned duration_us, void* stream) {
    if (!d_counters2 || duration_us == 0 || duration_us > 2000000u) return RRT_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), d_counters2,
                       (unsigned long long)duration_us * 100ull);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

/* Parameters of the reference-signature entry point launch_raymarch() (include/raymarcher.h), which has no
 * parameter for them: config.h defaults until the application says otherwise.  Nothing is allocated here --
 * a workspace or noise table named in the defaults is created (and destroyed) by the caller. */
std::mutex g_defaults_mu;
rrt_params g_defaults;
bool g_defaults_set = false;

int rrt_set_launch_defaults(const rrt_params* prm) {
    std::lock_guard<std::mutex> lk(g_defaults_mu);
    if (!prm) { g_defaults_set = false; return RRT_OK; }
    int rc = check_params_abi(prm);
    if (rc == RRT_OK) rc = check_params_values(prm);
    if (rc != RRT_OK) return rc;
    load_params(prm, g_defaults);
    g_defaults_set = true;
    return RRT_OK;
}

int rrt_get_launch_defaults_sized(void* out, uint32_t size) {
    if (!out) return RRT_ERR_INVALID_ARGUMENT;
    if (size != (uint32_t)sizeof(rrt_params) && size != kParamsSizeAbi4) return RRT_ERR_ABI_MISMATCH;
    std::lock_guard<std::mutex> lk(g_defaults_mu);
    if (!g_defaults_set) return rrt_params_init(out, size);
    memcpy(out, &g_defaults, size);
    static_cast<rrt_params*>(out)->struct_size = size;
    return RRT_OK;
}
/* the export ABI 4 binaries call: their struct has 48 bytes */
#pragma push_macro("rrt_get_launch_defaults")
#undef rrt_get_launch_defaults
int rrt_get_launch_defaults(void* abi4_48) { return rrt_get_launch_defaults_sized(abi4_48, kParamsSizeAbi4); }
#pragma pop_macro("rrt_get_launch_defaults")

int rrt_launch_auto_resources(int on, const rrt_params* base, size_t table_budget_bytes, size_t pool_bytes) {
    std::lock_guard<std::mutex> lk(g_auto_mu);
    if (g_auto.on) {                                   /* a second call replaces the first's objects; both from their device */
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess || dev != g_auto.device) return RRT_ERR_BAD_HANDLE;
        (void)hipDeviceSynchronize();
        auto_release_locked();
    }
    if (!on) return RRT_OK;
    rrt_params b;
    rrt_params_init(&b, (uint32_t)sizeof(rrt_params));
    if (base) {
        int rc = check_params_abi(base);
        if (rc == RRT_OK) rc = check_params_values(base);
        if (rc != RRT_OK) return rc;
        load_params(base, b);
    }
    AutoResources a;
    a.base = b;
    if (hipGetDevice(&a.device) != hipSuccess) return RRT_ERR_NO_DEVICE;
    a.table_budget = table_budget_bytes;
    int rc = RRT_OK;
    if (pool_bytes > 0) rc = rrt_workspace_create(pool_bytes, &a.pool);
    if (rc == RRT_OK) rc = rrt_tile_order_create(&a.order);
    if (rc != RRT_OK) {
        if (a.pool) rrt_workspace_destroy(a.pool);
        return rc;
    }
    a.on = true;
    g_auto = a;
    return RRT_OK;
}

int rrt_launch_auto_resources_info(int* on, int* table_builds, float* table_t0, float* table_t1, size_t* table_bytes) {
    std::lock_guard<std::mutex> lk(g_auto_mu);
    if (on) *on = g_auto.on ? 1 : 0;
    if (table_builds) *table_builds = g_auto.table_builds;
    if (table_t0) *table_t0 = g_auto.t0;
    if (table_t1) *table_t1 = g_auto.t1;
    if (table_bytes) {
        *table_bytes = 0;
        if (g_auto.table) rrt_noise_table_info(g_auto.table, nullptr, table_bytes, nullptr);
    }
    return RRT_OK;
}

/* launch_raymarch() as the reference spells it, minus the C++ types: cam12 = pos, forward, right, up;
 * effects36 = the 36 bytes of struct CameraEffects.  Asynchronous on the null stream.  The reference's
 * launcher reports nothing (src/raymarcher.cu:176-180); this one returns the status and, the first time a
 * launch fails, says why on stderr. */
int rrt_launch_raymarch_compat(void* d_out_rgba8, int width, int height, float time, const float* cam12,
                               rrt_sky_t sky, const void* effects36) {
    if (!cam12 || !effects36) return RRT_ERR_INVALID_ARGUMENT;
    rrt_camera c;
    memcpy(&c, cam12, sizeof(c));
    rrt_effects fx;
    memcpy(&fx, effects36, sizeof(fx));
    rrt_params prm;
    if (!auto_params(time, prm)) rrt_get_launch_defaults(&prm);
    const int rc = rrt_launch_raymarch(d_out_rgba8, width, height, time, &c, sky, &fx, &prm, nullptr);
    if (rc != RRT_OK) {
        static std::atomic<bool> said{false};
        if (!said.exchange(true)) {
            fprintf(stderr, "launch_raymarch: %s%s%s (reported once)\n", rrt_status_string(rc),
                    rc == RRT_ERR_HIP ? " -- " : "", rc == RRT_ERR_HIP ? rrt_last_hip_error() : "");
        }
    }
    return rc;
}

int rrt_launch_raymarch(void* d_out_rgba8, int width, int height, float time, const rrt_camera* cam,
                        rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream) {
    return rrt_launch_raymarch_rows(d_out_rgba8, width, height, 0, height, time, cam, sky, fx, prm, stream);
}

int rrt_launch_raymarch_rows(void* d_out_rows, int width, int height, int y0, int y1, float time,
                             const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                             const rrt_params* prm, void* stream) {
    int rc = check_common(d_out_rows, width, height, cam, fx, prm);
    if (rc) return rc;
    if (y0 < 0 || y1 > height || y0 > y1) return RRT_ERR_INVALID_ARGUMENT;
    const RowMap rows{y1 - y0, y0, y1 - y0 > 0 ? y1 - y0 : 1, 0, 1, nullptr};
    return launch_frame(d_out_rows, width, height, rows, time, cam, sky, fx, prm, nullptr, stream);
}

int rrt_launch_raymarch_tiles(void* d_out_tiles, int width, int height, int tile_rows, int shard, int n_shards,
                              float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                              const rrt_params* prm, void* stream) {
    int rc = check_common(d_out_tiles, width, height, cam, fx, prm);
    if (rc) return rc;
    RowMap rows;
    if ((rc = shard_map(height, tile_rows, shard, n_shards, rows))) return rc;
    return launch_frame(d_out_tiles, width, height, rows, time, cam, sky, fx, prm, nullptr, stream);
}

int rrt_tile_shard_rows(int height, int tile_rows, int shard, int n_shards, int* rows) {
    if (!rows || height <= 0 || tile_rows <= 0 || n_shards <= 0 || shard < 0 || shard >= n_shards)
        return RRT_ERR_INVALID_ARGUMENT;
    *rows = shard_rows(height, tile_rows, shard, n_shards);
    return RRT_OK;
}

int rrt_assemble_tiles(void* d_frame, const void* d_tiles, int width, int height, int tile_rows, int shard,
                       int n_shards, void* stream) {
    if (!d_frame || !d_tiles || width <= 0 || height <= 0) return RRT_ERR_INVALID_ARGUMENT;
    RowMap m;
    const int rc = shard_map(height, tile_rows, shard, n_shards, m);
    if (rc || m.n_local_rows == 0) return rc;
    dim3 grid((width + 255) / 256, m.n_local_rows < kMaxGridY ? m.n_local_rows : kMaxGridY);
    hipLaunchKernelGGL(assemble_tiles_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uchar4*>(d_frame), static_cast<const uchar4*>(d_tiles), width, height, m);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

int rrt_assemble_all_tiles(void* d_frame, const void* d_tiles_all, size_t shard_stride_bytes, int width, int height,
                           int tile_rows, int n_shards, void* stream) {
    if (!d_frame || !d_tiles_all || width <= 0 || height <= 0 || tile_rows <= 0 || n_shards <= 0 ||
        (shard_stride_bytes & 3) != 0)
        return RRT_ERR_INVALID_ARGUMENT;
    if (shard_stride_bytes / 4 < (size_t)shard_rows(height, tile_rows, 0, n_shards) * width) return RRT_ERR_INVALID_ARGUMENT;
    dim3 grid((width + 255) / 256, height < kMaxGridY ? height : kMaxGridY);
    hipLaunchKernelGGL(assemble_all_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<uchar4*>(d_frame), static_cast<const uchar4*>(d_tiles_all), shard_stride_bytes / 4,
                       width, height, tile_rows, n_shards);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

/* ---- explicit tile -> shard assignment (rrt_tile_map) ---- */
int rrt_tile_map_create(int height, int tile_rows, int n_shards, const int32_t* shard_of_tile, int* out_id) {
    if (!shard_of_tile || !out_id || height <= 0 || tile_rows <= 0 || n_shards <= 0) return RRT_ERR_INVALID_ARGUMENT;
    const int n_tiles = (height + tile_rows - 1) / tile_rows;
    auto m = std::make_shared<TileMapObject>();
    m->height = height; m->tile_rows = tile_rows; m->n_shards = n_shards; m->n_tiles = n_tiles;
    m->device = current_device();
    m->shard_of_tile.assign(shard_of_tile, shard_of_tile + n_tiles);
    m->offset.assign(n_shards + 1, 0);
    m->rows.assign(n_shards, 0);
    for (int t = 0; t < n_tiles; ++t) {
        const int sh = shard_of_tile[t];
        if (sh < 0 || sh >= n_shards) return RRT_ERR_INVALID_ARGUMENT;
        ++m->offset[sh + 1];
        m->rows[sh] += (t + 1) * tile_rows <= height ? tile_rows : height - t * tile_rows;
    }
    for (int sh = 0; sh < n_shards; ++sh) m->offset[sh + 1] += m->offset[sh];
    /* device image: [tile_of_local, grouped by shard, increasing t | shard_of_tile | k_of_tile] */
    std::vector<int> img(3 * (size_t)n_tiles), fill(m->offset.begin(), m->offset.end() - 1);
    for (int t = 0; t < n_tiles; ++t) {
        const int sh = shard_of_tile[t], k = fill[sh] - m->offset[sh];
        img[fill[sh]++] = t;
        img[n_tiles + t] = sh;
        img[2 * (size_t)n_tiles + t] = k;
    }
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->d_img), img.size() * sizeof(int));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(tile map)");
    e = hipMemcpy(m->d_img, img.data(), img.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(m->d_img); return hip_fail(e, "hipMemcpy(tile map)"); }
    *out_id = g_tile_maps.insert(m);
    return RRT_OK;
}

int rrt_tile_map_destroy(int id) {
    std::shared_ptr<TileMapObject> m;
    if (g_tile_maps.take(id, m, made_here<TileMapObject>)) return RRT_ERR_BAD_HANDLE;       /* freed under the device that owns it */
    hipError_t e = hipFree(m->d_img);
    if (e != hipSuccess) return hip_fail(e, "hipFree(tile map)");
    return RRT_OK;
}

int rrt_tile_map_shard_rows(int id, int shard, int* rows, int* max_rows) {
    std::shared_ptr<TileMapObject> m;
    if (!g_tile_maps.get(id, m)) return RRT_ERR_BAD_HANDLE;
    if (shard < 0 || shard >= m->n_shards) return RRT_ERR_INVALID_ARGUMENT;
    if (rows) *rows = m->rows[shard];
    if (max_rows) { int mx = 0; for (int r : m->rows) mx = r > mx ? r : mx; *max_rows = mx; }
    return RRT_OK;
}

/* Deal row tiles to shards by cost: longest-processing-time-first greedy -- tiles in decreasing cost (ties: increasing
 * index), each to the shard with the smallest load so far (ties: fewest rows, then lowest index).  Deterministic host
 * arithmetic in double: every rank computes the same map from the same costs, no exchange needed.  max_tiles_per_shard
 * (0: none) bounds the buffer a shard needs: ceil(n_tiles / n_shards) + slack is typical. */
int rrt_tile_map_balance(int n_tiles, const float* tile_cost, int n_shards, int max_tiles_per_shard, int32_t* shard_of_tile_out) {
    if (n_tiles <= 0 || n_shards <= 0 || !tile_cost || !shard_of_tile_out || max_tiles_per_shard < 0) return RRT_ERR_INVALID_ARGUMENT;
    if (max_tiles_per_shard > 0 && (long long)max_tiles_per_shard * n_shards < n_tiles) return RRT_ERR_INVALID_ARGUMENT;
    std::vector<int> idx(n_tiles);
    for (int t = 0; t < n_tiles; ++t) {
        if (!(tile_cost[t] >= 0.0f) || !(tile_cost[t] < 3.0e38f)) return RRT_ERR_INVALID_ARGUMENT;    /* NaN, negative, infinite */
        idx[t] = t;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return tile_cost[x] > tile_cost[y]; });
    std::vector<double> load(n_shards, 0.0);
    std::vector<int> count(n_shards, 0);
    for (int t : idx) {
        int best = -1;
        for (int sh = 0; sh < n_shards; ++sh) {
            if (max_tiles_per_shard > 0 && count[sh] >= max_tiles_per_shard) continue;
            if (best < 0 || load[sh] < load[best] || (load[sh] == load[best] && count[sh] < count[best])) best = sh;
        }
        shard_of_tile_out[t] = best;
        load[best] += (double)tile_cost[t];
        ++count[best];
    }
    return RRT_OK;
}

/* Estimated cost of every row tile of the frame, from the coarse march-only probe (one ray per 16 pixels in x, per
 * min(16, tile_rows) rows in y): what rrt_tile_map_balance wants for a frame nobody has rendered yet.  Synchronous (it
 * returns host numbers); allocates and frees its own scratch.  The unit is the tile-order object's (wave clocks / 16),
 * summed over the probe cells of the tile and scaled to the tile's pixel count. */
int rrt_probe_tile_costs(int width, int height, int tile_rows, float time, const rrt_camera* cam, const rrt_effects* fx,
                         const rrt_params* prm, float* tile_cost_host, int n_tiles, void* stream) {
    if (!tile_cost_host || tile_rows <= 0 || !cam || !fx || width <= 0 || height <= 0) return RRT_ERR_INVALID_ARGUMENT;
    if (n_tiles != (height + tile_rows - 1) / tile_rows) return RRT_ERR_INVALID_ARGUMENT;
    if (prm) { int rc = check_params_abi(prm); if (rc == RRT_OK) rc = check_params_values(prm); if (rc != RRT_OK) return rc; }
    rrt_params p;
    load_params(prm, p);
    FrameArgs a;
    memset(&a, 0, sizeof(a));
    a.width = width; a.height = height; a.time = time; a.cam = *cam;
    a.use_lens = fx->use_lens_distortion != 0; a.distortion_amount = fx->distortion_amount;
    a.spin = p.spin; a.drag_c = (2.0f * p.spin) * 2.0f; a.max_steps = p.max_steps;
    a.rows = frame_rows(height);
    a.grid_row_stride = 1;
    const int sy = tile_rows < kProbeStride ? tile_rows : kProbeStride;
    ProbeArgs q;
    const int cells_x = (width + kProbeStride - 1) / kProbeStride, cells_y = (height + sy - 1) / sy;
    unsigned* d_cells = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d_cells), (size_t)cells_x * cells_y * sizeof(unsigned));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc(probe)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = enqueue_probe(a, q, d_cells, kProbeStride, sy, p.volumetrics != 0, st);
    std::vector<unsigned> cells((size_t)cells_x * cells_y);
    if (rc == RRT_OK) {
        e = hipMemcpyAsync(cells.data(), d_cells, cells.size() * sizeof(unsigned), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = hip_fail(e, "probe read-back");
    }
    (void)hipFree(d_cells);
    if (rc != RRT_OK) return rc;
    for (int t = 0; t < n_tiles; ++t) {
        const int y0 = t * tile_rows, y1 = (t + 1) * tile_rows < height ? (t + 1) * tile_rows : height;
        double sum = 0.0; int n = 0;
        for (int cy = y0 / sy; cy * sy < y1 && cy < cells_y; ++cy) {
            const int yc = cy * sy + sy / 2 < height ? cy * sy + sy / 2 : height - 1;     /* the row the cell was probed at */
            if (yc < y0 || yc >= y1) continue;
            for (int cx = 0; cx < cells_x; ++cx) sum += (double)cells[(size_t)cy * cells_x + cx];
            ++n;
        }
        if (n == 0) {        /* no probe row inside the tile (only when tile_rows does not divide the stride): nearest one */
            const int cy = (y0 + y1) / 2 / sy < cells_y ? (y0 + y1) / 2 / sy : cells_y - 1;
            for (int cx = 0; cx < cells_x; ++cx) sum += (double)cells[(size_t)cy * cells_x + cx];
            n = 1;
        }
        tile_cost_host[t] = (float)(sum / n * (double)(y1 - y0) / (double)kWGPixY);      /* per 8-row wave tile row of the tile */
    }
    return RRT_OK;
}

int rrt_launch_raymarch_tilemap(void* d_out_tiles, int width, int height, int tile_map, int shard, float time,
                                const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream) {
    const int rc = check_common(d_out_tiles, width, height, cam, fx, prm);
    if (rc) return rc;
    std::shared_ptr<TileMapObject> m;
    if (lookup_here(g_tile_maps, tile_map, m)) return RRT_ERR_BAD_HANDLE;
    if (m->height != height || shard < 0 || shard >= m->n_shards) return RRT_ERR_INVALID_ARGUMENT;
    const RowMap rows{m->rows[shard], 0, m->tile_rows, shard, m->n_shards, m->d_img + m->offset[shard]};
    return launch_frame(d_out_tiles, width, height, rows, time, cam, sky, fx, prm, nullptr, stream);
}

int rrt_assemble_all_tilemap(void* d_frame, const void* d_tiles_all, size_t shard_stride_bytes, int width, int height,
                             int tile_map, void* stream) {
    if (!d_frame || !d_tiles_all || width <= 0 || height <= 0 || (shard_stride_bytes & 3) != 0) return RRT_ERR_INVALID_ARGUMENT;
    std::shared_ptr<TileMapObject> m;
    if (lookup_here(g_tile_maps, tile_map, m)) return RRT_ERR_BAD_HANDLE;
    if (m->height != height) return RRT_ERR_INVALID_ARGUMENT;
    for (int r : m->rows) if (shard_stride_bytes / 4 < (size_t)r * width) return RRT_ERR_INVALID_ARGUMENT;
    dim3 grid((width + 255) / 256, height < kMaxGridY ? height : kMaxGridY);
    hipLaunchKernelGGL(assemble_map_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<uchar4*>(d_frame),
                       static_cast<const uchar4*>(d_tiles_all), shard_stride_bytes / 4, width, height, m->tile_rows,
                       m->d_img + m->n_tiles, m->d_img + 2 * (size_t)m->n_tiles);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

int rrt_launch_raymarch_ex(void* d_out_rgba8, int width, int height, float time, const rrt_camera* cam,
                           rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm,
                           const rrt_debug_outputs* dbg, void* stream) {
    const int rc = check_common(d_out_rgba8, width, height, cam, fx, prm);
    if (rc) return rc;
    return launch_frame(d_out_rgba8, width, height, frame_rows(height), time, cam, sky, fx, prm, dbg, stream);
}

int rrt_launch_raymarch_ss(void* d_out_rgba8, float* d_hdr_rgba32f, int width, int height, int samples_per_axis, float time,
                           const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream) {
    const int rc = check_ss(d_out_rgba8, width, height, samples_per_axis, cam, fx, prm);
    if (rc) return rc;
    return launch_ss(d_out_rgba8, reinterpret_cast<float4*>(d_hdr_rgba32f), width, height, samples_per_axis, frame_rows(height),
                     nullptr, time, cam, sky, fx, prm, static_cast<hipStream_t>(stream));
}

int rrt_launch_raymarch_ss_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard, int n_shards,
                                 float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm,
                                 void* stream) {
    int rc = check_ss(d_out_tiles, width, height, samples_per_axis, cam, fx, prm);
    if (rc) return rc;
    RowMap rows;
    if ((rc = shard_map(height, tile_rows, shard, n_shards, rows))) return rc;
    return launch_ss(d_out_tiles, nullptr, width, height, samples_per_axis, rows, nullptr, time, cam, sky, fx, prm,
                     static_cast<hipStream_t>(stream));
}

int rrt_launch_raymarch_mb(void* d_out_rgba8, float* d_hdr_rgba32f, int width, int height, int samples_per_axis, int n_times,
                           const float* times, const rrt_camera* cams, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm,
                           void* stream) {
    const int rc = check_mb(d_out_rgba8, width, height, samples_per_axis, n_times, times, cams, fx, prm);
    if (rc) return rc;
    return launch_mb(d_out_rgba8, reinterpret_cast<float4*>(d_hdr_rgba32f), width, height, samples_per_axis, frame_rows(height),
                     n_times, times, cams, sky, fx, prm, static_cast<hipStream_t>(stream));
}

int rrt_launch_raymarch_mb_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard, int n_shards,
                                 int n_times, const float* times, const rrt_camera* cams, rrt_sky_t sky, const rrt_effects* fx,
                                 const rrt_params* prm, void* stream) {
    int rc = check_mb(d_out_tiles, width, height, samples_per_axis, n_times, times, cams, fx, prm);
    if (rc) return rc;
    RowMap rows;
    if ((rc = shard_map(height, tile_rows, shard, n_shards, rows))) return rc;
    return launch_mb(d_out_tiles, nullptr, width, height, samples_per_axis, rows, n_times, times, cams, sky, fx, prm,
                     static_cast<hipStream_t>(stream));
}

int rrt_launch_raymarch_dof(void* d_out_rgba8, float* d_hdr_rgba32f, int width, int height, int samples_per_axis, int n_samples,
                            const float* times, const rrt_camera* cams, const float* lens_xy, float focus, rrt_sky_t sky,
                            const rrt_effects* fx, const rrt_params* prm, void* stream) {
    const int rc = check_dof(d_out_rgba8, width, height, samples_per_axis, n_samples, times, cams, lens_xy, focus, fx, prm);
    if (rc) return rc;
    return launch_mb<LensLaunch>(d_out_rgba8, reinterpret_cast<float4*>(d_hdr_rgba32f), width, height, samples_per_axis,
                                 frame_rows(height), n_samples, times, cams, sky, fx, prm, static_cast<hipStream_t>(stream), lens_xy,
                                 focus);
}

int rrt_launch_raymarch_dof_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard, int n_shards,
                                  int n_samples, const float* times, const rrt_camera* cams, const float* lens_xy, float focus,
                                  rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* stream) {
    int rc = check_dof(d_out_tiles, width, height, samples_per_axis, n_samples, times, cams, lens_xy, focus, fx, prm);
    if (rc) return rc;
    RowMap rows;
    if ((rc = shard_map(height, tile_rows, shard, n_shards, rows))) return rc;
    return launch_mb<LensLaunch>(d_out_tiles, nullptr, width, height, samples_per_axis, rows, n_samples, times, cams, sky, fx, prm,
                                 static_cast<hipStream_t>(stream), lens_xy, focus);
}

int rrt_lens_ray(int width, int height, int x, int y, const rrt_camera* cam, float lx, float ly, float focus, float origin_out[3],
                 float dir_out[3]) {
    if (!cam || !origin_out || !dir_out || width <= 0 || height <= 0 || x < 0 || x >= width || y < 0 || y >= height ||
        !std::isfinite(lx) || !std::isfinite(ly) || !std::isfinite(focus) || !(focus > 0.0f))
        return RRT_ERR_INVALID_ARGUMENT;
    float uvx, uvy;
    lens_ray(width, height, x, y, *cam, 0, 0.0f, lx, ly, lx / focus, ly / focus, origin_out, dir_out, uvx, uvy);
    return RRT_OK;
}

int rrt_lens_points(float aperture, int n_samples, float rotation_rad, float* xy_out) {
    return lens_points(aperture, n_samples, rotation_rad, xy_out) ? RRT_OK : RRT_ERR_INVALID_ARGUMENT;
}

int rrt_glow_default(rrt_glow* g) {
    if (!g) return RRT_ERR_INVALID_ARGUMENT;
    g->struct_size = (uint32_t)sizeof(rrt_glow);
    g->radius = 0.004f;
    g->lobes = 4;
    g->threshold = 1.0f;
    g->intensity = 0.25f;
    return RRT_OK;
}

int rrt_glow_weights(const rrt_glow* g, int height, int lobe, float* out, int cap, int* radius_out) {
    GlowPlan p;
    const int rc = glow_plan(g, height, p);
    if (rc) return rc;
    if (lobe < 0 || lobe >= p.lobes) return RRT_ERR_INVALID_ARGUMENT;
    const int r = p.radius[lobe];
    if (out && cap < 2 * r + 1) return RRT_ERR_INVALID_ARGUMENT;
    if (out) glow_taps_host(p.sigma[lobe], r, out);
    if (radius_out) *radius_out = r;
    return RRT_OK;
}

int rrt_glow_scratch_bytes(int width, int height, const rrt_glow* g, size_t* bytes) {
    if (!bytes || !glow_frame_ok(width, height)) return RRT_ERR_INVALID_ARGUMENT;
    GlowPlan p;
    const int rc = glow_plan(g, height, p);
    if (rc) return rc;
    *bytes = glow_scratch(p, width, height);
    return RRT_OK;
}

int rrt_launch_glow(void* d_out_rgba8, const float* d_hdr_rgba32f, int width, int height, const rrt_glow* g, void* d_scratch,
                    size_t scratch_bytes, void* stream) {
    if (!d_out_rgba8 || !d_hdr_rgba32f || !d_scratch || !glow_frame_ok(width, height)) return RRT_ERR_INVALID_ARGUMENT;
    if ((reinterpret_cast<uintptr_t>(d_hdr_rgba32f) | reinterpret_cast<uintptr_t>(d_scratch)) & 15) return RRT_ERR_INVALID_ARGUMENT;
    GlowPlan p;
    const int rc = glow_plan(g, height, p);
    if (rc) return rc;
    if (scratch_bytes < glow_scratch(p, width, height)) return RRT_ERR_INVALID_ARGUMENT;
    return launch_glow(static_cast<uchar4*>(d_out_rgba8), reinterpret_cast<const float4*>(d_hdr_rgba32f), width, height, g, p,
                       d_scratch, static_cast<hipStream_t>(stream));
}

int rrt_exposure_default(rrt_exposure* e) {
    if (!e) return RRT_ERR_INVALID_ARGUMENT;
    e->struct_size = (uint32_t)sizeof(rrt_exposure);
    e->mode = RRT_EXPOSURE_MANUAL;
    e->ev = 0.0f;
    e->key = 0.5f;
    e->low_permille = 400;
    e->high_permille = 20;
    e->min_ev = -8.0f;
    e->max_ev = 8.0f;
    e->adapt_up = 1.0f;
    e->adapt_down = 1.0f;
    return RRT_OK;
}

int rrt_exposure_bin_ev(int bin, double* ev_out) {
    if (!ev_out || bin < 0 || bin >= kExposureBins) return RRT_ERR_INVALID_ARGUMENT;
    *ev_out = exposure_bin_centre(bin);
    return RRT_OK;
}

int rrt_exposure_adapt(double dt, double tau, float* alpha_out) {
    if (!alpha_out || !std::isfinite(dt) || !std::isfinite(tau) || dt < 0.0 || tau < 0.0) return RRT_ERR_INVALID_ARGUMENT;
    *alpha_out = tau == 0.0 ? 1.0f : (float)(1.0 - std::exp(-dt / tau));
    return RRT_OK;
}

int rrt_exposure_scratch_bytes(size_t* bytes) {
    if (!bytes) return RRT_ERR_INVALID_ARGUMENT;
    *bytes = kExposureScratchBytes;
    return RRT_OK;
}

int rrt_exposure_meter_host(const float* hdr_rgba32f_host, int width, int height, uint32_t* hist_out) {
    if (!hdr_rgba32f_host || !hist_out || !glow_frame_ok(width, height)) return RRT_ERR_INVALID_ARGUMENT;
    memset(hist_out, 0, kExposureBins * sizeof(uint32_t));
    const size_t n = (size_t)width * (size_t)height;
    for (size_t i = 0; i < n; ++i) {
        const float* p = hdr_rgba32f_host + 4 * i;
        const int b = exposure_bin(exposure_luma(p[0], p[1], p[2]));
        if (b >= 0) ++hist_out[b];
    }
    return RRT_OK;
}

int rrt_launch_exposure_reset(void* d_scratch, size_t scratch_bytes, void* stream) {
    if (!exposure_scratch_ok(d_scratch, scratch_bytes)) return RRT_ERR_INVALID_ARGUMENT;
    ExposureTable t;
    for (int b = 0; b < kExposureBins; ++b) t.ev[b] = exposure_bin_centre(b);
    hipLaunchKernelGGL(exposure_reset, dim3(1), dim3(kExposureBins), 0, static_cast<hipStream_t>(stream),
                       static_cast<uint8_t*>(d_scratch), t);
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

int rrt_launch_exposure(void* d_out_rgba8, float* d_hdr_out, const float* d_hdr_in, int width, int height, const rrt_exposure* e,
                        void* d_scratch, size_t scratch_bytes, void* stream) {
    const int rc = check_exposure(e);
    if (rc) return rc;
    if (!d_hdr_in || (!d_out_rgba8 && !d_hdr_out) || !glow_frame_ok(width, height)) return RRT_ERR_INVALID_ARGUMENT;
    const uintptr_t in = reinterpret_cast<uintptr_t>(d_hdr_in), out = reinterpret_cast<uintptr_t>(d_hdr_out);
    if (((in | out) & 15) || (reinterpret_cast<uintptr_t>(d_out_rgba8) & 3)) return RRT_ERR_INVALID_ARGUMENT;
    const uintptr_t hdr_bytes = (uintptr_t)width * (uintptr_t)height * sizeof(float4);
    if (out && out != in && out < in + hdr_bytes && in < out + hdr_bytes) return RRT_ERR_INVALID_ARGUMENT;    /* in place or apart */
    if (e->mode == RRT_EXPOSURE_AUTO && !exposure_scratch_ok(d_scratch, scratch_bytes)) return RRT_ERR_INVALID_ARGUMENT;
    return launch_exposure(static_cast<uchar4*>(d_out_rgba8), reinterpret_cast<float4*>(d_hdr_out),
                           reinterpret_cast<const float4*>(d_hdr_in), width, height, *e, d_scratch, static_cast<hipStream_t>(stream));
}

int rrt_projection_default(int kind, rrt_projection* p) {
    if (!p || (kind != RRT_PROJ_PINHOLE && kind != RRT_PROJ_EQUIRECT && kind != RRT_PROJ_FISHEYE)) return RRT_ERR_INVALID_ARGUMENT;
    p->struct_size = (uint32_t)sizeof(rrt_projection);
    p->kind = kind;
    p->fov_deg = kind == RRT_PROJ_EQUIRECT ? 360.0f : (kind == RRT_PROJ_FISHEYE ? 180.0f : 0.0f);
    p->vfov_deg = kind == RRT_PROJ_EQUIRECT ? 180.0f : 0.0f;
    return RRT_OK;
}

int rrt_projection_ray(const rrt_projection* p, int width, int height, int x, int y, const rrt_camera* cam, float dir_out[3],
                       int* inside_out) {
    const int rc = check_projection(p);
    if (rc) return rc;
    if (!cam || !dir_out || width <= 0 || height <= 0 || x < 0 || x >= width || y < 0 || y >= height) return RRT_ERR_INVALID_ARGUMENT;
    const bool inside = projection_dir(proj_args(*p), width, height, x, y, *cam, dir_out);
    if (inside_out) *inside_out = inside ? 1 : 0;
    return RRT_OK;
}

int rrt_launch_raymarch_pano(void* d_out_rgba8, float* d_hdr_rgba32f, int width, int height, int samples_per_axis,
                             const rrt_projection* proj, float time, const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx,
                             const rrt_params* prm, void* stream) {
    const int rc = check_pano(d_out_rgba8, width, height, samples_per_axis, proj, cam, fx, prm);
    if (rc) return rc;
    return launch_ss(d_out_rgba8, reinterpret_cast<float4*>(d_hdr_rgba32f), width, height, samples_per_axis, frame_rows(height),
                     proj, time, cam, sky, fx, prm, static_cast<hipStream_t>(stream));
}

int rrt_launch_projection_map(void* d_dir_rgba32f, int width, int height, const rrt_projection* proj, const rrt_camera* cam,
                              void* stream) {
    const int rc = check_projection(proj);
    if (rc) return rc;
    if (!d_dir_rgba32f || !cam || width <= 0 || height <= 0 || (long long)width * height >= (1ll << 31)) return RRT_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(d_dir_rgba32f) & 15) return RRT_ERR_INVALID_ARGUMENT;
    const long long n = (long long)width * height;
    hipLaunchKernelGGL(projection_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<float4*>(d_dir_rgba32f), width, height, *cam, proj_args(*proj));
    RRT_HIP(hipGetLastError());
    return RRT_OK;
}

int rrt_launch_raymarch_pano_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard,
                                   int n_shards, const rrt_projection* proj, float time, const rrt_camera* cam, rrt_sky_t sky,
                                   const rrt_effects* fx, const rrt_params* prm, void* stream) {
    int rc = check_pano(d_out_tiles, width, height, samples_per_axis, proj, cam, fx, prm);
    if (rc) return rc;
    RowMap rows;
    if ((rc = shard_map(height, tile_rows, shard, n_shards, rows))) return rc;
    return launch_ss(d_out_tiles, nullptr, width, height, samples_per_axis, rows, proj, time, cam, sky, fx, prm,
                     static_cast<hipStream_t>(stream));
}

int rrt_adaptive_default(rrt_adaptive* ad) {
    if (!ad) return RRT_ERR_INVALID_ARGUMENT;
    ad->struct_size = (uint32_t)sizeof(rrt_adaptive);
    ad->threshold = 8;
    return RRT_OK;
}

int rrt_adaptive_scratch_bytes(int width, int height, size_t* bytes) {
    if (!bytes || !adaptive_frame_ok(width, height)) return RRT_ERR_INVALID_ARGUMENT;
    *bytes = adaptive_scratch(width, height);
    return RRT_OK;
}

int rrt_adaptive_mask(const uint8_t* rgba8_host, int width, int height, const rrt_adaptive* ad, uint8_t* mask_out,
                      uint32_t* count_out) {
    const int rc = check_adaptive(ad);
    if (rc) return rc;
    if (!rgba8_host || !mask_out || !adaptive_frame_ok(width, height)) return RRT_ERR_INVALID_ARGUMENT;
    uint32_t n = 0;
    for (int row = 0; row < height; ++row)
        for (int x = 0; x < width; ++x) {
            const bool r = adaptive_refined(rgba8_host, width, height, x, row, ad->threshold);
            mask_out[(size_t)row * width + x] = r ? 1 : 0;
            n += r ? 1u : 0u;
        }
    if (count_out) *count_out = n;
    return RRT_OK;
}

int rrt_launch_raymarch_adaptive(void* d_out_rgba8, float* d_hdr_rgba32f, int width, int height, int samples_per_axis,
                                 const rrt_projection* proj, const rrt_adaptive* ad, float time, const rrt_camera* cam,
                                 rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm, void* d_scratch, size_t scratch_bytes,
                                 void* stream) {
    int rc = check_adaptive(ad);
    if (rc) return rc;
    rc = proj ? check_pano(d_out_rgba8, width, height, samples_per_axis, proj, cam, fx, prm)
              : check_ss(d_out_rgba8, width, height, samples_per_axis, cam, fx, prm);
    if (rc) return rc;
    if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 15) || scratch_bytes < adaptive_scratch(width, height))
        return RRT_ERR_INVALID_ARGUMENT;
    return launch_adaptive(d_out_rgba8, reinterpret_cast<float4*>(d_hdr_rgba32f), width, height, samples_per_axis, proj, *ad, time,
                           cam, sky, fx, prm, d_scratch, static_cast<hipStream_t>(stream));
}

int rrt_stereo_default(int layout, rrt_stereo* st) {
    if (!st || !valid_layout(layout)) return RRT_ERR_INVALID_ARGUMENT;
    st->struct_size = (uint32_t)sizeof(rrt_stereo);
    st->layout = layout;
    st->base = 1.0f;
    st->convergence = 0.0f;
    st->pole_merge_from_deg = 90.0f;
    st->pole_merge_to_deg = 90.0f;
    return RRT_OK;
}

int rrt_stereo_ray(const rrt_projection* p, const rrt_stereo* st, int width, int height, int eye, int x, int y,
                   const rrt_camera* cam, float origin_out[3], float dir_out[3], int* inside_out) {
    const int rc = check_stereo(p, st);
    if (rc) return rc;
    if (!cam || !origin_out || !dir_out || width <= 0 || height <= 0 || x < 0 || x >= width || y < 0 || y >= height ||
        (eye != RRT_EYE_LEFT && eye != RRT_EYE_RIGHT))
        return RRT_ERR_INVALID_ARGUMENT;
    float uvx, uvy;
    stereo_ray(proj_args(*p), stereo_args(*st, width, height), eye, x, y, *cam, 0, 0.0f, origin_out, dir_out, uvx, uvy);
    if (inside_out) *inside_out = 1;
    return RRT_OK;
}

int rrt_launch_raymarch_stereo(void* d_out_rgba8, float* d_hdr_rgba32f, int width, int height, int samples_per_axis,
                               const rrt_projection* proj, const rrt_stereo* st, float time, const rrt_camera* cam, rrt_sky_t sky,
                               const rrt_effects* fx, const rrt_params* prm, void* stream) {
    int cw, ch;
    const int rc = check_stereo_launch(d_out_rgba8, width, height, samples_per_axis, proj, st, cam, fx, prm, cw, ch);
    if (rc) return rc;
    return launch_ss(d_out_rgba8, reinterpret_cast<float4*>(d_hdr_rgba32f), width, height, samples_per_axis, frame_rows(ch),
                     proj, time, cam, sky, fx, prm, static_cast<hipStream_t>(stream), st);
}

int rrt_launch_raymarch_stereo_tiles(void* d_out_tiles, int width, int height, int samples_per_axis, int tile_rows, int shard,
                                     int n_shards, const rrt_projection* proj, const rrt_stereo* st, float time,
                                     const rrt_camera* cam, rrt_sky_t sky, const rrt_effects* fx, const rrt_params* prm,
                                     void* stream) {
    int cw, ch;
    int rc = check_stereo_launch(d_out_tiles, width, height, samples_per_axis, proj, st, cam, fx, prm, cw, ch);
    if (rc) return rc;
    RowMap rows;
    if ((rc = shard_map(ch, tile_rows, shard, n_shards, rows))) return rc;
    return launch_ss(d_out_tiles, nullptr, width, height, samples_per_axis, rows, proj, time, cam, sky, fx, prm,
                     static_cast<hipStream_t>(stream), st);
}

/* ---- march cache (include/rrt.h) ---- */
int rrt_march_cache_configure(int device, size_t max_bytes) {
    const int dev = march_cache_device(device);
    if (dev < 0) return RRT_ERR_NO_DEVICE;
    MarchCacheObject* c = march_cache_of(dev, true);
    std::lock_guard<std::mutex> lk(c->mu);
    c->pol.reset();
    c->configured = true; c->budget_known = true; c->max_bytes = max_bytes;
    if (c->bytes > max_bytes) return on_device(dev, [&] { MarchCacheRegistry::free_device_memory(*c); return RRT_OK; });
    return RRT_OK;
}

int rrt_march_cache_stats(int device, rrt_march_cache_info* out) {
    if (!out) return RRT_ERR_INVALID_ARGUMENT;
    memset(out, 0, sizeof(*out));
    const int dev = march_cache_device(device);
    if (dev < 0) return RRT_ERR_NO_DEVICE;
    MarchCacheObject* c = march_cache_of(dev, false);
    if (!c) return RRT_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    out->fills = c->pol.st.fills; out->hits = c->pol.st.hits; out->drops = c->pol.st.drops;
    out->misses = c->pol.st.misses; out->uncacheable = c->pol.st.uncacheable;
    out->bytes = c->bytes;
    out->max_bytes = march_cache_env_off() ? 0 : (c->budget_known ? c->max_bytes : 0);
    out->state = c->pol.state; out->why = c->pol.why;
    if (c->pol.state == rrt_mc::kReady || c->pol.state == rrt_mc::kPending) {
        out->blocks_capacity = c->cap_blocks;
        if (c->pol.state == rrt_mc::kReady) out->blocks_used = c->used_blocks;
    }
    return RRT_OK;
}

int rrt_march_cache_release(int device) {
    const int dev = march_cache_device(device);
    if (dev < 0) return RRT_ERR_NO_DEVICE;
    MarchCacheObject* c = march_cache_of(dev, false);
    if (!c) return RRT_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    c->pol.reset();
    return on_device(dev, [&] { MarchCacheRegistry::destroy(*c); return RRT_OK; });
}

#ifdef RRT_TEST_HOOKS
#define RRT_TEST_HOOKS_PART 2
#include "rrt_test_hooks.h"
#undef RRT_TEST_HOOKS_PART
#endif

}  // extern "C"

/* The reference's entry point as a linkable C++ symbol (include/raymarcher.h:19, src/raymarcher.cu:176-180),
 * for translation units built against THIS repository's include/raymarcher.h (HIP vector types).  The twin
 * under the reference's own mangled name (CUDA's `struct uchar4`) is csrc/rrt_compat.cpp. */
#include "../../include/raymarcher.h"
void launch_raymarch(uchar4* d_out, int w, int h, float time, CameraState cam, cudaTextureObject_t skyboxTex,
                     CameraEffects effects) {
    (void)rrt_launch_raymarch_compat(d_out, w, h, time, reinterpret_cast<const float*>(&cam), skyboxTex, &effects);
}
