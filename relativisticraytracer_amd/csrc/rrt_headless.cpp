// rrt_headless.cpp -- the reference's main loop (src/main.cpp:482-539) without a window, in C++, on top of
// the C ABI (include/rrt.h).  Per frame k = 1..N exactly what main() does while recording: advance the
// fixed 1/24 s float clock (main.cpp:511-516), take the camera from the active path (getInterpolatedState,
// :176-203) or the start-up camera (:128-130), launch_raymarch (:467), hand the pixels to the recorder
// (captureFrame, :85-97 -- here a raw RGBA stream, the bytes the reference pipes into ffmpeg).
//
//   rrt_headless --width 1000 --height 700 --frames 24 --path 0 --spin 0.9 --out frames.rgba [--sky-seed 1 | --sky file.rrtsky]
//                [--gpus N] [--tile-rows 16] [--workspace-gib G] [--noise-table-gib B | --no-noise-table]
//                [--arith strict|fmad|fast] [--path-window F | --path-window -1 | --path-policy auto|single|three-pass]
//                [--init-timeout 300] [--frame-timeout 120]      (watchdog, seconds; exit status 3 when it fires)
//                [--supersample 1|2|4|8]       (S x S sub-samples per pixel: rrt_launch_raymarch_ss*, single kernel, no pool)
//                [--motion-blur 1|2|4|8|16 [--shutter F]]   (K sub-frames over the last F of the frame interval, default 0.5:
//                                              rrt_motion_clock, rrt_launch_raymarch_mb*, single kernel, no pool)
//                [--glow INTENSITY [--glow-radius R] [--glow-threshold T] [--glow-lobes L]]   (HDR glow: the frame renders through
//                                              rrt_launch_raymarch_ss / _mb into an HDR buffer, rrt_launch_glow writes its RGBA8;
//                                              one GPU only, single kernel, no pool)
//                [--projection pinhole|equirect|fisheye [--fov DEG] [--vfov DEG]]   (panoramas: rrt_launch_raymarch_pano*, single
//                                              kernel, no pool; equirect --fov 360 --vfov 180, fisheye --fov 180 (aperture); not with
//                                              --motion-blur > 1, equirect not with --glow)
//                [--stereo top-bottom|side-by-side [--stereo-base B] [--convergence Z] [--pole-merge FROM TO]]   (a stereo pair
//                                              per frame: rrt_launch_raymarch_stereo*, single kernel, no pool; --width / --height per
//                                              eye, the composite is written; pinhole (off-axis) or equirect (ODS); not with fisheye,
//                                              --motion-blur > 1 or --glow; --convergence pinhole only, --pole-merge equirect only)
//                [--supersample 2|4|8 --adaptive [T]]   (adaptive supersampling: rrt_launch_raymarch_adaptive -- the 1x frame, only the
//                                              pixels that differ from a 4-neighbour by more than T (0 ... 255, default 8) rendered
//                                              S x S; one GPU only; not with --motion-blur > 1 or --stereo; combines with
//                                              --projection and --glow)
//                [--dof APERTURE [--focus Z|hole] [--dof-samples 1|2|4|8|16]]   (depth of field: rrt_launch_raymarch_dof* through K
//                                              points of a thin lens of radius APERTURE (rrt_lens_points; K default 8), sample m
//                                              through lens point bitrev_K(m), focused Z along forward (default hole: the frame's
//                                              camera's distance to the origin); single kernel, no pool; with --motion-blur M > 1
//                                              the samples are the shutter's sub-frames (K = M); pinhole only, not with --stereo
//                                              or --adaptive)
//                [--exposure EV | --auto-exposure [KEY]] [--exposure-speed UP DOWN] [--exposure-range MIN MAX]
//                [--exposure-percentiles LOW HIGH]   (exposure control: the frame renders into an HDR buffer as with --glow,
//                                              rrt_launch_exposure writes its RGBA8 -- with --glow it scales the HDR in place and the
//                                              glow follows.  --exposure alone: EV stops, manual; --auto-exposure: metered per frame
//                                              and adapted on the device (KEY default 0.5), --exposure then the compensation;
//                                              UP / DOWN: time constants in seconds towards a higher / lower EV, turned into
//                                              per-frame factors with 1 / fps (default 0 0: no smoothing); LOW HIGH in per mille;
//                                              one GPU only, single kernel, no pool; with every frame kind)
//                [--y4m x.y4m [--y4m-chroma 420|444] [--y4m-range limited|full] [--y4m-depth 8|10]]   (also -- or, without --out,
//                                              only -- a YUV4MPEG2 file: BT.709 Y'CbCr packed on device 0 (include/rrt_yuv.h), top-down.
//                                              Depth 8 converts the assembled RGBA8 frame, in every mode; depth 10 converts the frame's
//                                              linear HDR, the whole-frame HDR path of --exposure: one GPU only, not with --glow)
//                [--y4m-transfer sdr|pq [--hdr-white NITS] [--hdr-peak NITS] [--hdr-knee F]]   (pq, with --y4m-depth 10: HDR10 -- the
//                                              linear HDR as absolute light behind SMPTE ST 2084, BT.2020 -- and x.y4m.hdr10.json with
//                                              MaxCLL / MaxFALL, metered on the device, and the encoder options)
//                [--exr f.%04d.exr [--exr-type half|float] [--exr-compression none|zips|zip] [--exr-level 1..9]]   (also, or only,
//                                              one scene-linear OpenEXR file per frame (include/rrt_exr.h): the frame's linear HDR --
//                                              after the exposure, before any tone map -- as B, G, R scanlines packed on device 0 and
//                                              deflated with zlib on a small thread pool.  The pattern holds one frame field; a plain
//                                              name serves --frames 1.  The whole-frame HDR path: one GPU only, not with --glow)
//                [--exr-layers steps,horizon,transmittance,emission,direction,position|all]   (with --exr: per-ray data layers next
//                                              to B, G, R in every file.  The frame is rendered by the debug launch, whose planes the
//                                              layers read as the march left them; the exposure scales B, G, R only.  The 1x pinhole
//                                              frame only)
//                [--png f.%04d.png [--png-depth 8|16] [--png-filter adaptive|none|sub|up|average|paeth] [--png-level 1..9] [--png-deflate host|device]]   (also,
//                                              or only, one PNG file per frame (include/rrt_png.h): RGB scanlines filtered, scored and
//                                              summed on device 0, deflated in slices with zlib on the same thread pool.  Depth 8
//                                              converts the assembled RGBA8 frame, in every mode; depth 16 tone-maps the frame's
//                                              linear HDR to 16 bits -- the whole-frame HDR path: one GPU only, not with --glow)
//
// Noise tables: the reference's simTime runs without bound (main.cpp:515) and a table's size grows with the times
// it covers, so each device keeps ONE table over a window of the clock that fits --noise-table-gib (default 2;
// rrt_noise_table_fit_window picks window and coverage) and rebuilds it -- milliseconds -- when the clock leaves the
// window.  Frames that had to render without a table are counted in the summary line, never silent.
//
// Multi-GPU (the reference is single-GPU): ONE process drives N devices.  ncclCommInitAll
// gives one RCCL communicator per device; image tile t (rows [16t, 16t+16)) belongs to device t mod N; every
// frame each device renders its tiles into a compact buffer (rrt_launch_raymarch_tiles), ONE grouped
// ncclSend / ncclRecv exchange -- a gather over xGMI -- lands all shards in one allocation on device 0, and
// device 0 scatters them into the bottom-up frame with one launch (rrt_assemble_all_tiles).  Two frames are in
// flight: frame k lives on stream k mod 2 of every device (own tile / gather / frame buffers and own pool), so
// the next frame's wavefronts fill the drain of this one's kernels and the exchange sits under marching.
// The same scheme as relativisticraytracer_amd/sharding.py (one process per GPU over torch.distributed), which
// bench.py uses; the bytes are identical (tests/test_headless.py).
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <sched.h>
#include <unistd.h>
#include <zlib.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <filesystem>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rrt.h"
#include "../../include/rrt_yuv.h"
#include "../../include/rrt_exr.h"
#include "../../include/rrt_png.h"
#include "../../include/rrt_deflate.h"

namespace {

// the bench/test sky (relativisticraytracer_amd/sky.py: synthetic_sky), integer arithmetic only
uint32_t mix(uint64_t a) {
    a &= 0xFFFFFFFFull;
    a = ((a ^ (a >> 16)) * 0x7FEB352Dull) & 0xFFFFFFFFull;
    a = ((a ^ (a >> 15)) * 0x846CA68Bull) & 0xFFFFFFFFull;
    a = a ^ (a >> 16);
    return (uint32_t)a;
}
std::vector<uint8_t> synthetic_sky(int w, int h, int seed) {
    std::vector<uint8_t> out((size_t)w * h * 4);
    for (int64_t j = 0; j < h; ++j)
        for (int64_t i = 0; i < w; ++i) {
            auto tri = [](int64_t v) { int64_t m = v % 512; if (m < 0) m += 512; m -= 256; return m < 0 ? -m : m; };
            int64_t ti = tri(i * 4 * 256 / w), tj = tri(j * 2 * 256 / h);
            int64_t band = 96 - (j - h / 2 < 0 ? h / 2 - j : j - h / 2) * 96 * 6 / h;
            if (band < 0) band = 0;
            if (band > 96) band = 96;
            int64_t r = 10 + ti * 30 / 256 + band * 2 / 3, g = 12 + tj * 26 / 256 + band / 2, b = 28 + (ti + tj) * 20 / 256 + band;
            uint32_t hsh = mix((uint64_t)(i + j * w + (int64_t)seed * 0x9E3779B1ll));
            if (hsh % 641u == 0) {
                int64_t mag = 96 + (hsh >> 11) % 160u, tint = (hsh >> 20) % 48u;
                r = mag + tint > 255 ? 255 : mag + tint; g = mag; b = mag + 48 - tint > 255 ? 255 : mag + 48 - tint;
            }
            auto cl = [](int64_t v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); };
            uint8_t* t = &out[4 * ((size_t)j * w + i)];
            t[0] = cl(r); t[1] = cl(g); t[2] = cl(b); t[3] = 255;
        }
    return out;
}

// A raw sky (relativisticraytracer_amd/sky.py: save_sky_raw, tools/sky_to_raw.py): "RRTSKY1\n", "<width> <height>\n", then height x width
// RGBA8 texels, row 0 = top -- the bytes the reference's stbi_load(..., 4) returns (src/main.cpp:240), decoded ONCE with the reference's
// own decoder and shipped (JPEG decoders differ: SURVEY.md row f1).  Returns false with a message on anything else.
bool load_sky_raw(const std::string& path, std::vector<uint8_t>& texels, int& w, int& h) {
    FILE* fh = fopen(path.c_str(), "rb");
    if (!fh) { fprintf(stderr, "rrt_headless: cannot open sky %s\n", path.c_str()); return false; }
    char magic[8] = {};
    bool ok = fread(magic, 1, 8, fh) == 8 && memcmp(magic, "RRTSKY1\n", 8) == 0;
    char line[64] = {};
    long long lw = 0, lh = 0;
    ok = ok && fgets(line, sizeof(line), fh) != nullptr && sscanf(line, "%lld %lld", &lw, &lh) == 2 && lw > 0 && lh > 0 && lw * lh <= (1ll << 30);
    if (ok) {
        texels.resize((size_t)(lw * lh * 4));
        ok = fread(texels.data(), 1, texels.size(), fh) == texels.size() && fgetc(fh) == EOF;
    }
    fclose(fh);
    if (!ok) { fprintf(stderr, "rrt_headless: %s is not a raw sky (RRTSKY1 header, width height, RGBA8 texels)\n", path.c_str()); return false; }
    w = (int)lw; h = (int)lh;
    return true;
}

// Progress trace + watchdog.  Every phase of the driver passes a trace point; the last kTraceKeep of them are kept in
// memory (RRT_HEADLESS_TRACE=1 also prints them as they happen).  A watchdog thread looks at the time since the last
// trace point: it says on stderr every 30 s where the driver is waiting, and once the wait exceeds the limit of the
// phase (--init-timeout for the bring-up -- communicator included --, --frame-timeout once frames are being rendered) it
// prints the kept trace and every communicator's ncclCommGetAsyncError and _exit()s with status 3: a sick node or a stuck
// collective ends the run with a diagnosis instead of hanging it (no retry, nothing is re-executed).
// Why the bring-up gets its own, longer limit: /opt/rocm/lib/librccl.so is a 573 MB fat binary; the first collective of a
// process page-faults the gfx950 code object out of it, which took minutes on a box with a cold page cache (the one
// abnormal end of round 3) -- warm_library_pages() below turns that into one sequential read.
constexpr int kTraceKeep = 96;
struct TraceState {
    std::mutex mu;
    std::string lines[kTraceKeep];
    unsigned long long n = 0;
    std::atomic<long long> last_ns{0};
    std::atomic<const char*> phase{"start-up"};
    std::atomic<bool> in_frames{false}, stop{false};
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    std::vector<ncclComm_t> comms;              // filled once, before in_frames (read by the watchdog on expiry only)
};
TraceState g_tr;

long long now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - g_tr.t0).count();
}
void trace(const char* what, int k = -1) {
    static const bool on = getenv("RRT_HEADLESS_TRACE") != nullptr;
    const long long t = now_ns();
    char buf[160];
    if (k >= 0) snprintf(buf, sizeof(buf), "[rrt_headless %8.3f s] %s %d", t * 1e-9, what, k);
    else snprintf(buf, sizeof(buf), "[rrt_headless %8.3f s] %s", t * 1e-9, what);
    {
        std::lock_guard<std::mutex> lk(g_tr.mu);
        g_tr.lines[g_tr.n++ % kTraceKeep] = buf;
    }
    g_tr.phase.store(what);
    g_tr.last_ns.store(t);
    if (on) { fprintf(stderr, "%s\n", buf); fflush(stderr); }
}
void dump_trace() {
    std::lock_guard<std::mutex> lk(g_tr.mu);
    const unsigned long long first = g_tr.n > kTraceKeep ? g_tr.n - kTraceKeep : 0;
    for (unsigned long long i = first; i < g_tr.n; ++i) fprintf(stderr, "  %s\n", g_tr.lines[i % kTraceKeep].c_str());
}
void watchdog(double init_limit_s, double frame_limit_s) {
    long long said = 0;
    while (!g_tr.stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(200));
        const long long idle = now_ns() - g_tr.last_ns.load();
        const double limit = g_tr.in_frames.load() ? frame_limit_s : init_limit_s;
        if (idle > (said + 1) * 30000000000ll) {
            ++said;
            fprintf(stderr, "rrt_headless: %.0f s in \"%s\" (limit %.0f s)\n", idle * 1e-9, g_tr.phase.load(), limit);
            fflush(stderr);
        }
        if (idle < 30000000000ll) said = 0;
        if (limit > 0.0 && idle * 1e-9 > limit) {
            fprintf(stderr, "rrt_headless: no progress for %.0f s in \"%s\" -- giving up.  Last trace points:\n", idle * 1e-9,
                    g_tr.phase.load());
            dump_trace();
            std::vector<ncclComm_t> comms;
            { std::lock_guard<std::mutex> lk(g_tr.mu); comms = g_tr.comms; }
            for (size_t d = 0; d < comms.size(); ++d) {
                ncclResult_t async = ncclSuccess;
                const ncclResult_t q = ncclCommGetAsyncError(comms[d], &async);
                fprintf(stderr, "  communicator %zu: ncclCommGetAsyncError -> %s, async error: %s\n", d, ncclGetErrorString(q),
                        ncclGetErrorString(async));
            }
            fflush(stderr);
            _exit(3);
        }
    }
}

// Read a shared library's file once, front to back, so that its pages are in the page cache before the loader / the HIP
// runtime fault them in one by one (on a cold overlay file system the page-by-page path is the slow one).
void warm_library_pages(const void* symbol_in_library) {
    Dl_info info;
    if (!dladdr(symbol_in_library, &info) || !info.dli_fname) return;
    const int fd = open(info.dli_fname, O_RDONLY);
    if (fd < 0) return;
    (void)posix_fadvise(fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    std::vector<char> buf(8u << 20);
    while (read(fd, buf.data(), buf.size()) > 0) {}
    close(fd);
}

int fail(const char* what, int rc) {
    fprintf(stderr, "rrt_headless: %s: %s (%s)\n", what, rrt_status_string(rc), rrt_last_hip_error());
    return 1;
}
#define HIPCHK(call)                                                                                          \
    do {                                                                                                      \
        hipError_t e_ = (call);                                                                               \
        if (e_ != hipSuccess) { fprintf(stderr, "rrt_headless: %s: %s\n", #call, hipGetErrorString(e_)); return 1; } \
    } while (0)
#define NCCLCHK(call)                                                                                          \
    do {                                                                                                       \
        ncclResult_t r_ = (call);                                                                              \
        if (r_ != ncclSuccess) { fprintf(stderr, "rrt_headless: %s: %s\n", #call, ncclGetErrorString(r_)); return 1; } \
    } while (0)

constexpr int kMaxSlots = 4;   // capacity of the per-slot arrays; --frames-in-flight picks 1..kMaxSlots of them

struct Device {                // everything one GPU owns
    int id = 0;
    rrt_sky_t sky = 0;
    int noise_table = 0;                          // this device's copy of the current window's table (0: none)
    int pool[kMaxSlots] = {};
    int order[kMaxSlots] = {};                    // rrt_tile_order per slot (0: static dispatch order)
    hipStream_t stream[kMaxSlots] = {};
    void* tiles[kMaxSlots] = {};                  // this device's shard of a frame
    int shard_rows = 0;
    ncclComm_t comm = nullptr;
    void* probe = nullptr;                        // 256 B to send + 256 B per peer to receive: the bring-up exchange
    hipEvent_t comm_free = nullptr;               // after this device's part of the last exchange (orders the next one behind it)
    // per-window path choice (include/rrt.h: rrt_path_chooser_*): the end of every frame's render on this device, kept for
    // 2 * kMaxSlots frames so that frame k - 1's event is still frame k - 1's when frame k is delivered
    int chooser = 0;
    hipEvent_t render_end[2 * kMaxSlots] = {};
};

// ---- the command line

struct Options {               // what the command line sets (parse_options), then what check_options derives from it
    int w = 1000, h = 700, frames = 24, fps = 24, path = -1, sky_seed = 1, all_fx = 0;   // config.h:7-9
    int arith = RRT_ARITH_STRICT;  // --arith strict | fmad | fast (--fast = --arith fast)
    int path_policy = -1;          // --path-policy auto|single|three-pass pins rrt_params.path_policy for every launch (no per-window choice)
    int path_window = 0;           // frames per window of the per-rank path choice (0: the library's default, 48); -1: no choice, the
                                   // three-pass path for every small share as in rounds 1-5
    int gpus = 1, tile_rows = 16, workspace_gib = 2, use_table = 1, force_collective = 0;
    int tile_order = -1;           // cost-ordered dispatch: -1 auto (on when frames are rendered one at a time), 0 off, 1 on
    int supersample = 1;           // --supersample S: S x S sub-samples per pixel (rrt_launch_raymarch_ss*); 1 = one ray per pixel
    int motion = 1;                // --motion-blur K: K shutter sub-frames per frame (rrt_launch_raymarch_mb*); 1 = one instant
    float shutter = 0.5f;          // --shutter F: the fraction of the frame interval the shutter is open (180 degrees)
    rrt_glow glow;                 // --glow INTENSITY (+ --glow-radius / -threshold / -lobes): rrt_launch_glow on every frame
    bool use_glow = false;
    rrt_exposure exposure;         // --exposure EV / --auto-exposure [KEY] (+ --exposure-speed / -range / -percentiles): rrt_launch_exposure
    bool use_exposure = false, exposure_opts = false;
    double exposure_tau[2] = {0.0, 0.0};     // --exposure-speed UP DOWN, seconds
    int projection = RRT_PROJ_PINHOLE;   // --projection: the camera (rrt_launch_raymarch_pano* for equirect / fisheye)
    float fov = 0.0f, vfov = 0.0f;       // --fov / --vfov DEG (0: not given -- the kind's default, rrt_projection_default)
    int stereo_layout = 0;               // --stereo: RRT_STEREO_* (0: mono); rrt_launch_raymarch_stereo*
    bool stereo_base = false, stereo_conv = false, stereo_merge = false;   // which of the stereo options were given
    rrt_stereo stereo;                   // --stereo-base / --convergence / --pole-merge over rrt_stereo_default
    bool use_adaptive = false;           // --adaptive [T]: rrt_launch_raymarch_adaptive
    rrt_adaptive adaptive;
    bool use_dof = false;                // --dof APERTURE: rrt_launch_raymarch_dof*
    float dof_aperture = 0.0f, dof_focus = 0.0f;     // --focus Z (0: hole -- the frame's camera's distance to the origin)
    int dof_samples = 0;                 // --dof-samples K (0: not given -- 8, or --motion-blur's M)
    bool dof_focus_given = false;
    int slots = 3;                 // frames in flight: frame k renders on stream k mod slots while its predecessors are
                                   // gathered / assembled / copied out (a rank's share of a frame is only a few rounds of
                                   // wavefronts; 3 measured best at 8 shards of a 4K frame: profiles/r02_frames_in_flight.txt)
    float spin = 0.0f;
    double table_gib = 2.0;
    double init_timeout = 300.0, frame_timeout = 120.0;       // watchdog limits in seconds (0: none)
    std::string out_path, sky_path;
    std::string y4m_path;                // --y4m PATH: the sequence as a YUV4MPEG2 file (include/rrt_yuv.h)
    bool y4m_opts = false;               // one of --y4m-chroma / --y4m-range / --y4m-depth was given
    rrt_yuv_format yuv;
    int y4m_transfer = -1;               // --y4m-transfer: -1 not given, 0 sdr, 1 pq
    bool hdr_opts = false;               // one of --hdr-white / --hdr-peak / --hdr-knee was given
    bool hdr_nits_ok = true, hdr_knee_ok = true;
    rrt_yuv_hdr10 hdr10;
    std::string exr_path;                // --exr PATTERN: one OpenEXR file per frame (include/rrt_exr.h)
    bool exr_opts = false;               // one of --exr-type / --exr-compression / --exr-level was given
    int exr_type = 0, exr_compression = 2, exr_level = 4;      // the lists' indices (-1: not on the list); the deflate level (0: not 1 ... 9)
    rrt_exr_format exr;
    std::string png_path;                // --png PATTERN: one PNG file per frame (include/rrt_png.h)
    bool png_opts = false;               // one of --png-depth / --png-filter / --png-level was given
    int png_depth = 0, png_filter = 0, png_level = 4;          // the lists' indices (-1: not on the list); the deflate level (0: not 1 ... 9)
    rrt_png_format png;
    bool use_png = false, png16 = false; // depth 16 reads the frame's linear HDR: the whole-frame HDR path
    size_t png_bytes = 0, png_stride = 0, png_sum_bytes = 0;
    int32_t png_slice_rows = 0, png_slices = 0;
    int png_deflate = 0;                 // --png-deflate: 0 host (zlib on the thread pool) | 1 device (include/rrt_deflate.h) | -1: not on the list
    bool png_deflate_opt = false, png_level_opt = false;
    size_t dfl_bound = 0, dfl_scratch = 0;          // --png-deflate device: the most bytes a frame's streams take; the launch's scratch
    std::string exr_layers_arg;          // --exr-layers LIST
    bool exr_layers_given = false;

    // derived: w x h is the frame that is sharded and written (with --stereo the composite of two ew x eh eyes)
    bool pano = false, use_stereo = false, collective = false, auto_exposure = false;
    int ew = 0, eh = 0;
    rrt_projection proj;
    int dof_k = 0;                 // lens samples per sub-sample; sample m looks through dof_xy[2m], dof_xy[2m + 1]
    float dof_xy[32];
    size_t glow_bytes = 0;
    bool y4m = false, y4m10 = false;     // y4m10: the Y4M frames come from the HDR -- the whole-frame HDR path
    bool y4m_pq = false;                 // ... as HDR10 (rrt_launch_yuv_hdr10_from_hdr), with the sidecar
    bool hdr_frame = false;              // --glow, --exposure or y4m10: the frame renders into the slot's HDR buffer
    size_t yuv_bytes = 0;
    bool use_exr = false;                // the EXR frames are the HDR itself: the whole-frame HDR path
    size_t exr_bytes = 0;
    int32_t exr_chunks = 0;
    bool use_layers = false;             // --exr-layers: the frame comes from the debug launch, the files from rrt_launch_exr_layers
    int layer_planes = 0;                // the debug planes the layers read: bit p of kLayerPlanes
    int layer_source[8] = {};            // ... and plane p's index in layers.sources
    rrt_exr_layers layers;               // the channel list and the sources' shapes; the sources' addresses are the slot's (slot_layers)

    Options() {
        rrt_exr_layers_default(&layers);
        rrt_exr_format_default(&exr);
        rrt_png_format_default(&png);
        rrt_yuv_format_default(&yuv);
        rrt_yuv_hdr10_default(&hdr10);
        rrt_glow_default(&glow);
        rrt_exposure_default(&exposure);
        rrt_stereo_default(RRT_STEREO_TOP_BOTTOM, &stereo);
        rrt_adaptive_default(&adaptive);
    }
};

// a refusal: the message on stderr (each keeps the prefix it has always had), exit status 2
__attribute__((format(printf, 1, 2))) int refuse(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    return 2;
}
const char kFovRange[] = "--fov DEG in (0, 360], --vfov DEG in (0, 180]";        // said by the parser (0) and by the host query
const char kDofAperture[] = "usage: --dof APERTURE: the lens radius in scene units, >= 0";   // by the parser and by rrt_lens_points

// all of `text` as a number: false when it is empty or has characters left over; `finite` also refuses inf and nan
bool parse_float(const char* text, float& v, bool finite) {
    char* end = nullptr;
    v = strtof(text, &end);
    return end != text && *end == 0 && (!finite || std::isfinite(v));
}
bool parse_double(const char* text, double& v) {
    char* end = nullptr;
    v = strtod(text, &end);
    return end != text && *end == 0 && std::isfinite(v);
}
bool parse_whole(const char* text, long& v) {
    char* end = nullptr;
    v = strtol(text, &end, 10);
    return end != text && *end == 0;
}
// the index of `text` among `names`; -1: none of them
int one_of(const char* text, std::initializer_list<const char*> names) {
    int j = 0;
    for (const char* n : names) { if (strcmp(text, n) == 0) return j; ++j; }
    return -1;
}

int parse_options(int argc, char** argv, Options& o) {
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const bool more = i + 1 < argc;
        auto next = [&]() -> const char* { return i + 1 < argc ? argv[++i] : ""; };     // the option's value ("": the line ends here)
        auto val = [&](int& dst) { if (more) dst = atoi(argv[++i]); };
        int j;
        const char* m;
        if (a == "--width") val(o.w); else if (a == "--height") val(o.h); else if (a == "--frames") val(o.frames);
        else if (a == "--fps") val(o.fps); else if (a == "--path") val(o.path); else if (a == "--sky-seed") val(o.sky_seed);
        else if (a == "--gpus") val(o.gpus); else if (a == "--tile-rows") val(o.tile_rows); else if (a == "--workspace-gib") val(o.workspace_gib);
        else if (a == "--frames-in-flight") val(o.slots);
        else if (a == "--spin" && more) o.spin = (float)atof(next());
        else if (a == "--noise-table-gib" && more) o.table_gib = atof(next());
        else if (a == "--init-timeout" && more) o.init_timeout = atof(next());
        else if (a == "--frame-timeout" && more) o.frame_timeout = atof(next());
        else if (a == "--no-noise-table") o.use_table = 0;
        else if (a == "--tile-order") o.tile_order = 1; else if (a == "--no-tile-order") o.tile_order = 0;
        else if (a == "--force-collective") o.force_collective = 1;     // run the RCCL exchange even with one GPU (self-check)
        else if (a == "--out" && more) o.out_path = next();
        else if (a == "--sky" && more) o.sky_path = next();
        else if (a == "--y4m" && more) o.y4m_path = next();
        else if (a == "--y4m-chroma") {
            if ((j = one_of(next(), {"420", "444"})) < 0) return refuse("usage: --y4m-chroma 420 | 444");
            o.yuv.chroma = j == 0 ? 420 : 444; o.y4m_opts = true;
        }
        else if (a == "--y4m-range") {
            if ((j = one_of(next(), {"limited", "full"})) < 0) return refuse("usage: --y4m-range limited | full");
            o.yuv.range = j; o.y4m_opts = true;
        }
        else if (a == "--y4m-depth") {
            if ((j = one_of(next(), {"8", "10"})) < 0) return refuse("usage: --y4m-depth 8 | 10");
            o.yuv.bits = j == 0 ? 8 : 10; o.y4m_opts = true;
        }
        else if (a == "--y4m-transfer") {
            if ((o.y4m_transfer = one_of(next(), {"sdr", "pq"})) < 0) return refuse("usage: --y4m-transfer sdr | pq");
        }
        else if (a == "--hdr-white" || a == "--hdr-peak") {
            float& dst = a == "--hdr-white" ? o.hdr10.white_nits : o.hdr10.peak_nits;
            if (!parse_float(next(), dst, true) || !(dst > 0.0f && dst <= 10000.0f)) o.hdr_nits_ok = false;
            o.hdr_opts = true;
        }
        else if (a == "--hdr-knee") {
            if (!parse_float(next(), o.hdr10.knee, true) || !(o.hdr10.knee >= 0.0f && o.hdr10.knee <= 1.0f)) o.hdr_knee_ok = false;
            o.hdr_opts = true;
        }
        // --exr's values are checked in check_options, behind "need --exr PATTERN", as headless.py checks them
        else if (a == "--exr" && more) o.exr_path = next();
        else if (a == "--exr-type") { o.exr_type = one_of(next(), {"half", "float"}); o.exr_opts = true; }
        else if (a == "--exr-compression") { o.exr_compression = one_of(next(), {"none", "zips", "zip"}); o.exr_opts = true; }
        // --png's values are checked in check_options as well, behind "need --png PATTERN"
        else if (a == "--png" && more) o.png_path = next();
        else if (a == "--png-depth") { o.png_depth = one_of(next(), {"8", "16"}); o.png_opts = true; }
        else if (a == "--png-filter") { o.png_filter = one_of(next(), {"adaptive", "none", "sub", "up", "average", "paeth"}); o.png_opts = true; }
        else if (a == "--png-level") { o.png_level = one_of(next(), {"1", "2", "3", "4", "5", "6", "7", "8", "9"}) + 1; o.png_opts = true; o.png_level_opt = true; }
        else if (a == "--png-deflate") { o.png_deflate = one_of(next(), {"host", "device"}); o.png_deflate_opt = true; }
        else if (a == "--exr-layers" && more) { o.exr_layers_arg = next(); o.exr_layers_given = true; }
        else if (a == "--exr-level") { o.exr_level = one_of(next(), {"1", "2", "3", "4", "5", "6", "7", "8", "9"}) + 1; o.exr_opts = true; }
        else if (a == "--all-effects") o.all_fx = 1; else if (a == "--fast") o.arith = RRT_ARITH_FAST;
        else if (a == "--path-window") val(o.path_window);
        else if (a == "--path-policy" && more) {
            const int policy[] = {RRT_PATH_AUTO, RRT_PATH_SINGLE, RRT_PATH_THREE_PASS};
            if ((j = one_of(next(), {"auto", "single", "three-pass"})) < 0) return refuse("--path-policy auto | single | three-pass");
            o.path_policy = policy[j]; o.path_window = -1;
        }
        else if (a == "--supersample") {
            if (one_of(m = next(), {"1", "2", "4", "8"}) < 0) return refuse("--supersample 1 | 2 | 4 | 8 (sub-samples per pixel along each axis)");
            o.supersample = atoi(m);
        }
        else if (a == "--motion-blur") {
            if (one_of(m = next(), {"1", "2", "4", "8", "16"}) < 0) return refuse("--motion-blur 1 | 2 | 4 | 8 | 16 (sub-frames per frame)");
            o.motion = atoi(m);
        }
        else if (a == "--shutter") {
            if (!parse_float(next(), o.shutter, false) || !(o.shutter >= 0.0f && o.shutter <= 1.0f))
                return refuse("--shutter F: a fraction of the frame interval in [0, 1]");
        }
        else if (a == "--glow" || a == "--glow-radius" || a == "--glow-threshold" || a == "--glow-lobes") {
            float v;
            if (!parse_float(next(), v, true)) return refuse("%s: a number", a.c_str());
            if (a == "--glow") { o.glow.intensity = v; o.use_glow = true; }
            else if (a == "--glow-radius") o.glow.radius = v;
            else if (a == "--glow-threshold") o.glow.threshold = v;
            else if (v == (float)(int)v) o.glow.lobes = (int)v;
            else return refuse("--glow-lobes 1 | 2 | 3 | 4");
        }
        else if (a == "--exposure" || a == "--exposure-speed" || a == "--exposure-range" || a == "--exposure-percentiles") {
            double v[2] = {0.0, 0.0};
            const int n = a == "--exposure" ? 1 : 2;
            for (j = 0; j < n; ++j)
                if (!parse_double(next(), v[j])) return refuse("usage: %s: %s", a.c_str(), n == 1 ? "a number" : "two numbers");
            o.exposure_opts = o.exposure_opts || n == 2;
            if (a == "--exposure") { o.exposure.ev = (float)v[0]; o.use_exposure = true; }
            else if (a == "--exposure-speed") { o.exposure_tau[0] = v[0]; o.exposure_tau[1] = v[1]; }
            else if (a == "--exposure-range") { o.exposure.min_ev = (float)v[0]; o.exposure.max_ev = (float)v[1]; }
            else if (v[0] == (double)(int)v[0] && v[1] == (double)(int)v[1]) { o.exposure.low_permille = (int)v[0]; o.exposure.high_permille = (int)v[1]; }
            else return refuse("usage: --exposure-percentiles LOW HIGH: whole numbers in per mille");
        }
        else if (a == "--auto-exposure") {  // the key is optional: the next argument unless it is another option
            o.use_exposure = true;
            o.exposure.mode = RRT_EXPOSURE_AUTO;
            if (more && strncmp(argv[i + 1], "--", 2) != 0 && !parse_float(next(), o.exposure.key, false))
                return refuse("usage: --auto-exposure [KEY]: a luminance > 0 (default 0.5)");
        }
        else if (a == "--projection") {
            if ((j = one_of(next(), {"pinhole", "equirect", "fisheye"})) < 0) return refuse("--projection pinhole | equirect | fisheye");
            o.projection = j == 0 ? RRT_PROJ_PINHOLE : (j == 1 ? RRT_PROJ_EQUIRECT : RRT_PROJ_FISHEYE);
        }
        else if (a == "--fov" || a == "--vfov") {
            float& v = a == "--fov" ? o.fov : o.vfov;
            if (!parse_float(next(), v, false)) return refuse("%s DEG: a number of degrees", a.c_str());
            if (v == 0.0f) return refuse("%s", kFovRange);
        }
        else if (a == "--stereo") {
            if ((j = one_of(next(), {"top-bottom", "side-by-side"})) < 0) return refuse("usage: --stereo top-bottom | side-by-side");
            o.stereo_layout = j == 0 ? RRT_STEREO_TOP_BOTTOM : RRT_STEREO_SIDE_BY_SIDE;
        }
        else if (a == "--stereo-base" || a == "--convergence" || a == "--pole-merge") {
            float v[2];
            const int n = a == "--pole-merge" ? 2 : 1;
            for (j = 0; j < n; ++j)
                if (!parse_float(next(), v[j], false)) return refuse("usage: %s: a number", a.c_str());
            if (a == "--stereo-base") { o.stereo.base = v[0]; o.stereo_base = true; }
            else if (a == "--convergence") { o.stereo.convergence = v[0]; o.stereo_conv = true; }
            else { o.stereo.pole_merge_from_deg = v[0]; o.stereo.pole_merge_to_deg = v[1]; o.stereo_merge = true; }
        }
        else if (a == "--adaptive") {       // the threshold is optional: the next argument unless it is another option
            o.use_adaptive = true;
            if (more && strncmp(argv[i + 1], "--", 2) != 0) {
                long v;
                if (!parse_whole(next(), v) || v < 0 || v > 255) return refuse("usage: --adaptive [T]: a threshold in 0 ... 255 (default 8)");
                o.adaptive.threshold = (int32_t)v;
            }
        }
        else if (a == "--dof") {
            if (!parse_float(next(), o.dof_aperture, true) || o.dof_aperture < 0.0f) return refuse("%s", kDofAperture);
            o.use_dof = true;
        }
        else if (a == "--focus") {
            o.dof_focus = 0.0f;
            if (strcmp(m = next(), "hole") != 0 && (!parse_float(m, o.dof_focus, true) || !(o.dof_focus > 0.0f)))
                return refuse("usage: --focus: a distance > 0 along forward, or `hole`");
            o.dof_focus_given = true;
        }
        else if (a == "--dof-samples") {
            if (one_of(m = next(), {"1", "2", "4", "8", "16"}) < 0) return refuse("usage: --dof-samples 1 | 2 | 4 | 8 | 16 (lens samples per sub-sample)");
            o.dof_samples = atoi(m);
        }
        else if (a == "--arith" && more) {
            const int mode[] = {RRT_ARITH_STRICT, RRT_ARITH_FMAD, RRT_ARITH_FAST};
            if ((j = one_of(next(), {"strict", "fmad", "fast"})) < 0) return refuse("--arith strict | fmad | fast");
            o.arith = mode[j];
        }
        else return refuse("unknown argument %s", a.c_str());
    }
    return 0;
}

// `path` from the root, "." and ".." resolved by name only (os.path.abspath's rule: the file need not exist)
std::string absolute_path(const std::string& path) {
    return (std::filesystem::current_path() / path).lexically_normal().string();
}

// A file name pattern's frame fields, `%d` or `%0Nd` (sinks.py: frame_fields, frame_name).  frame_name fills every field with k;
// with count it only counts them.
std::string frame_name(const std::string& pattern, int k, int* count = nullptr) {
    std::string out;
    int fields = 0;
    for (size_t i = 0; i < pattern.size();) {
        size_t j = i + 1;
        int width = 0;
        if (pattern[i] == '%' && j < pattern.size() && pattern[j] == '0' && j + 1 < pattern.size() && isdigit((unsigned char)pattern[j + 1]))
            for (++j; j < pattern.size() && isdigit((unsigned char)pattern[j]) && width < 100; ++j) width = width * 10 + (pattern[j] - '0');
        if (pattern[i] == '%' && j < pattern.size() && pattern[j] == 'd') {
            char text[128];
            snprintf(text, sizeof(text), "%0*d", width, k);
            out += text;
            ++fields;
            i = j + 1;
        } else out += pattern[i++];
    }
    if (count) *count = fields;
    return out;
}

// Every refusal that depends on more than one option, in the order that decides which message a command line gets, and the values
// derived from the options.  Host arithmetic and the library's host-only queries: no device is touched before this has returned.
// --exr-layers: the debug launch's planes the layers read, and the standard layers' channels (headless.py: EXR_LAYERS).  type -1:
// --exr-type's
enum { kPlaneRad, kPlaneVel, kPlanePos, kPlaneSteps, kPlaneHit, kLayerPlaneCount };
struct LayerPlane { int words, kind; };
const LayerPlane kLayerPlanes[kLayerPlaneCount] = {{4, RRT_EXR_SRC_F32}, {3, RRT_EXR_SRC_F32}, {3, RRT_EXR_SRC_F32}, {1, RRT_EXR_SRC_I32}, {1, RRT_EXR_SRC_I32}};
struct LayerChannel { const char* layer; const char* name; int type, plane, word; };
const LayerChannel kLayerChannels[] = {
    {"steps", "steps", RRT_EXR_UINT, kPlaneSteps, 0},
    {"horizon", "horizon", RRT_EXR_HALF, kPlaneHit, 0},
    {"transmittance", "transmittance", -1, kPlaneRad, 3},
    {"emission", "emission.B", -1, kPlaneRad, 2}, {"emission", "emission.G", -1, kPlaneRad, 1}, {"emission", "emission.R", -1, kPlaneRad, 0},
    {"direction", "direction.X", RRT_EXR_FLOAT, kPlaneVel, 0}, {"direction", "direction.Y", RRT_EXR_FLOAT, kPlaneVel, 1},
    {"direction", "direction.Z", RRT_EXR_FLOAT, kPlaneVel, 2},
    {"position", "position.X", RRT_EXR_FLOAT, kPlanePos, 0}, {"position", "position.Y", RRT_EXR_FLOAT, kPlanePos, 1},
    {"position", "position.Z", RRT_EXR_FLOAT, kPlanePos, 2},
};

// --exr-layers' refusals (headless.py words them alike) and o.layers: B, G, R of --exr-type from source 0, the HDR plane, next to the
// named layers' channels, in the names' byte order -- the file's
int check_exr_layers(Options& o) {
    int mask = 0;       // bit i: the layer of kLayerNames[i]
    const char* const kLayerNames[] = {"steps", "horizon", "transmittance", "emission", "direction", "position"};
    if (o.exr_layers_arg == "all") mask = 63;
    else for (size_t at = 0; at <= o.exr_layers_arg.size();) {
        size_t end = o.exr_layers_arg.find(',', at);
        if (end == std::string::npos) end = o.exr_layers_arg.size();
        const std::string name = o.exr_layers_arg.substr(at, end - at);
        int i = 0;
        while (i < 6 && name != kLayerNames[i]) ++i;
        if (i == 6) return refuse("usage: --exr-layers LIST: a comma-separated subset of steps,horizon,transmittance,emission,direction,position, or all");
        if (mask & (1 << i)) return refuse("usage: --exr-layers LIST names a layer twice");
        mask |= 1 << i;
        at = end + 1;
    }
    const char* with = o.use_adaptive ? "--adaptive" : o.use_dof ? "--dof" : o.use_stereo ? "--stereo" : o.pano ? "--projection equirect | fisheye"
                     : o.motion > 1 ? "--motion-blur > 1" : o.supersample > 1 ? "--supersample > 1" : nullptr;
    if (with) return refuse("usage: --exr-layers stores per-ray data of the 1x pinhole frame: not with %s", with);
    std::vector<rrt_exr_channel> list;
    auto channel = [&](const char* name, int type, int source, int word) {
        rrt_exr_channel c = {};
        snprintf(c.name, sizeof(c.name), "%s", name);
        c.type = type; c.source = source; c.word = word;
        list.push_back(c);
    };
    o.layers.compression = o.exr.compression;
    o.layers.half_max = o.exr.half_max;
    o.layers.sources[0].words = 4; o.layers.sources[0].kind = RRT_EXR_SRC_F32; o.layers.sources[0].bottom_up = 1;
    o.layers.n_sources = 1;
    channel("B", o.exr.type, 0, 2); channel("G", o.exr.type, 0, 1); channel("R", o.exr.type, 0, 0);
    int* source_of = o.layer_source;
    for (int p = 0; p < kLayerPlaneCount; ++p) source_of[p] = -1;
    for (const LayerChannel& c : kLayerChannels) {
        int i = 0;
        while (strcmp(kLayerNames[i], c.layer) != 0) ++i;
        if (!(mask & (1 << i))) continue;
        if (source_of[c.plane] < 0) {
            rrt_exr_source& src = o.layers.sources[o.layers.n_sources];
            src.words = kLayerPlanes[c.plane].words; src.kind = kLayerPlanes[c.plane].kind; src.bottom_up = 0;
            source_of[c.plane] = o.layers.n_sources++;
            o.layer_planes |= 1 << c.plane;
        }
        channel(c.name, c.type < 0 ? o.exr.type : c.type, source_of[c.plane], c.word);
    }
    std::sort(list.begin(), list.end(), [](const rrt_exr_channel& a, const rrt_exr_channel& b) { return strcmp(a.name, b.name) < 0; });
    o.layers.n_channels = (int32_t)list.size();
    for (size_t i = 0; i < list.size(); ++i) o.layers.channels[i] = list[i];
    if (rrt_exr_layers_frame_bytes(&o.layers, o.w, o.h, &o.exr_bytes, &o.exr_chunks) != RRT_OK) return refuse("bad arguments");
    o.use_layers = true;
    return 0;
}

int check_options(Options& o) {
    if (o.w <= 0 || o.h <= 0 || o.frames < 0 || o.fps <= 0 || o.gpus < 1 || o.tile_rows < 1 || o.slots < 1 || o.slots > kMaxSlots)
        return refuse("bad arguments");
    o.collective = o.gpus > 1 || o.force_collective;
    // the glow needs the whole frame's HDR on one device (rrt_launch_glow has no _tiles form); its settings are checked up front
    if (o.use_glow) {
        if (o.collective) return refuse("rrt_headless: --glow renders on one GPU only (--gpus 1)");
        if (rrt_glow_scratch_bytes(o.w, o.h, &o.glow, &o.glow_bytes) != RRT_OK)
            return refuse("--glow INTENSITY >= 0, --glow-radius R > 0 (a fraction of the height; widest lobe <= 1024 px), "
                          "--glow-threshold T >= 0, --glow-lobes 1 | 2 | 3 | 4");
    }
    // exposure control needs the whole frame's HDR on one device (the meter sees every pixel; rrt_launch_exposure has no _tiles form)
    if (!o.use_exposure && o.exposure_opts)
        return refuse("usage: --exposure-speed / --exposure-range / --exposure-percentiles need --exposure EV | --auto-exposure [KEY]");
    if (o.use_exposure) {
        if (o.collective) return refuse("usage: --exposure / --auto-exposure: one GPU only (--gpus 1)");
        // the settings' ranges are rrt_launch_exposure's own refusals, stated here before any device is touched
        rrt_exposure& e = o.exposure;
        const bool speeds = rrt_exposure_adapt(1.0 / (double)o.fps, o.exposure_tau[0], &e.adapt_up) == RRT_OK &&
                            rrt_exposure_adapt(1.0 / (double)o.fps, o.exposure_tau[1], &e.adapt_down) == RRT_OK &&
                            e.adapt_up > 0.0f && e.adapt_down > 0.0f;
        if (!speeds || !std::isfinite(e.key) || !(e.key > 0.0f) || !(e.min_ev <= e.max_ev) ||
            e.low_permille < 0 || e.high_permille < 0 || (long long)e.low_permille + e.high_permille >= 1000)
            return refuse("usage: --auto-exposure KEY > 0, --exposure-speed UP DOWN >= 0 (seconds), --exposure-range MIN MAX with MIN <= MAX, "
                          "--exposure-percentiles LOW HIGH >= 0 with LOW + HIGH < 1000");
        o.auto_exposure = e.mode == RRT_EXPOSURE_AUTO;
    }
    // panoramas: the spans are checked by the host query (the launch's own refusals), the combinations the kernels lack up front
    o.pano = o.projection != RRT_PROJ_PINHOLE;
    rrt_projection_default(o.projection, &o.proj);
    if (!o.pano && (o.fov != 0.0f || o.vfov != 0.0f)) return refuse("--fov / --vfov need --projection equirect | fisheye");
    if (o.projection == RRT_PROJ_FISHEYE && o.vfov != 0.0f) return refuse("--vfov: equirect only (a fisheye's aperture is --fov)");
    if (o.fov != 0.0f) o.proj.fov_deg = o.fov;
    if (o.vfov != 0.0f) o.proj.vfov_deg = o.vfov;
    const rrt_camera c0 = {};
    float org[3], dir[3];
    if (o.pano) {
        if (rrt_projection_ray(&o.proj, 1, 1, 0, 0, &c0, dir, nullptr) != RRT_OK) return refuse("%s", kFovRange);
        if (o.motion > 1) return refuse("rrt_headless: a panorama renders one instant per frame (--motion-blur 1)");
        if (o.projection == RRT_PROJ_EQUIRECT && o.use_glow)
            return refuse("rrt_headless: --glow clamps at the frame's edge and an equirect frame wraps: not with --projection equirect");
    }
    // stereo: the values are checked by the host query (the launch's own refusals), the combinations the kernel lacks up front;
    // --width / --height stay per eye (ew x eh, what the launch takes), w x h becomes the composite that is sharded and written
    o.use_stereo = o.stereo_layout != 0;
    o.ew = o.w; o.eh = o.h;
    if (!o.use_stereo && (o.stereo_base || o.stereo_conv || o.stereo_merge))
        return refuse("usage: --stereo-base / --convergence / --pole-merge need --stereo top-bottom | side-by-side");
    if (o.use_stereo) {
        o.stereo.layout = o.stereo_layout;
        if (o.projection == RRT_PROJ_FISHEYE) return refuse("usage: --stereo: pinhole or equirect (no stereo fisheye domes)");
        if (o.motion > 1) return refuse("usage: --stereo renders one instant per frame (--motion-blur 1)");
        if (o.use_glow) return refuse("usage: --stereo: not with --glow");
        if (o.stereo_conv && o.projection != RRT_PROJ_PINHOLE) return refuse("usage: --convergence: pinhole only");
        if (o.stereo_merge && o.projection != RRT_PROJ_EQUIRECT) return refuse("usage: --pole-merge: equirect only");
        if (rrt_stereo_ray(&o.proj, &o.stereo, 1, 1, RRT_EYE_LEFT, 0, 0, &c0, org, dir, nullptr) != RRT_OK)
            return refuse("usage: --stereo-base B >= 0, --convergence Z >= 0, --pole-merge FROM TO with 0 <= FROM <= TO <= 90");
        if (o.stereo_layout == RRT_STEREO_SIDE_BY_SIDE) o.w = 2 * o.ew; else o.h = 2 * o.eh;
    }
    // adaptive supersampling needs the whole frame on one device (the mask looks at every pixel's neighbours; no _tiles form)
    if (o.use_adaptive) {
        if (o.supersample <= 1) return refuse("usage: --adaptive needs --supersample 2 | 4 | 8");
        if (o.collective) return refuse("usage: --adaptive renders on one GPU only (--gpus 1)");
        if (o.motion > 1) return refuse("usage: --adaptive renders one instant per frame (--motion-blur 1)");
        if (o.use_stereo) return refuse("usage: --adaptive: not with --stereo");
    }
    // depth of field: a thin lens in front of the pinhole camera; its K samples are the shutter's sub-frames when there are any
    if (!o.use_dof && (o.dof_focus_given || o.dof_samples != 0)) return refuse("usage: --focus / --dof-samples need --dof APERTURE");
    if (o.use_dof) {
        if (o.pano) return refuse("usage: --dof: a thin lens in front of a pinhole camera, not with --projection equirect | fisheye");
        if (o.use_stereo) return refuse("usage: --dof: not with --stereo");
        if (o.use_adaptive) return refuse("usage: --dof: not with --adaptive");
        if (o.motion > 1 && o.dof_samples != 0 && o.dof_samples != o.motion)
            return refuse("usage: --dof-samples: with --motion-blur M > 1 the lens samples are the shutter's sub-frames (K = M)");
        o.dof_k = o.motion > 1 ? o.motion : (o.dof_samples != 0 ? o.dof_samples : 8);
        float spiral[32];
        if (rrt_lens_points(o.dof_aperture, o.dof_k, 0.0f, spiral) != RRT_OK) return refuse("%s", kDofAperture);
        for (int m = 0; m < o.dof_k; ++m) {       // sample m looks through lens point bitrev_K(m): the spiral's radius grows with its index
            int r = 0;
            for (int b = 1, v = m; b < o.dof_k; b <<= 1, v >>= 1) r = (r << 1) | (v & 1);
            o.dof_xy[2 * m] = spiral[2 * r]; o.dof_xy[2 * m + 1] = spiral[2 * r + 1];
        }
    }
    // Y4M output (headless.py words these alike): depth 10 reads the frame's linear HDR, whole, on one device
    o.y4m = !o.y4m_path.empty();
    o.y4m_pq = o.y4m_transfer == 1;
    if (!o.y4m_pq && o.hdr_opts) return refuse("usage: --hdr-white / --hdr-peak / --hdr-knee need --y4m-transfer pq");
    if (o.y4m_pq && (!o.y4m || o.yuv.bits != 10)) return refuse("usage: --y4m-transfer pq needs --y4m PATH and --y4m-depth 10");
    if (!o.hdr_nits_ok) return refuse("usage: --hdr-white / --hdr-peak NITS: in (0, 10000]");
    if (!o.hdr_knee_ok) return refuse("usage: --hdr-knee F: in [0, 1]");
    if (!o.y4m && o.y4m_transfer >= 0) return refuse("usage: --y4m-transfer needs --y4m PATH");
    if (!o.y4m && o.y4m_opts) return refuse("usage: --y4m-chroma / --y4m-range / --y4m-depth need --y4m PATH");
    if (o.y4m) {
        o.y4m10 = o.yuv.bits == 10;
        if (o.y4m10 && o.use_glow)
            return refuse("usage: --y4m-depth 10 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow");
        if (o.y4m10 && o.collective) return refuse("usage: --y4m-depth 10: one GPU only (--gpus 1)");
        if (!o.out_path.empty() && absolute_path(o.y4m_path) == absolute_path(o.out_path)) return refuse("usage: --y4m and --out name the same file");
        if (rrt_yuv_frame_bytes(&o.yuv, o.w, o.h, &o.yuv_bytes, nullptr) != RRT_OK) return refuse("bad arguments");
    }
    // EXR output (headless.py words these alike): the frame's linear HDR, whole, on one device
    o.use_exr = !o.exr_path.empty();
    if (!o.use_exr && o.exr_opts) return refuse("usage: --exr-type / --exr-compression / --exr-level need --exr PATTERN");
    if (o.use_exr) {
        if (o.exr_type < 0) return refuse("usage: --exr-type half | float");
        if (o.exr_compression < 0) return refuse("usage: --exr-compression none | zips | zip");
        if (o.exr_level < 1) return refuse("usage: --exr-level 1 ... 9");
        if (o.use_glow) return refuse("usage: --exr reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow");
        if (o.collective) return refuse("usage: --exr: one GPU only (--gpus 1)");
        int fields = 0;
        frame_name(o.exr_path, 0, &fields);
        if (fields > 1) return refuse("usage: --exr PATTERN: one frame field (%%d or %%0Nd)");
        if (fields == 0 && o.frames > 1)
            return refuse("usage: --exr PATTERN needs a frame field (%%04d) when --frames > 1: the frames would overwrite one another");
        for (int k = 1; k <= (o.frames > 1 ? o.frames : 1); ++k) {
            const std::string name = absolute_path(frame_name(o.exr_path, k));
            if (!o.out_path.empty() && name == absolute_path(o.out_path)) return refuse("usage: --exr and --out name the same file");
            if (o.y4m && name == absolute_path(o.y4m_path)) return refuse("usage: --exr and --y4m name the same file");
        }
        const int types[] = {RRT_EXR_HALF, RRT_EXR_FLOAT}, compressions[] = {RRT_EXR_NONE, RRT_EXR_ZIPS, RRT_EXR_ZIP};
        o.exr.type = types[o.exr_type];
        o.exr.compression = compressions[o.exr_compression];
        if (rrt_exr_frame_bytes(&o.exr, o.w, o.h, &o.exr_bytes, &o.exr_chunks) != RRT_OK) return refuse("bad arguments");
    }
    if (!o.use_exr && o.exr_layers_given) return refuse("usage: --exr-layers needs --exr PATTERN");
    if (o.exr_layers_given) { const int rc = check_exr_layers(o); if (rc) return rc; }
    // PNG output (headless.py words these alike): depth 8 converts the assembled RGBA8 frame, in every mode; depth 16 reads the
    // frame's linear HDR, whole, on one device
    o.use_png = !o.png_path.empty();
    if (!o.use_png && o.png_opts) return refuse("usage: --png-depth / --png-filter / --png-level need --png PATTERN");
    if (!o.use_png && o.png_deflate_opt) return refuse("usage: --png-deflate needs --png PATTERN");
    if (o.use_png) {
        if (o.png_depth < 0) return refuse("usage: --png-depth 8 | 16");
        if (o.png_filter < 0) return refuse("usage: --png-filter adaptive | none | sub | up | average | paeth");
        if (o.png_level < 1) return refuse("usage: --png-level 1 ... 9");
        if (o.png_deflate < 0) return refuse("usage: --png-deflate host | device");
        if (o.png_deflate == 1 && o.png_level_opt) return refuse("usage: --png-level is the host zlib's level: not with --png-deflate device");
        o.png16 = o.png_depth == 1;
        if (o.png16 && o.use_glow)
            return refuse("usage: --png-depth 16 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow");
        if (o.png16 && o.collective) return refuse("usage: --png-depth 16: one GPU only (--gpus 1)");
        int fields = 0;
        frame_name(o.png_path, 0, &fields);
        if (fields > 1) return refuse("usage: --png PATTERN: one frame field (%%d or %%0Nd)");
        if (fields == 0 && o.frames > 1)
            return refuse("usage: --png PATTERN needs a frame field (%%04d) when --frames > 1: the frames would overwrite one another");
        for (int k = 1; k <= (o.frames > 1 ? o.frames : 1); ++k) {
            const std::string name = absolute_path(frame_name(o.png_path, k));
            if (!o.out_path.empty() && name == absolute_path(o.out_path)) return refuse("usage: --png and --out name the same file");
            if (o.y4m && name == absolute_path(o.y4m_path)) return refuse("usage: --png and --y4m name the same file");
            if (o.use_exr && name == absolute_path(frame_name(o.exr_path, k))) return refuse("usage: --png and --exr name the same file");
        }
        const int filters[] = {RRT_PNG_ADAPTIVE, RRT_PNG_NONE, RRT_PNG_SUB, RRT_PNG_UP, RRT_PNG_AVERAGE, RRT_PNG_PAETH};
        o.png.depth = o.png16 ? 16 : 8;
        o.png.filter = filters[o.png_filter];
        if (rrt_png_frame_bytes(&o.png, o.w, o.h, &o.png_bytes, &o.png_stride, &o.png_sum_bytes) != RRT_OK ||
            rrt_png_slices(&o.png, o.w, o.h, &o.png_slice_rows, &o.png_slices) != RRT_OK) return refuse("bad arguments");
        if (o.png_deflate == 1 && rrt_deflate_plan(o.png_bytes, (size_t)o.png_slice_rows * o.png_stride, nullptr, nullptr, &o.dfl_bound, &o.dfl_scratch) != RRT_OK)
            return refuse("bad arguments");
    }
    o.hdr_frame = o.use_glow || o.use_exposure || o.y4m10 || o.use_exr || o.png16;
    // a supersampled launch is always the single kernel in the static order (include/rrt.h): no pool, no path choice, no tile order
    if (o.supersample > 1 || o.motion > 1 || o.hdr_frame || o.pano || o.use_stereo || o.use_dof) {
        o.workspace_gib = 0; o.path_window = -1; o.tile_order = 0;
    }
    return 0;
}

// ---- the run's resources

// --png: a slot's buffer holds the payload, then -- on the next 16 bytes -- the row sums; one copy brings both to the host
size_t png_table_offset(const Options& o) { return (o.png_bytes + 15) & ~(size_t)15; }
// --png-deflate device: the payload stays on the device.  A small buffer holds the streams' sizes and -- on the next 16 bytes -- the row
// sums; it is copied first, and then exactly the streams' bytes, which land behind it in the pinned buffer
size_t png_meta_offset(const Options& o) { return (4 * (size_t)o.png_slices + 15) & ~(size_t)15; }
size_t png_meta_bytes(const Options& o) { return (png_meta_offset(o) + o.png_sum_bytes + 15) & ~(size_t)15; }

struct Slots {                 // what device 0 owns per frame slot: gathered shards + assembled frame, the pinned host frame for the sink
    void* gathered[kMaxSlots] = {};
    void* frame[kMaxSlots] = {};
    void* host[kMaxSlots] = {};
    void* yuv[kMaxSlots] = {};             // --y4m: each slot's packed planes on device 0, and the pinned host copy for the sink
    void* yuv_host[kMaxSlots] = {};
    void* exr[kMaxSlots] = {};             // --exr: each slot's packed chunks on device 0, and the pinned host copy the files are made of
    void* exr_host[kMaxSlots] = {};
    void* png[kMaxSlots] = {};             // --png: each slot's filtered scanlines, then its row sums, on device 0, and their pinned host copy
    void* png_host[kMaxSlots] = {};
    void* png_meta[kMaxSlots] = {};        // --png-deflate device: sizes and row sums, the streams, the launch's scratch
    void* dfl_out[kMaxSlots] = {};
    void* dfl_scratch[kMaxSlots] = {};
    void* layer_plane[kLayerPlaneCount][kMaxSlots] = {};      // --exr-layers: each slot's planes of the debug launch
    void* hdr[kMaxSlots] = {};             // --glow / --exposure / --y4m-depth 10 / --exr: each slot's linear frame; the glow's scratch
    void* glow_scratch[kMaxSlots] = {};
    void* ad_scratch[kMaxSlots] = {};      // --adaptive: each slot's list, and the pinned word its count is copied to
    void* ad_count[kMaxSlots] = {};
    hipEvent_t done[kMaxSlots] = {};
    size_t shard_stride = 0;               // bytes between shards in the gathered buffer
    size_t frame_bytes = 0, ad_bytes = 0;
    // --auto-exposure: ONE state for the sequence.  The frames' renders overlap on their slots' streams; their exposure passes run in
    // frame order, each behind the event its predecessor recorded
    void* exposure_scratch = nullptr;
    size_t exposure_bytes = 0;
    hipEvent_t exposed = nullptr;
    // --y4m-transfer pq: ONE light-level state for the film, in the same way -- a frame's pack and fold run behind its predecessor's
    void* light = nullptr;
    hipEvent_t lit = nullptr;
};

// each device's shard of the frame; the stride between shards in the gathered buffer
void plan_shards(const Options& o, std::vector<Device>& dev, Slots& R) {
    for (int d = 0; d < o.gpus; ++d) {
        int rows = 0;
        rrt_tile_shard_rows(o.h, o.tile_rows, d, o.gpus, &rows);
        dev[d].id = d;
        dev[d].shard_rows = rows;
        if ((size_t)rows * o.w * 4 > R.shard_stride) R.shard_stride = (size_t)rows * o.w * 4;
    }
    R.shard_stride = (R.shard_stride + 255) & ~(size_t)255;
}

int create_device(Device& D, const Options& o, const std::vector<uint8_t>& sky, int sky_w, int sky_h, size_t shard_stride) {
    int rc;
    HIPCHK(hipSetDevice(D.id));
    const int rows = o.collective ? D.shard_rows : o.h;            // image rows of one launch on this device
    if ((rc = rrt_sky_create(sky.data(), sky_w, sky_h, &D.sky)) != RRT_OK) return fail("sky", rc);
    HIPCHK(hipMalloc(&D.probe, 256 * (size_t)(o.gpus + 1)));
    HIPCHK(hipEventCreateWithFlags(&D.comm_free, hipEventDisableTiming));
    const bool three_pass_likely = o.workspace_gib > 0 && (long long)o.w * rows <= (long long)rrt_path_auto_max_rays();   // RRT_PATH_AUTO's own threshold
    // the path is a choice only where a launch could take either: a pool, a share under RRT_PATH_AUTO's threshold, frames in
    // flight (one frame at a time the three-pass path's two chains win: DESIGN.md section 5)
    if (o.path_window >= 0 && o.slots >= 2 && three_pass_likely) {
        if ((rc = rrt_path_chooser_create(o.slots, o.path_window, &D.chooser)) != RRT_OK) return fail("path chooser", rc);
        for (int e = 0; e < 2 * o.slots; ++e) HIPCHK(hipEventCreate(&D.render_end[e]));
    }
    for (int s = 0; s < o.slots; ++s) {
        HIPCHK(hipStreamCreateWithFlags(&D.stream[s], hipStreamNonBlocking));
        HIPCHK(hipMalloc(&D.tiles[s], shard_stride));
        if (o.workspace_gib > 0 && (rc = rrt_workspace_create(((size_t)o.workspace_gib << 30) / o.slots, &D.pool[s])) != RRT_OK)
            return fail("workspace", rc);
        // every frame's wave tiles dispatched longest-first by what the slot's previous frame measured (the first frame: by
        // the library's probe of the view): worth it when the frames do not overlap (their drains are exposed) AND the
        // launch takes the single kernel; a wash when frames overlap, and measured harmful on the three-pass path's two
        // chains (it piles every expensive tile into the first chain: an eighth of a 4K frame 5.15 -> 5.45 ms, of a
        // disk-heavy one 7.7 -> 10.6; profiles/r04_shard_kernel_times_*.txt), which is what small launches with a pool take
        if ((o.tile_order == 1 || (o.tile_order < 0 && o.slots == 1 && !three_pass_likely)) && (rc = rrt_tile_order_create(&D.order[s])) != RRT_OK)
            return fail("tile order", rc);
    }
    return 0;
}

void destroy_device(Device& D, int slots) {
    if (D.comm) ncclCommDestroy(D.comm);
    (void)hipFree(D.probe);
    (void)hipEventDestroy(D.comm_free);
    if (D.chooser) { rrt_path_chooser_destroy(D.chooser); for (int e = 0; e < 2 * slots; ++e) (void)hipEventDestroy(D.render_end[e]); }
    for (int s = 0; s < slots; ++s) {
        if (D.pool[s]) rrt_workspace_destroy(D.pool[s]);
        if (D.order[s]) rrt_tile_order_destroy(D.order[s]);
        (void)hipFree(D.tiles[s]);
        (void)hipStreamDestroy(D.stream[s]);
    }
    if (D.noise_table) rrt_noise_table_destroy(D.noise_table);
    rrt_sky_destroy(D.sky);
}

// one RCCL communicator per device, and one untimed exchange of a few bytes
int create_communicators(std::vector<Device>& dev, std::thread& warm) {
    const int gpus = (int)dev.size();
    std::vector<int> ids(gpus);
    std::vector<ncclComm_t> comms(gpus);
    for (int d = 0; d < gpus; ++d) ids[d] = d;
    if (warm.joinable()) { trace("waiting for the RCCL library pages"); warm.join(); }
    trace("ncclCommInitAll ...");
    NCCLCHK(ncclCommInitAll(comms.data(), gpus, ids.data()));
    trace("ncclCommInitAll done");
    for (int d = 0; d < gpus; ++d) dev[d].comm = comms[d];
    { std::lock_guard<std::mutex> lk(g_tr.mu); g_tr.comms = comms; }
    // One untimed exchange of a few bytes brings up the peer-to-peer channels and loads RCCL's code object now, under
    // the bring-up limit, instead of under frame 1's.
    trace("first exchange (channel set-up) ...");
    NCCLCHK(ncclGroupStart());
    for (int d = 0; d < gpus; ++d) {
        NCCLCHK(ncclSend(dev[d].probe, 256, ncclUint8, 0, dev[d].comm, dev[d].stream[0]));
        NCCLCHK(ncclRecv(static_cast<uint8_t*>(dev[0].probe) + 256 * (size_t)(d + 1), 256, ncclUint8, d, dev[0].comm, dev[0].stream[0]));
    }
    NCCLCHK(ncclGroupEnd());
    for (int d = 0; d < gpus; ++d) { HIPCHK(hipSetDevice(d)); HIPCHK(hipStreamSynchronize(dev[d].stream[0])); }
    trace("first exchange done");
    return 0;
}

// device 0's per-slot buffers (pinned host frames only with a sink; --y4m's planes and their pinned copy) and the sequence's exposure state
int create_slots(Slots& R, const Options& o, bool sink, hipStream_t stream0) {
    int rc;
    HIPCHK(hipSetDevice(0));
    if (o.auto_exposure) {
        if ((rc = rrt_exposure_scratch_bytes(&R.exposure_bytes)) != RRT_OK) return fail("exposure scratch", rc);
        HIPCHK(hipMalloc(&R.exposure_scratch, R.exposure_bytes));
        HIPCHK(hipEventCreateWithFlags(&R.exposed, hipEventDisableTiming));
        if ((rc = rrt_launch_exposure_reset(R.exposure_scratch, R.exposure_bytes, stream0)) != RRT_OK) return fail("exposure reset", rc);
    }
    if (o.y4m_pq) {
        size_t light_bytes = 0;
        if ((rc = rrt_yuv_hdr10_light_bytes(&light_bytes)) != RRT_OK) return fail("hdr10 light state", rc);
        HIPCHK(hipMalloc(&R.light, light_bytes));
        HIPCHK(hipEventCreateWithFlags(&R.lit, hipEventDisableTiming));
        if ((rc = rrt_launch_yuv_hdr10_light_reset(R.light, stream0)) != RRT_OK) return fail("hdr10 light reset", rc);
    }
    if (o.use_adaptive && (rc = rrt_adaptive_scratch_bytes(o.w, o.h, &R.ad_bytes)) != RRT_OK) return fail("adaptive scratch", rc);
    R.frame_bytes = (size_t)o.w * o.h * 4;
    for (int s = 0; s < o.slots; ++s) {
        HIPCHK(hipMalloc(&R.gathered[s], R.shard_stride * o.gpus));
        HIPCHK(hipMalloc(&R.frame[s], R.frame_bytes));
        if (o.hdr_frame) HIPCHK(hipMalloc(&R.hdr[s], R.frame_bytes * sizeof(float)));
        if (o.y4m) { HIPCHK(hipMalloc(&R.yuv[s], o.yuv_bytes)); HIPCHK(hipHostMalloc(&R.yuv_host[s], o.yuv_bytes, hipHostMallocDefault)); }
        if (o.use_exr) { HIPCHK(hipMalloc(&R.exr[s], o.exr_bytes)); HIPCHK(hipHostMalloc(&R.exr_host[s], o.exr_bytes, hipHostMallocDefault)); }
        if (o.use_png) {
            HIPCHK(hipMalloc(&R.png[s], png_table_offset(o) + o.png_sum_bytes));
            HIPCHK(hipHostMalloc(&R.png_host[s], o.png_deflate == 1 ? png_meta_bytes(o) + o.dfl_bound : png_table_offset(o) + o.png_sum_bytes, hipHostMallocDefault));
            if (o.png_deflate == 1) {
                HIPCHK(hipMalloc(&R.png_meta[s], png_meta_bytes(o)));
                HIPCHK(hipMalloc(&R.dfl_out[s], o.dfl_bound));
                HIPCHK(hipMalloc(&R.dfl_scratch[s], o.dfl_scratch));
            }
        }
        for (int p = 0; p < kLayerPlaneCount; ++p)
            if (o.layer_planes & (1 << p)) HIPCHK(hipMalloc(&R.layer_plane[p][s], (size_t)o.w * o.h * 4 * kLayerPlanes[p].words));
        if (o.use_glow) HIPCHK(hipMalloc(&R.glow_scratch[s], o.glow_bytes));
        if (o.use_adaptive) { HIPCHK(hipMalloc(&R.ad_scratch[s], R.ad_bytes)); HIPCHK(hipHostMalloc(&R.ad_count[s], 4, hipHostMallocDefault)); }
        HIPCHK(hipEventCreateWithFlags(&R.done[s], hipEventDisableTiming));
    }
    if (sink) for (int s = 0; s < o.slots; ++s) HIPCHK(hipHostMalloc(&R.host[s], R.frame_bytes, hipHostMallocDefault));
    return 0;
}

void destroy_slots(Slots& R, int slots) {
    (void)hipFree(R.exposure_scratch);
    if (R.exposed) (void)hipEventDestroy(R.exposed);
    (void)hipFree(R.light);
    if (R.lit) (void)hipEventDestroy(R.lit);
    for (int s = 0; s < slots; ++s) {
        (void)hipFree(R.gathered[s]); (void)hipFree(R.frame[s]); (void)hipFree(R.hdr[s]); (void)hipFree(R.glow_scratch[s]);
        (void)hipFree(R.ad_scratch[s]); (void)hipFree(R.yuv[s]);
        if (R.yuv_host[s]) (void)hipHostFree(R.yuv_host[s]);
        (void)hipFree(R.exr[s]);
        (void)hipFree(R.png[s]);
        (void)hipFree(R.png_meta[s]);
        (void)hipFree(R.dfl_out[s]);
        (void)hipFree(R.dfl_scratch[s]);
        if (R.png_host[s]) (void)hipHostFree(R.png_host[s]);
        for (int p = 0; p < kLayerPlaneCount; ++p) (void)hipFree(R.layer_plane[p][s]);
        if (R.exr_host[s]) (void)hipHostFree(R.exr_host[s]);
        if (R.ad_count[s]) (void)hipHostFree(R.ad_count[s]);
        if (R.host[s]) (void)hipHostFree(R.host[s]);
        (void)hipEventDestroy(R.done[s]);
    }
}

// ---- EXR files (include/rrt_exr.h, step 5; sinks.py: EXRSink)

// One frame's file from its payload in host memory: every chunk deflated (zlib, `level`) on up to `threads` threads -- the chunks are
// independent --, a chunk that deflate does not shrink stored raw, un-filtered; header, offset table, chunks into NAME.tmp, renamed.
int write_exr_file(const std::string& name, const uint8_t* payload, const Options& o, int threads) {
    struct Piece { int32_t y = 0; size_t offset = 0, bytes = 0; std::vector<uint8_t> data; };
    std::vector<Piece> pieces((size_t)o.exr_chunks);
    for (int i = 0; i < o.exr_chunks; ++i)
        if ((o.use_layers ? rrt_exr_layers_chunk(&o.layers, o.w, o.h, i, &pieces[i].y, &pieces[i].offset, &pieces[i].bytes)
                          : rrt_exr_chunk(&o.exr, o.w, o.h, i, &pieces[i].y, &pieces[i].offset, &pieces[i].bytes)) != RRT_OK) return 1;
    if (o.exr.compression != RRT_EXR_NONE) {
        std::atomic<int> next{0}, failed{0};
        auto work = [&]() {
            for (int i; (i = next.fetch_add(1)) < o.exr_chunks;) {
                Piece& c = pieces[i];
                uLongf n = compressBound((uLong)c.bytes);
                c.data.resize(n);
                if (compress2(c.data.data(), &n, payload + c.offset, (uLong)c.bytes, o.exr_level) != Z_OK) { failed.store(1); return; }
                if (n < c.bytes) { c.data.resize(n); continue; }
                c.data.resize(c.bytes);
                if (rrt_exr_unfilter_host(c.data.data(), payload + c.offset, c.bytes) != RRT_OK) { failed.store(1); return; }
            }
        };
        const int n_threads = threads < o.exr_chunks ? threads : o.exr_chunks;
        std::vector<std::thread> pool;
        for (int t = 1; t < n_threads; ++t) pool.emplace_back(work);
        work();
        for (std::thread& t : pool) t.join();
        if (failed.load()) { fprintf(stderr, "rrt_headless: exr: deflate failed\n"); return 1; }
    }
    uint8_t header[2048];
    size_t header_bytes = 0;
    if ((o.use_layers ? rrt_exr_layers_header(&o.layers, o.w, o.h, o.fps, 1, header, sizeof(header), &header_bytes)
                      : rrt_exr_header(&o.exr, o.w, o.h, o.fps, 1, header, sizeof(header), &header_bytes)) != RRT_OK) {
        fprintf(stderr, "rrt_headless: exr header: %s\n", rrt_exr_last_error());
        return 1;
    }
    const std::string tmp = name + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { perror("fopen"); return 1; }
    bool ok = fwrite(header, 1, header_bytes, f) == header_bytes;
    uint64_t at = header_bytes + 8 * (uint64_t)o.exr_chunks;
    auto put = [&](uint64_t v, int n) {     // little-endian
        uint8_t b[8];
        for (int k = 0; k < n; ++k) b[k] = (uint8_t)(v >> (8 * k));
        ok = ok && fwrite(b, 1, (size_t)n, f) == (size_t)n;
    };
    for (const Piece& c : pieces) {
        put(at, 8);
        at += 8 + (o.exr.compression != RRT_EXR_NONE ? c.data.size() : c.bytes);
    }
    for (const Piece& c : pieces) {
        const bool raw = o.exr.compression == RRT_EXR_NONE;
        const size_t n = raw ? c.bytes : c.data.size();
        put((uint32_t)c.y, 4);
        put((uint32_t)n, 4);
        ok = ok && fwrite(raw ? payload + c.offset : c.data.data(), 1, n, f) == n;
    }
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), name.c_str()) != 0) { fprintf(stderr, "rrt_headless: exr: cannot write %s\n", name.c_str()); return 1; }
    return 0;
}

// ---- PNG files (include/rrt_png.h, step 6; sinks.py: PNGSink)

// the file around its IDAT pieces: the header's chunks, one IDAT per piece, IEND; NAME.tmp, then renamed
int write_png_pieces(const std::string& name, const std::vector<std::vector<uint8_t>>& pieces, const Options& o) {
    uint8_t header[256];
    size_t header_bytes = 0;
    if (rrt_png_header(&o.png, o.w, o.h, header, sizeof(header), &header_bytes) != RRT_OK) {
        fprintf(stderr, "rrt_headless: png header: %s\n", rrt_png_last_error());
        return 1;
    }
    const std::string tmp = name + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) { perror("fopen"); return 1; }
    bool ok = fwrite(header, 1, header_bytes, f) == header_bytes;
    auto chunk = [&](const char* type, const uint8_t* data, size_t n) {       // length, type, data, CRC-32 of type and data; big-endian
        uint8_t b[8] = {(uint8_t)(n >> 24), (uint8_t)(n >> 16), (uint8_t)(n >> 8), (uint8_t)n, (uint8_t)type[0], (uint8_t)type[1], (uint8_t)type[2], (uint8_t)type[3]};
        uLong crc = crc32(0L, b + 4, 4);
        if (n) crc = crc32(crc, data, (uInt)n);
        ok = ok && fwrite(b, 1, 8, f) == 8 && (n == 0 || fwrite(data, 1, n, f) == n);
        const uint8_t c[4] = {(uint8_t)(crc >> 24), (uint8_t)(crc >> 16), (uint8_t)(crc >> 8), (uint8_t)crc};
        ok = ok && fwrite(c, 1, 4, f) == 4;
    };
    for (const std::vector<uint8_t>& piece : pieces) chunk("IDAT", piece.data(), piece.size());
    chunk("IEND", nullptr, 0);
    ok = (fclose(f) == 0) && ok;
    if (!ok || rename(tmp.c_str(), name.c_str()) != 0) { fprintf(stderr, "rrt_headless: png: cannot write %s\n", name.c_str()); return 1; }
    return 0;
}

// One frame's file from its payload and row sums in host memory: the slices deflated (zlib, `level`, Z_FILTERED as PNGSink; raw
// streams that end on a sync flush, the last on a finish) on up to `threads` threads, one IDAT each; the Adler-32 from the row sums.
int write_png_file(const std::string& name, const uint8_t* payload, const uint32_t* row_sums, const Options& o, int threads) {
    std::vector<std::vector<uint8_t>> pieces((size_t)o.png_slices);
    uint32_t adler = 0;
    if (rrt_png_adler32(row_sums, o.w, o.h, &o.png, &adler) != RRT_OK) return 1;
    const size_t step = (size_t)o.png_slice_rows * o.png_stride;
    std::atomic<int> next{0}, failed{0};
    auto work = [&]() {
        for (int i; (i = next.fetch_add(1)) < o.png_slices;) {
            const bool first = i == 0, last = i == o.png_slices - 1;
            const size_t from = (size_t)i * step, n = last ? o.png_bytes - from : step;
            z_stream z;
            memset(&z, 0, sizeof(z));
            if (deflateInit2(&z, o.png_level, Z_DEFLATED, -15, 8, Z_FILTERED) != Z_OK) { failed.store(1); return; }
            std::vector<uint8_t>& out = pieces[i];
            out.resize((first ? 2 : 0) + deflateBound(&z, (uLong)n) + 16 + (last ? 4 : 0));
            if (first) { out[0] = 0x78; out[1] = 0x01; }
            z.next_in = const_cast<Bytef*>(payload + from);
            z.avail_in = (uInt)n;
            z.next_out = out.data() + (first ? 2 : 0);
            z.avail_out = (uInt)(out.size() - (first ? 2 : 0) - (last ? 4 : 0));
            const int rc = deflate(&z, last ? Z_FINISH : Z_SYNC_FLUSH);
            const bool done = last ? rc == Z_STREAM_END : (rc == Z_OK && z.avail_in == 0 && z.avail_out != 0);
            size_t at = (first ? 2 : 0) + (size_t)z.total_out;
            deflateEnd(&z);
            if (!done) { failed.store(1); return; }
            if (last) for (int b = 3; b >= 0; --b) out[at++] = (uint8_t)(adler >> (8 * b));
            out.resize(at);
        }
    };
    const int n_threads = threads < o.png_slices ? threads : o.png_slices;
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; ++t) pool.emplace_back(work);
    work();
    for (std::thread& t : pool) t.join();
    if (failed.load()) { fprintf(stderr, "rrt_headless: png: deflate failed\n"); return 1; }
    return write_png_pieces(name, pieces, o);
}

// The same file from slices that are deflated already (--png-deflate device; sinks.py: PNGSink.write_streams): `streams` holds them back
// to back, sizes[i] bytes each
int write_png_streams(const std::string& name, const uint8_t* streams, const uint32_t* sizes, const uint32_t* row_sums, const Options& o) {
    std::vector<std::vector<uint8_t>> pieces((size_t)o.png_slices);
    uint32_t adler = 0;
    if (rrt_png_adler32(row_sums, o.w, o.h, &o.png, &adler) != RRT_OK) return 1;
    size_t at = 0;
    for (int i = 0; i < o.png_slices; ++i) {
        std::vector<uint8_t>& out = pieces[(size_t)i];
        if (i == 0) { out.push_back(0x78); out.push_back(0x01); }
        out.insert(out.end(), streams + at, streams + at + sizes[i]);
        at += sizes[i];
        if (i == o.png_slices - 1) for (int b = 3; b >= 0; --b) out.push_back((uint8_t)(adler >> (8 * b)));
    }
    return write_png_pieces(name, pieces, o);
}

// the deflate pool's size: the CPUs this process may run on, 16 at the most
int deflate_threads() {
    cpu_set_t set;
    const int n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : 1;
    return n < 1 ? 1 : (n > 16 ? 16 : n);
}

// ---- the frame loop

// The devices' noise tables over a sliding window of the clock (relativisticraytracer_amd/__init__.py: NoiseWindows).
struct NoiseWindow {
    bool enabled;
    size_t budget;
    float seq_end;                               // the recording clock's last time + 1 s: the tables slide along it
    float t0 = 0.0f, t1 = -1.0f;                 // the window the devices' tables (or the remembered failure) cover; empty at first
    bool has_table = false, warned = false;
    int builds = 0, table_frames = 0, arith_frames = 0, coarsest = RRT_TABLE_FULL;
    size_t peak = 0;

    // Frame k reads the noise from fit_t on.  When the clock has left the window, every device builds the next one (after its frames
    // in flight, which may still read the old table, have drained).  The window is ONE decision for all devices: if it
    // cannot be built on any of them (nothing fits the budget, out of memory) it is dropped on all of them and
    // REMEMBERED -- no new fit, no device synchronise, no retry until the clock has left it (retrying
    // every frame serialised the frames in flight and rebuilt the other devices' tables for nothing).
    int slide(float fit_t, int k, std::vector<Device>& dev) {
        if (enabled && !(fit_t >= t0 && fit_t <= t1)) {
            float end = fit_t; int cov = RRT_TABLE_FULL; size_t bytes = 0;
            // trace points around the rebuild: it synchronises every device and creates a table on each, which on a
            // starved box takes time that must neither count against --frame-timeout under the name of the last frame nor
            // leave the watchdog's notices pointing at the wrong phase
            trace("noise table window: fitting", k);
            rrt_noise_table_fit_window(fit_t, seq_end > fit_t ? seq_end : fit_t, budget, &end, &cov, &bytes);
            bool ok = bytes != 0;
            for (Device& D : dev) {
                HIPCHK(hipSetDevice(D.id));
                trace("noise table window: draining and rebuilding on device", D.id);
                HIPCHK(hipDeviceSynchronize());
                if (D.noise_table) { rrt_noise_table_destroy(D.noise_table); D.noise_table = 0; }
                const int rc = ok ? rrt_noise_table_create_window(fit_t, end, cov, &D.noise_table) : RRT_OK;
                if (rc != RRT_OK) {
                    D.noise_table = 0;
                    ok = false;
                    if (!warned) {
                        fprintf(stderr, "rrt_headless: noise table [%g, %g] not built on device %d: %s (%s); hashing arithmetically\n",
                                fit_t, end, D.id, rrt_status_string(rc), rrt_last_hip_error());
                        warned = true;
                    }
                }
            }
            if (!ok) {      // all or nothing: the devices must agree on which kernels a frame runs for the timing to mean anything
                for (Device& D : dev) if (D.noise_table) { HIPCHK(hipSetDevice(D.id)); rrt_noise_table_destroy(D.noise_table); D.noise_table = 0; }
                if (bytes == 0) end = fit_t + 5.0f;          // nothing fits: look again after 5 s of sim time
            }
            t0 = fit_t; t1 = end; has_table = ok;
            trace("noise table window: done", k);
            if (ok) { ++builds; if (cov > coarsest) coarsest = cov; if (bytes > peak) peak = bytes; }
        }
        if (enabled && has_table) ++table_frames; else ++arith_frames;
        return 0;
    }
};

struct FrameView {             // one frame's times and cameras
    float sim_t = 0.0f;
    float fit_t = 0.0f;        // the earliest time the frame reads the noise at: the noise table's window is fitted from it
    rrt_camera cam;            // the start-up camera until a path moves it
    float sub_t[16];           // --motion-blur / --dof: the samples' times and cameras
    rrt_camera sub_cam[16];
    float focus = 0.0f;
};

// frame k as main() sees it while recording: the clock (main.cpp:511-516) and the camera of the active path
int view_frame(int k, const Options& o, FrameView& v) {
    int rc;
    float path_t = 0.0f;
    rrt_recording_clock(k, o.fps, &v.sim_t, &path_t);
    if (o.path >= 0 && (rc = rrt_path_camera_at(o.path, path_t, &v.cam)) != RRT_OK) return fail("camera", rc);
    // motion blur: the shutter's sub-times and the path camera at each; the noise table's window is fitted from the earliest
    v.fit_t = v.sim_t;
    if (o.motion > 1) {
        float sub_p[16];
        rrt_motion_clock(k, o.fps, o.shutter, o.motion, v.sub_t, sub_p);
        for (int m = 0; m < o.motion; ++m) {
            v.sub_cam[m] = v.cam;
            if (o.path >= 0 && (rc = rrt_path_camera_at(o.path, sub_p[m], &v.sub_cam[m])) != RRT_OK) return fail("camera", rc);
        }
        v.fit_t = v.sub_t[0];
    }
    // depth of field: without a shutter the K samples share the frame's instant; --focus hole: the camera position's distance to
    // the origin, the double root of the sum of the exact squares in x, y, z order, rounded to float (headless.py's)
    v.focus = o.dof_focus;
    if (o.use_dof) {
        if (o.motion <= 1) for (int m = 0; m < o.dof_k; ++m) { v.sub_t[m] = v.sim_t; v.sub_cam[m] = v.cam; }
        if (v.focus == 0.0f) {
            const double x = v.cam.pos[0], y = v.cam.pos[1], z = v.cam.pos[2];
            v.focus = (float)std::sqrt(x * x + y * y + z * z);
        }
    }
    return 0;
}

// frame k on device D: its tiles, or with one device the whole frame and the post passes behind it on the same stream
int launch_frame(Device& D, int slot, int k, const FrameView& v, const Options& o, const rrt_effects& fx, const Slots& R) {
    HIPCHK(hipSetDevice(D.id));
    rrt_params prm; rrt_params_default(&prm);
    prm.spin = o.spin; prm.arith_mode = o.arith;
    prm.workspace = D.pool[slot]; prm.noise_table = D.noise_table; prm.tile_order = D.order[slot];
    // frames in flight fill each other's drains: ONE chain per launch (the second chain's streams only compete with the other
    // frames: 2-7 % per frame, profiles/r05_sustained_chains.txt).  The plain single kernel would be faster still on most views,
    // but its longest wavefront (up to 19 ms on a disk-grazing view) bounds a slot's frame rate; a moving camera keeps the
    // path that is never slow
    prm.pass_chains = o.slots >= 2 ? 1 : 0;
    // ... per window, by measurement: rrt_path_chooser (csrc/rrt_path_chooser.cpp) tries the single kernel for a few frames
    // of a window, keeps it where it sustains the faster frames, and drops it at once on a frame that takes > 1.5 x the
    // three-pass median (same bytes either way)
    if (D.chooser) { int pol = RRT_PATH_AUTO; rrt_path_chooser_policy(D.chooser, k, &pol); prm.path_policy = pol; }
    else if (o.path_policy >= 0) prm.path_policy = o.path_policy;
    void* dst = o.collective ? D.tiles[slot] : R.frame[slot];
    const hipStream_t st = D.stream[slot];
    const int w = o.w, h = o.h, ss = o.supersample, rows = o.tile_rows, d = D.id, n = o.gpus;
    // the stereo / defocused / panorama / blurred / supersampled launch (_stereo, _dof, _pano, _mb, _ss): this device's tiles, or the whole frame and
    // its HDR (may be NULL)
    auto launch_sampled = [&](bool tiles, float* lin) {
        if (o.use_stereo) return tiles ? rrt_launch_raymarch_stereo_tiles(dst, o.ew, o.eh, ss, rows, d, n, &o.proj, &o.stereo, v.sim_t, &v.cam, D.sky, &fx, &prm, st)
                                       : rrt_launch_raymarch_stereo(dst, lin, o.ew, o.eh, ss, &o.proj, &o.stereo, v.sim_t, &v.cam, D.sky, &fx, &prm, st);
        if (o.use_dof) return tiles ? rrt_launch_raymarch_dof_tiles(dst, w, h, ss, rows, d, n, o.dof_k, v.sub_t, v.sub_cam, o.dof_xy, v.focus, D.sky, &fx, &prm, st)
                                    : rrt_launch_raymarch_dof(dst, lin, w, h, ss, o.dof_k, v.sub_t, v.sub_cam, o.dof_xy, v.focus, D.sky, &fx, &prm, st);
        if (o.pano) return tiles ? rrt_launch_raymarch_pano_tiles(dst, w, h, ss, rows, d, n, &o.proj, v.sim_t, &v.cam, D.sky, &fx, &prm, st)
                                 : rrt_launch_raymarch_pano(dst, lin, w, h, ss, &o.proj, v.sim_t, &v.cam, D.sky, &fx, &prm, st);
        if (o.motion > 1) return tiles ? rrt_launch_raymarch_mb_tiles(dst, w, h, ss, rows, d, n, o.motion, v.sub_t, v.sub_cam, D.sky, &fx, &prm, st)
                                       : rrt_launch_raymarch_mb(dst, lin, w, h, ss, o.motion, v.sub_t, v.sub_cam, D.sky, &fx, &prm, st);
        return tiles ? rrt_launch_raymarch_ss_tiles(dst, w, h, ss, rows, d, n, v.sim_t, &v.cam, D.sky, &fx, &prm, st)
                     : rrt_launch_raymarch_ss(dst, lin, w, h, ss, v.sim_t, &v.cam, D.sky, &fx, &prm, st);
    };
    // --adaptive: one device (check_options), the whole frame and its HDR (may be NULL); the count of refined pixels follows
    // in a 4-byte asynchronous copy, read when the frame is delivered
    auto launch_adaptive = [&](float* lin) {
        const int rc = rrt_launch_raymarch_adaptive(dst, lin, w, h, ss, o.pano ? &o.proj : nullptr, &o.adaptive, v.sim_t, &v.cam, D.sky,
                                                    &fx, &prm, R.ad_scratch[slot], R.ad_bytes, st);
        if (rc == RRT_OK && hipMemcpyAsync(R.ad_count[slot], R.ad_scratch[slot], 4, hipMemcpyDeviceToHost, st) != hipSuccess)
            return (int)RRT_ERR_HIP;
        return rc;
    };
    int rc;
    if (o.hdr_frame) {     // one device (check_options): the slot's HDR through launch_sampled, then the post passes on the same stream
        float* lin = static_cast<float*>(R.hdr[slot]);
        if (o.use_layers) {     // the 1x pinhole frame (check_exr_layers): its HDR is the debug launch's d_hdr, next to the planes the layers read
            rrt_debug_outputs dbg = {};
            dbg.d_hdr = lin;
            dbg.d_rad = static_cast<float*>(R.layer_plane[kPlaneRad][slot]);
            dbg.d_vel = static_cast<float*>(R.layer_plane[kPlaneVel][slot]);
            dbg.d_pos = static_cast<float*>(R.layer_plane[kPlanePos][slot]);
            dbg.d_steps = static_cast<int32_t*>(R.layer_plane[kPlaneSteps][slot]);
            dbg.d_hit = static_cast<int32_t*>(R.layer_plane[kPlaneHit][slot]);
            rc = rrt_launch_raymarch_ex(dst, w, h, v.sim_t, &v.cam, D.sky, &fx, &prm, &dbg, st);
        }
        else rc = o.use_adaptive ? launch_adaptive(lin) : launch_sampled(false, lin);
        if (rc == RRT_OK && o.use_exposure) {     // the bytes -- and, in front of the glow, a 10-bit Y4M conversion or an EXR file, the scaled HDR in place
            if (o.auto_exposure) HIPCHK(hipStreamWaitEvent(st, R.exposed, 0));
            rc = rrt_launch_exposure(o.use_glow ? nullptr : dst, o.use_glow || o.y4m10 || o.use_exr || o.png16 ? lin : nullptr, lin, w, h, &o.exposure, R.exposure_scratch,
                                     R.exposure_bytes, st);
            if (o.auto_exposure) HIPCHK(hipEventRecord(R.exposed, st));
        }
        if (rc == RRT_OK && o.use_glow) rc = rrt_launch_glow(dst, lin, w, h, &o.glow, R.glow_scratch[slot], o.glow_bytes, st);
    }
    else if (o.use_adaptive) rc = launch_adaptive(nullptr);
    else if (o.use_stereo || o.use_dof || o.pano || o.motion > 1 || ss > 1) rc = launch_sampled(o.collective, nullptr);
    else if (o.collective) rc = rrt_launch_raymarch_tiles(dst, w, h, rows, d, n, v.sim_t, &v.cam, D.sky, &fx, &prm, st);
    else rc = rrt_launch_raymarch(dst, w, h, v.sim_t, &v.cam, D.sky, &fx, &prm, st);
    if (rc != RRT_OK) return fail("launch", rc);
    if (D.chooser) HIPCHK(hipEventRecord(D.render_end[k % (2 * o.slots)], st));
    return 0;
}

// one gather: every device sends its shard, device 0 receives all of them (its own included) and scatters them into the frame
int gather_frame(std::vector<Device>& dev, int slot, int k, const Options& o, const Slots& R) {
    // Successive frames use the SAME communicators from DIFFERENT streams (slot k mod slots).  RCCL orders the
    // operations of one communicator by itself; the event chain states that order in the stream graph as well:
    // a device's part of exchange k starts after its part of exchange k-1 has finished, whatever streams they ran on.
    if (k > 1) for (Device& D : dev) { HIPCHK(hipSetDevice(D.id)); HIPCHK(hipStreamWaitEvent(D.stream[slot], D.comm_free, 0)); }
    NCCLCHK(ncclGroupStart());
    for (Device& D : dev) {
        const size_t bytes = (size_t)D.shard_rows * o.w * 4;
        if (bytes == 0) continue;
        NCCLCHK(ncclSend(D.tiles[slot], bytes, ncclUint8, 0, D.comm, D.stream[slot]));
        NCCLCHK(ncclRecv(static_cast<uint8_t*>(R.gathered[slot]) + (size_t)D.id * R.shard_stride, bytes, ncclUint8, D.id, dev[0].comm,
                         dev[0].stream[slot]));
    }
    NCCLCHK(ncclGroupEnd());
    for (Device& D : dev) { HIPCHK(hipSetDevice(D.id)); HIPCHK(hipEventRecord(D.comm_free, D.stream[slot])); }
    // device 0 scatters the shards into the bottom-up frame
    HIPCHK(hipSetDevice(0));
    const int rc = rrt_assemble_all_tiles(R.frame[slot], R.gathered[slot], R.shard_stride, o.w, o.h, o.tile_rows, o.gpus, dev[0].stream[slot]);
    return rc == RRT_OK ? 0 : fail("assemble", rc);
}

// ---- the summary line

__attribute__((format(printf, 2, 3))) void appendf(std::string& s, const char* fmt, ...) {
    va_list ap, again;
    va_start(ap, fmt);
    va_copy(again, ap);
    const int n = vsnprintf(nullptr, 0, fmt, ap);
    va_end(ap);
    if (n > 0) {
        const size_t at = s.size();
        s.resize(at + (size_t)n + 1);
        vsnprintf(&s[at], (size_t)n + 1, fmt, again);
        s.resize(at + (size_t)n);
    }
    va_end(again);
}

struct Totals {                // what the frame loop measured
    double seconds = 0.0;
    unsigned long long refined = 0;   // --adaptive: refined pixels over all frames
    float final_ev = 0.0f;            // --exposure / --auto-exposure: the EV after the last frame
};

std::string summary_line(const Options& o, const std::vector<Device>& dev, const NoiseWindow& nw, const char* path_name, const Totals& t) {
    const double dt = t.seconds;
    std::string s;
    appendf(s, "{\"frames\": %d, \"width\": %d, \"height\": %d, \"n_gpus\": %d, \"seconds\": %.4f, \"fps\": %.3f, \"Mrays_per_s\": %.3f, ",
            o.frames, o.w, o.h, o.gpus, dt, o.frames / dt, (double)o.frames * o.w * o.h / dt / 1e6);
    appendf(s, "\"path\": \"%s\", \"spin\": %g, \"arith_mode\": \"%s\", \"noise_tables\": {\"builds\": %d, \"table_frames\": %d, "
            "\"arith_frames\": %d, \"coarsest_coverage\": %d, \"peak_bytes\": %zu, \"budget_bytes\": %zu}, \"tile_order\": %s, \"collective\": \"%s\", ",
            path_name, o.spin, o.arith == RRT_ARITH_FAST ? "fast" : (o.arith == RRT_ARITH_FMAD ? "fmad" : "strict"),
            nw.builds, nw.table_frames, nw.arith_frames, nw.coarsest, nw.peak, nw.budget, dev[0].order[0] ? "true" : "false",
            o.collective ? "rccl grouped send/recv gather" : "none");
    s += "\"path_choice\": ";
    if (dev[0].chooser) {
        for (const Device& D : dev) {
            rrt_path_chooser_stats st;
            rrt_path_chooser_get_stats(D.chooser, &st);
            appendf(s, "%s{\"device\": %d, \"frames_three_pass\": %d, \"frames_single_kernel\": %d, \"windows\": %d, \"trials\": %d, "
                    "\"trials_aborted\": %d, \"switches\": %d, \"outliers\": %d}", D.id ? ", " : "[", D.id, st.frames[0], st.frames[1], st.windows, st.trials,
                    st.trials_aborted, st.switches, st.outliers);
        }
        s += "]";
    } else s += "null";
    appendf(s, ", \"supersample\": %d, \"motion_blur\": %d, \"shutter\": %g, \"glow\": ", o.supersample, o.motion, o.shutter);
    if (o.use_glow) appendf(s, "{\"radius\": %g, \"lobes\": %d, \"threshold\": %g, \"intensity\": %g}", o.glow.radius, o.glow.lobes,
                            o.glow.threshold, o.glow.intensity);
    else s += "null";
    appendf(s, ", \"projection\": \"%s\", \"fov_deg\": ",
            o.projection == RRT_PROJ_EQUIRECT ? "equirect" : (o.projection == RRT_PROJ_FISHEYE ? "fisheye" : "pinhole"));
    if (o.pano) appendf(s, "%g", o.proj.fov_deg); else s += "null";
    s += ", \"vfov_deg\": ";
    if (o.projection == RRT_PROJ_EQUIRECT) appendf(s, "%g", o.proj.vfov_deg); else s += "null";
    s += ", \"stereo\": ";
    if (o.use_stereo) appendf(s, "{\"layout\": \"%s\", \"base\": %.17g, \"convergence\": %.17g, \"pole_merge_deg\": [%.17g, %.17g]}",
                              o.stereo_layout == RRT_STEREO_TOP_BOTTOM ? "top-bottom" : "side-by-side", o.stereo.base, o.stereo.convergence,
                              o.stereo.pole_merge_from_deg, o.stereo.pole_merge_to_deg);
    else s += "null";
    s += ", \"dof\": ";
    if (o.use_dof) {
        appendf(s, "{\"aperture\": %.9g, \"focus\": ", o.dof_aperture);
        if (o.dof_focus == 0.0f) s += "\"hole\""; else appendf(s, "%.9g", o.dof_focus);
        appendf(s, ", \"samples\": %d}", o.dof_k);
    } else s += "null";
    s += ", \"adaptive\": ";
    if (o.use_adaptive) appendf(s, "{\"threshold\": %d, \"refined_fraction\": %.9g}", o.adaptive.threshold,
                                o.frames > 0 ? (double)t.refined / ((double)o.frames * o.w * o.h) : 0.0);
    else s += "null";
    s += ", \"exposure\": ";
    if (o.use_exposure) {
        const rrt_exposure& e = o.exposure;
        appendf(s, "{\"mode\": \"%s\", \"ev\": %.9g, \"key\": %.9g, \"low_permille\": %d, \"high_permille\": %d, \"min_ev\": %.9g, "
                "\"max_ev\": %.9g, \"adapt_up\": %.9g, \"adapt_down\": %.9g, \"final_ev\": %.9g}", o.auto_exposure ? "auto" : "manual", e.ev,
                e.key, e.low_permille, e.high_permille, e.min_ev, e.max_ev, e.adapt_up, e.adapt_down, t.final_ev);
    } else s += "null";
    /* which path the frames took through each device's march cache (launches without a workspace: one GPU, or --workspace-gib 0) */
    s += ", \"march_cache\": ";
    for (const Device& D : dev) {
        rrt_march_cache_info mc = {};
        (void)rrt_march_cache_stats(D.id, &mc);
        appendf(s, "%s{\"device\": %d, \"fills\": %llu, \"hits\": %llu, \"drops\": %llu, \"misses\": %llu, \"uncacheable\": %llu, "
                "\"bytes\": %llu, \"max_bytes\": %llu}", D.id ? ", " : "[", D.id, (unsigned long long)mc.fills, (unsigned long long)mc.hits,
                (unsigned long long)mc.drops, (unsigned long long)mc.misses, (unsigned long long)mc.uncacheable, (unsigned long long)mc.bytes,
                (unsigned long long)mc.max_bytes);
    }
    s += "]}\n";
    return s;
}

}  // namespace

int main(int argc, char** argv) {
    Options o;
    int rc;
    if ((rc = parse_options(argc, argv, o)) != 0 || (rc = check_options(o)) != 0) return rc;
    int n_dev = 0;
    if ((rc = rrt_device_count(&n_dev)) != RRT_OK) return fail("no GPU", rc);
    if (o.gpus > n_dev) { fprintf(stderr, "rrt_headless: --gpus %d but %d device(s) visible\n", o.gpus, n_dev); return 2; }
    trace("start");
    std::thread dog(watchdog, o.init_timeout, o.frame_timeout);
    struct DogStop { std::thread& t; ~DogStop() { g_tr.stop.store(true); t.join(); } } dog_stop{dog};      // every return path
    // the RCCL library's pages, read sequentially in the background while the per-device resources are set up
    std::thread warm;
    if (o.collective && !getenv("RRT_NO_LIBRARY_WARMUP")) warm = std::thread(warm_library_pages, (const void*)&ncclCommInitAll);
    struct WarmJoin { std::thread& t; ~WarmJoin() { if (t.joinable()) t.join(); } } warm_join{warm};
    // a failing communicator says why (RCCL prints nothing below WARN); the caller's setting wins
    if (o.collective) setenv("NCCL_DEBUG", "WARN", 0);
    // one process, one node: RCCL's bootstrap and RAS sockets need no interface but the loopback (by default it picks
    // the first non-loopback one -- in a container a veth whose state is not this program's business)
    if (o.collective) setenv("NCCL_SOCKET_IFNAME", "lo", 0);

    // the recording clock (main.cpp:511-516) says which times the sequence reaches; the tables slide along it
    float seq_end = 0.0f;
    { float unused = 0.0f; rrt_recording_clock(o.frames, o.fps, &seq_end, &unused); seq_end += 1.0f; }
    const size_t table_budget = o.table_gib > 0.0 ? (size_t)(o.table_gib * (double)(1ull << 30)) : 0;
    NoiseWindow noise{o.use_table && table_budget != 0, table_budget, seq_end};

    std::vector<uint8_t> sky;
    int sky_w = 2048, sky_h = 1024;
    if (o.sky_path.empty()) sky = synthetic_sky(sky_w, sky_h, o.sky_seed);
    else if (!load_sky_raw(o.sky_path, sky, sky_w, sky_h)) return 2;
    rrt_effects fx; rrt_effects_default(&fx);
    fx.use_chromatic_aberration = (uint8_t)o.all_fx;

    // ---- bring-up: per-device resources, the communicators, device 0's slots, the sink
    std::vector<Device> dev(o.gpus);
    Slots R;
    plan_shards(o, dev, R);
    for (Device& D : dev) if (create_device(D, o, sky, sky_w, sky_h, R.shard_stride)) return 1;
    trace("per-device resources ready");
    if (o.collective && create_communicators(dev, warm)) return 1;
    FILE* f = o.out_path.empty() ? nullptr : fopen(o.out_path.c_str(), "wb");
    if (!o.out_path.empty() && !f) { perror("fopen"); return 1; }
    if (create_slots(R, o, f != nullptr, dev[0].stream[0])) return 1;
    FILE* fy = nullptr;
    if (o.y4m) {
        char header[160];
        size_t n = 0;
        if ((rc = rrt_y4m_header(&o.yuv, o.w, o.h, o.fps, 1, header, sizeof(header), &n)) != RRT_OK) return fail("y4m header", rc);
        if (!(fy = fopen(o.y4m_path.c_str(), "wb"))) { perror("fopen"); return 1; }
        if (fwrite(header, 1, n, fy) != n) { perror("fwrite"); return 1; }
        trace(o.y4m10 ? "y4m sink ready: planes from the HDR frame" : "y4m sink ready: planes from the RGBA8 frame");
    }
    FrameView view;
    const float start_pos[3] = {0.0f, 10.0f, -60.0f};
    rrt_camera_from_angles(start_pos, 0.0f, -10.0f, &view.cam);
    const char* path_name = "";
    if (o.path >= 0 && (rc = rrt_path_info(o.path, &path_name, nullptr, nullptr)) != RRT_OK) return fail("path", rc);

    // write frame `k`'s pixels once its copy has landed (called one frame late, so that the copy overlaps the next render)
    // (without a sink the wait still happens: the host never runs more than `slots` frames ahead of the device, a device
    // fault is reported at the frame it belongs to, and the watchdog sees frames complete)
    Totals totals;
    int delivered = 0;
    const int exr_threads = deflate_threads();
    auto deliver = [&](int slot) -> int {
        HIPCHK(hipEventSynchronize(R.done[slot]));
        trace("frame complete", ++delivered);
        if (o.use_adaptive) totals.refined += *static_cast<const uint32_t*>(R.ad_count[slot]);
        // frame `delivered` has been rendered on every device (the gather waited for all shards): its sustained time on a device =
        // the interval between the ends of frame delivered - 1's and its own render there
        if (delivered >= 2) for (Device& D : dev) if (D.chooser) {
            float ms = 0.0f;
            HIPCHK(hipSetDevice(D.id));
            if (hipEventElapsedTime(&ms, D.render_end[(delivered - 1) % (2 * o.slots)], D.render_end[delivered % (2 * o.slots)]) == hipSuccess)
                rrt_path_chooser_report(D.chooser, delivered, ms > 0.0f ? ms : 0.0f);   // (a frame that ended before its predecessor: 0)
        }
        if (f && fwrite(R.host[slot], 1, R.frame_bytes, f) != R.frame_bytes) fprintf(stderr, "Warning: Frame write incomplete\n");
        if (fy && (fwrite("FRAME\n", 1, 6, fy) != 6 || fwrite(R.yuv_host[slot], 1, o.yuv_bytes, fy) != o.yuv_bytes))
            fprintf(stderr, "Warning: Frame write incomplete\n");
        if (o.use_exr && write_exr_file(frame_name(o.exr_path, delivered), static_cast<const uint8_t*>(R.exr_host[slot]), o, exr_threads)) return 1;
        if (o.use_png && o.png_deflate == 1) {      // the sizes and the row sums are here; the streams' bytes, and no more, follow now
            const uint8_t* meta = static_cast<const uint8_t*>(R.png_host[slot]);
            const uint32_t* sizes = reinterpret_cast<const uint32_t*>(meta);
            size_t total = 0;
            for (int i = 0; i < o.png_slices; ++i) total += sizes[i];
            if (total > o.dfl_bound) { fprintf(stderr, "rrt_headless: png: the streams' sizes exceed their bound\n"); return 1; }
            uint8_t* streams = static_cast<uint8_t*>(R.png_host[slot]) + png_meta_bytes(o);
            HIPCHK(hipSetDevice(0));
            HIPCHK(hipMemcpyAsync(streams, R.dfl_out[slot], total, hipMemcpyDeviceToHost, dev[0].stream[slot]));
            HIPCHK(hipStreamSynchronize(dev[0].stream[slot]));
            if (write_png_streams(frame_name(o.png_path, delivered), streams, sizes, reinterpret_cast<const uint32_t*>(meta + png_meta_offset(o)), o)) return 1;
        } else if (o.use_png) {
            const uint8_t* png = static_cast<const uint8_t*>(R.png_host[slot]);
            if (write_png_file(frame_name(o.png_path, delivered), png, reinterpret_cast<const uint32_t*>(png + png_table_offset(o)), o, exr_threads)) return 1;
        }
        return 0;
    };

    for (Device& D : dev) { HIPCHK(hipSetDevice(D.id)); HIPCHK(hipDeviceSynchronize()); }
    trace("bring-up complete; rendering");
    g_tr.in_frames.store(true);
    auto t0 = std::chrono::steady_clock::now();
    for (int k = 1; k <= o.frames; ++k) {
        const int slot = k % o.slots;
        if (view_frame(k, o, view)) return 1;
        trace("frame", k);
        // slot reuse: frame k-slots used the same buffers; its host copy must have been written out
        if (k > o.slots && deliver(slot)) return 1;
        if (noise.slide(view.fit_t, k, dev)) return 1;
        for (Device& D : dev) if (launch_frame(D, slot, k, view, o, fx, R)) return 1;
        if (o.collective && gather_frame(dev, slot, k, o, R)) return 1;
        // hand the frame to the sink: asynchronous copy now, the write happens one frame later
        HIPCHK(hipSetDevice(0));
        if (f) HIPCHK(hipMemcpyAsync(R.host[slot], R.frame[slot], R.frame_bytes, hipMemcpyDeviceToHost, dev[0].stream[slot]));
        if (fy) {       // the planes of the assembled frame (depth 10: of its HDR as the last pass left it), then their copy
            if (o.y4m_pq) {     // metered into the film's one state, in frame order
                if (k > 1) HIPCHK(hipStreamWaitEvent(dev[0].stream[slot], R.lit, 0));
                rc = rrt_launch_yuv_hdr10_from_hdr(R.yuv[slot], static_cast<const float*>(R.hdr[slot]), o.w, o.h, &o.yuv, &o.hdr10, R.light,
                                                   dev[0].stream[slot]);
                if (rc == RRT_OK) HIPCHK(hipEventRecord(R.lit, dev[0].stream[slot]));
            } else
            rc = o.y4m10 ? rrt_launch_yuv_from_hdr(R.yuv[slot], static_cast<const float*>(R.hdr[slot]), o.w, o.h, &o.yuv, dev[0].stream[slot])
                         : rrt_launch_yuv_from_rgba8(R.yuv[slot], R.frame[slot], o.w, o.h, &o.yuv, dev[0].stream[slot]);
            if (rc != RRT_OK) { fprintf(stderr, "rrt_headless: y4m: %s (%s)\n", rrt_status_string(rc), rrt_yuv_last_error()); return 1; }
            HIPCHK(hipMemcpyAsync(R.yuv_host[slot], R.yuv[slot], o.yuv_bytes, hipMemcpyDeviceToHost, dev[0].stream[slot]));
        }
        if (o.use_exr) {    // the chunks of the frame's HDR as the last pass left it, then their copy; the file is made when the frame is delivered
            if (o.use_layers) {     // ... next to the data layers, from the slot's planes
                rrt_exr_layers layers = o.layers;
                layers.sources[0].d_data = R.hdr[slot];
                for (int p = 0; p < kLayerPlaneCount; ++p)
                    if (o.layer_planes & (1 << p)) layers.sources[o.layer_source[p]].d_data = R.layer_plane[p][slot];
                rc = rrt_launch_exr_layers(R.exr[slot], &layers, o.w, o.h, dev[0].stream[slot]);
            }
            else rc = rrt_launch_exr_from_hdr(R.exr[slot], static_cast<const float*>(R.hdr[slot]), o.w, o.h, &o.exr, dev[0].stream[slot]);
            if (rc != RRT_OK) { fprintf(stderr, "rrt_headless: exr: %s (%s)\n", rrt_status_string(rc), rrt_exr_last_error()); return 1; }
            HIPCHK(hipMemcpyAsync(R.exr_host[slot], R.exr[slot], o.exr_bytes, hipMemcpyDeviceToHost, dev[0].stream[slot]));
        }
        if (o.use_png) {    // the filtered scanlines and row sums of the assembled frame (depth 16: of its HDR as the last pass left it), then their copy
            uint8_t* png = static_cast<uint8_t*>(R.png[slot]);
            uint32_t* sums = o.png_deflate == 1 ? reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(R.png_meta[slot]) + png_meta_offset(o))
                                                : reinterpret_cast<uint32_t*>(png + png_table_offset(o));
            rc = o.png16 ? rrt_launch_png_from_hdr(png, sums, static_cast<const float*>(R.hdr[slot]), o.w, o.h, &o.png, dev[0].stream[slot])
                         : rrt_launch_png_from_rgba8(png, sums, R.frame[slot], o.w, o.h, &o.png, dev[0].stream[slot]);
            if (rc != RRT_OK) { fprintf(stderr, "rrt_headless: png: %s (%s)\n", rrt_status_string(rc), rrt_png_last_error()); return 1; }
            if (o.png_deflate == 1) {   // deflate behind the filtering, on the same stream; the payload is not copied
                rc = rrt_launch_deflate(R.dfl_out[slot], static_cast<uint32_t*>(R.png_meta[slot]), R.dfl_scratch[slot], png, o.png_bytes,
                                        (size_t)o.png_slice_rows * o.png_stride, 1, dev[0].stream[slot]);
                if (rc != RRT_OK) { fprintf(stderr, "rrt_headless: png deflate: %s (%s)\n", rrt_status_string(rc), rrt_deflate_last_error()); return 1; }
                HIPCHK(hipMemcpyAsync(R.png_host[slot], R.png_meta[slot], png_meta_bytes(o), hipMemcpyDeviceToHost, dev[0].stream[slot]));
            } else
            HIPCHK(hipMemcpyAsync(R.png_host[slot], R.png[slot], png_table_offset(o) + o.png_sum_bytes, hipMemcpyDeviceToHost, dev[0].stream[slot]));
        }
        HIPCHK(hipEventRecord(R.done[slot], dev[0].stream[slot]));
    }
    trace("all frames enqueued; draining");
    // drain: the last min(frames, slots) frames, oldest first
    for (int k = o.frames - o.slots + 1; k <= o.frames; ++k)
        if (k >= 1 && deliver(k % o.slots)) return 1;
    for (Device& D : dev) { HIPCHK(hipSetDevice(D.id)); HIPCHK(hipDeviceSynchronize()); }
    totals.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (f) fclose(f);
    if (fy) fclose(fy);
    if (o.y4m_pq) {     // the film's light levels: one copy of the state, after the last frame, and the sidecar next to the file
        alignas(16) unsigned char state[32];
        uint32_t levels[3];
        char text[1024];
        size_t n = 0;
        HIPCHK(hipMemcpy(state, R.light, sizeof(state), hipMemcpyDeviceToHost));
        if ((rc = rrt_yuv_hdr10_light_levels(state, o.w, o.h, levels)) != RRT_OK) return fail("hdr10 light levels", rc);
        if ((rc = rrt_y4m_hdr10_sidecar(&o.hdr10, levels, text, sizeof(text), &n)) != RRT_OK) return fail("hdr10 sidecar", rc);
        FILE* fs = fopen((o.y4m_path + ".hdr10.json").c_str(), "wb");
        if (!fs) { perror("fopen"); return 1; }
        if (fwrite(text, 1, n, fs) != n) { perror("fwrite"); return 1; }
        fclose(fs);
    }
    totals.final_ev = o.exposure.ev;        // the final EV: one 4-byte read of the state, after the last frame
    if (o.auto_exposure) HIPCHK(hipMemcpy(&totals.final_ev, static_cast<const uint8_t*>(R.exposure_scratch) + RRT_EXPOSURE_STATE_OFFSET, 4, hipMemcpyDeviceToHost));
    fputs(summary_line(o, dev, noise, path_name, totals).c_str(), stdout);

    for (Device& D : dev) { HIPCHK(hipSetDevice(D.id)); destroy_device(D, o.slots); }
    HIPCHK(hipSetDevice(0));
    destroy_slots(R, o.slots);
    return 0;
}
