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
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rrt.h"

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

}  // namespace

int main(int argc, char** argv) {
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
    rrt_glow_default(&glow);
    bool use_glow = false;
    rrt_exposure exposure;         // --exposure EV / --auto-exposure [KEY] (+ --exposure-speed / -range / -percentiles): rrt_launch_exposure
    rrt_exposure_default(&exposure);
    bool use_exposure = false, exposure_opts = false;
    double exposure_tau[2] = {0.0, 0.0};     // --exposure-speed UP DOWN, seconds
    int projection = RRT_PROJ_PINHOLE;   // --projection: the camera (rrt_launch_raymarch_pano* for equirect / fisheye)
    float fov = 0.0f, vfov = 0.0f;       // --fov / --vfov DEG (0: not given -- the kind's default, rrt_projection_default)
    int stereo_layout = 0;               // --stereo: RRT_STEREO_* (0: mono); rrt_launch_raymarch_stereo*
    bool stereo_base = false, stereo_conv = false, stereo_merge = false;   // which of the stereo options were given
    rrt_stereo stereo;                   // --stereo-base / --convergence / --pole-merge over rrt_stereo_default
    rrt_stereo_default(RRT_STEREO_TOP_BOTTOM, &stereo);
    bool use_adaptive = false;           // --adaptive [T]: rrt_launch_raymarch_adaptive
    rrt_adaptive adaptive;
    rrt_adaptive_default(&adaptive);
    bool use_dof = false;                // --dof APERTURE: rrt_launch_raymarch_dof*
    float dof_aperture = 0.0f, dof_focus = 0.0f;     // --focus Z (0: hole -- the frame's camera's distance to the origin)
    int dof_samples = 0;                 // --dof-samples K (0: not given -- 8, or --motion-blur's M)
    bool dof_focus_given = false;
    int kSlots = 3;                // frames in flight: frame k renders on stream k mod kSlots while its predecessors are
                                   // gathered / assembled / copied out (a rank's share of a frame is only a few rounds of
                                   // wavefronts; 3 measured best at 8 shards of a 4K frame: profiles/r02_frames_in_flight.txt)
    float spin = 0.0f;
    double table_gib = 2.0;
    double init_timeout = 300.0, frame_timeout = 120.0;       // watchdog limits in seconds (0: none)
    std::string out_path, sky_path;
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        auto val = [&](int& dst) { if (i + 1 < argc) dst = atoi(argv[++i]); };
        if (a == "--width") val(w); else if (a == "--height") val(h); else if (a == "--frames") val(frames);
        else if (a == "--fps") val(fps); else if (a == "--path") val(path); else if (a == "--sky-seed") val(sky_seed);
        else if (a == "--gpus") val(gpus); else if (a == "--tile-rows") val(tile_rows); else if (a == "--workspace-gib") val(workspace_gib);
        else if (a == "--frames-in-flight") val(kSlots);
        else if (a == "--spin" && i + 1 < argc) spin = (float)atof(argv[++i]);
        else if (a == "--noise-table-gib" && i + 1 < argc) table_gib = atof(argv[++i]);
        else if (a == "--init-timeout" && i + 1 < argc) init_timeout = atof(argv[++i]);
        else if (a == "--frame-timeout" && i + 1 < argc) frame_timeout = atof(argv[++i]);
        else if (a == "--no-noise-table") use_table = 0;
        else if (a == "--tile-order") tile_order = 1; else if (a == "--no-tile-order") tile_order = 0;
        else if (a == "--force-collective") force_collective = 1;     // run the RCCL exchange even with one GPU (self-check)
        else if (a == "--out" && i + 1 < argc) out_path = argv[++i];
        else if (a == "--sky" && i + 1 < argc) sky_path = argv[++i];
        else if (a == "--all-effects") all_fx = 1; else if (a == "--fast") arith = RRT_ARITH_FAST;
        else if (a == "--path-window") val(path_window);
        else if (a == "--path-policy" && i + 1 < argc) {
            const std::string m = argv[++i];
            if (m == "auto") path_policy = RRT_PATH_AUTO; else if (m == "single") path_policy = RRT_PATH_SINGLE; else if (m == "three-pass") path_policy = RRT_PATH_THREE_PASS;
            else { fprintf(stderr, "--path-policy auto | single | three-pass\n"); return 2; }
            path_window = -1;
        }
        else if (a == "--supersample") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m == "1" || m == "2" || m == "4" || m == "8") supersample = atoi(m.c_str());
            else { fprintf(stderr, "--supersample 1 | 2 | 4 | 8 (sub-samples per pixel along each axis)\n"); return 2; }
        }
        else if (a == "--motion-blur") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m == "1" || m == "2" || m == "4" || m == "8" || m == "16") motion = atoi(m.c_str());
            else { fprintf(stderr, "--motion-blur 1 | 2 | 4 | 8 | 16 (sub-frames per frame)\n"); return 2; }
        }
        else if (a == "--shutter") {
            const char* m = i + 1 < argc ? argv[++i] : "";
            char* end = nullptr;
            const float f = strtof(m, &end);
            if (end != m && *end == 0 && f >= 0.0f && f <= 1.0f) shutter = f;
            else { fprintf(stderr, "--shutter F: a fraction of the frame interval in [0, 1]\n"); return 2; }
        }
        else if (a == "--glow" || a == "--glow-radius" || a == "--glow-threshold" || a == "--glow-lobes") {
            const char* m = i + 1 < argc ? argv[++i] : "";
            char* end = nullptr;
            const float v = strtof(m, &end);
            if (end == m || *end != 0 || !std::isfinite(v)) { fprintf(stderr, "%s: a number\n", a.c_str()); return 2; }
            if (a == "--glow") { glow.intensity = v; use_glow = true; }
            else if (a == "--glow-radius") glow.radius = v;
            else if (a == "--glow-threshold") glow.threshold = v;
            else if (v == (float)(int)v) glow.lobes = (int)v;
            else { fprintf(stderr, "--glow-lobes 1 | 2 | 3 | 4\n"); return 2; }
        }
        else if (a == "--exposure" || a == "--exposure-speed" || a == "--exposure-range" || a == "--exposure-percentiles") {
            double v[2] = {0.0, 0.0};
            const int n = a == "--exposure" ? 1 : 2;
            for (int j = 0; j < n; ++j) {
                const char* m = i + 1 < argc ? argv[++i] : "";
                char* end = nullptr;
                v[j] = strtod(m, &end);
                if (end == m || *end != 0 || !std::isfinite(v[j])) { fprintf(stderr, "usage: %s: %s\n", a.c_str(), n == 1 ? "a number" : "two numbers"); return 2; }
            }
            if (a == "--exposure") { exposure.ev = (float)v[0]; use_exposure = true; }
            else {
                exposure_opts = true;
                if (a == "--exposure-speed") { exposure_tau[0] = v[0]; exposure_tau[1] = v[1]; }
                else if (a == "--exposure-range") { exposure.min_ev = (float)v[0]; exposure.max_ev = (float)v[1]; }
                else if (v[0] == (double)(int)v[0] && v[1] == (double)(int)v[1]) { exposure.low_permille = (int)v[0]; exposure.high_permille = (int)v[1]; }
                else { fprintf(stderr, "usage: --exposure-percentiles LOW HIGH: whole numbers in per mille\n"); return 2; }
            }
        }
        else if (a == "--auto-exposure") {  // the key is optional: the next argument unless it is another option
            use_exposure = true;
            exposure.mode = RRT_EXPOSURE_AUTO;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) {
                const char* m = argv[++i];
                char* end = nullptr;
                exposure.key = strtof(m, &end);
                if (end == m || *end != 0) { fprintf(stderr, "usage: --auto-exposure [KEY]: a luminance > 0 (default 0.5)\n"); return 2; }
            }
        }
        else if (a == "--projection") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m == "pinhole") projection = RRT_PROJ_PINHOLE; else if (m == "equirect") projection = RRT_PROJ_EQUIRECT;
            else if (m == "fisheye") projection = RRT_PROJ_FISHEYE;
            else { fprintf(stderr, "--projection pinhole | equirect | fisheye\n"); return 2; }
        }
        else if (a == "--fov" || a == "--vfov") {
            const char* m = i + 1 < argc ? argv[++i] : "";
            char* end = nullptr;
            const float v = strtof(m, &end);
            if (end == m || *end != 0) { fprintf(stderr, "%s DEG: a number of degrees\n", a.c_str()); return 2; }
            (a == "--fov" ? fov : vfov) = v;
            if (v == 0.0f) { fprintf(stderr, "--fov DEG in (0, 360], --vfov DEG in (0, 180]\n"); return 2; }
        }
        else if (a == "--stereo") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m == "top-bottom") stereo_layout = RRT_STEREO_TOP_BOTTOM; else if (m == "side-by-side") stereo_layout = RRT_STEREO_SIDE_BY_SIDE;
            else { fprintf(stderr, "usage: --stereo top-bottom | side-by-side\n"); return 2; }
        }
        else if (a == "--stereo-base" || a == "--convergence" || a == "--pole-merge") {
            float v[2];
            const int n = a == "--pole-merge" ? 2 : 1;
            for (int j = 0; j < n; ++j) {
                const char* m = i + 1 < argc ? argv[++i] : "";
                char* end = nullptr;
                v[j] = strtof(m, &end);
                if (end == m || *end != 0) { fprintf(stderr, "usage: %s: a number\n", a.c_str()); return 2; }
            }
            if (a == "--stereo-base") { stereo.base = v[0]; stereo_base = true; }
            else if (a == "--convergence") { stereo.convergence = v[0]; stereo_conv = true; }
            else { stereo.pole_merge_from_deg = v[0]; stereo.pole_merge_to_deg = v[1]; stereo_merge = true; }
        }
        else if (a == "--adaptive") {       // the threshold is optional: the next argument unless it is another option
            use_adaptive = true;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) {
                const char* m = argv[++i];
                char* end = nullptr;
                const long v = strtol(m, &end, 10);
                if (end == m || *end != 0 || v < 0 || v > 255) { fprintf(stderr, "usage: --adaptive [T]: a threshold in 0 ... 255 (default 8)\n"); return 2; }
                adaptive.threshold = (int32_t)v;
            }
        }
        else if (a == "--dof") {
            const char* m = i + 1 < argc ? argv[++i] : "";
            char* end = nullptr;
            const float v = strtof(m, &end);
            if (end == m || *end != 0 || !std::isfinite(v) || v < 0.0f) { fprintf(stderr, "usage: --dof APERTURE: the lens radius in scene units, >= 0\n"); return 2; }
            dof_aperture = v; use_dof = true;
        }
        else if (a == "--focus") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            char* end = nullptr;
            const float v = m == "hole" ? 0.0f : strtof(m.c_str(), &end);
            if (m != "hole" && (end == m.c_str() || *end != 0 || !std::isfinite(v) || !(v > 0.0f))) {
                fprintf(stderr, "usage: --focus: a distance > 0 along forward, or `hole`\n"); return 2;
            }
            dof_focus = v; dof_focus_given = true;
        }
        else if (a == "--dof-samples") {
            const std::string m = i + 1 < argc ? argv[++i] : "";
            if (m == "1" || m == "2" || m == "4" || m == "8" || m == "16") dof_samples = atoi(m.c_str());
            else { fprintf(stderr, "usage: --dof-samples 1 | 2 | 4 | 8 | 16 (lens samples per sub-sample)\n"); return 2; }
        }
        else if (a == "--arith" && i + 1 < argc) {
            const std::string m = argv[++i];
            if (m == "strict") arith = RRT_ARITH_STRICT; else if (m == "fmad") arith = RRT_ARITH_FMAD; else if (m == "fast") arith = RRT_ARITH_FAST;
            else { fprintf(stderr, "--arith strict | fmad | fast\n"); return 2; }
        }
        else { fprintf(stderr, "unknown argument %s\n", a.c_str()); return 2; }
    }
    if (w <= 0 || h <= 0 || frames < 0 || fps <= 0 || gpus < 1 || tile_rows < 1 || kSlots < 1 || kSlots > kMaxSlots) {
        fprintf(stderr, "bad arguments\n"); return 2;
    }
    // the glow needs the whole frame's HDR on one device (rrt_launch_glow has no _tiles form); its settings are checked up front
    size_t glow_bytes = 0;
    if (use_glow) {
        if (gpus > 1 || force_collective) { fprintf(stderr, "rrt_headless: --glow renders on one GPU only (--gpus 1)\n"); return 2; }
        if (rrt_glow_scratch_bytes(w, h, &glow, &glow_bytes) != RRT_OK) {
            fprintf(stderr, "--glow INTENSITY >= 0, --glow-radius R > 0 (a fraction of the height; widest lobe <= 1024 px), "
                            "--glow-threshold T >= 0, --glow-lobes 1 | 2 | 3 | 4\n");
            return 2;
        }
    }
    // exposure control needs the whole frame's HDR on one device (the meter sees every pixel; rrt_launch_exposure has no _tiles form)
    if (!use_exposure && exposure_opts) {
        fprintf(stderr, "usage: --exposure-speed / --exposure-range / --exposure-percentiles need --exposure EV | --auto-exposure [KEY]\n"); return 2;
    }
    if (use_exposure) {
        if (gpus > 1 || force_collective) { fprintf(stderr, "usage: --exposure / --auto-exposure: one GPU only (--gpus 1)\n"); return 2; }
        // the settings' ranges are rrt_launch_exposure's own refusals, stated here before any device is touched
        const bool speeds = rrt_exposure_adapt(1.0 / (double)fps, exposure_tau[0], &exposure.adapt_up) == RRT_OK &&
                            rrt_exposure_adapt(1.0 / (double)fps, exposure_tau[1], &exposure.adapt_down) == RRT_OK &&
                            exposure.adapt_up > 0.0f && exposure.adapt_down > 0.0f;
        if (!speeds || !std::isfinite(exposure.key) || !(exposure.key > 0.0f) || !(exposure.min_ev <= exposure.max_ev) ||
            exposure.low_permille < 0 || exposure.high_permille < 0 || (long long)exposure.low_permille + exposure.high_permille >= 1000) {
            fprintf(stderr, "usage: --auto-exposure KEY > 0, --exposure-speed UP DOWN >= 0 (seconds), --exposure-range MIN MAX with MIN <= MAX, "
                            "--exposure-percentiles LOW HIGH >= 0 with LOW + HIGH < 1000\n");
            return 2;
        }
    }
    // panoramas: the spans are checked by the host query (the launch's own refusals), the combinations the kernels lack up front
    const bool pano = projection != RRT_PROJ_PINHOLE;
    rrt_projection proj;
    rrt_projection_default(projection, &proj);
    if (!pano && (fov != 0.0f || vfov != 0.0f)) { fprintf(stderr, "--fov / --vfov need --projection equirect | fisheye\n"); return 2; }
    if (projection == RRT_PROJ_FISHEYE && vfov != 0.0f) { fprintf(stderr, "--vfov: equirect only (a fisheye's aperture is --fov)\n"); return 2; }
    if (fov != 0.0f) proj.fov_deg = fov;
    if (vfov != 0.0f) proj.vfov_deg = vfov;
    if (pano) {
        const rrt_camera c0 = {};
        float d[3];
        if (rrt_projection_ray(&proj, 1, 1, 0, 0, &c0, d, nullptr) != RRT_OK) {
            fprintf(stderr, "--fov DEG in (0, 360], --vfov DEG in (0, 180]\n"); return 2;
        }
        if (motion > 1) { fprintf(stderr, "rrt_headless: a panorama renders one instant per frame (--motion-blur 1)\n"); return 2; }
        if (projection == RRT_PROJ_EQUIRECT && use_glow) {
            fprintf(stderr, "rrt_headless: --glow clamps at the frame's edge and an equirect frame wraps: not with --projection equirect\n");
            return 2;
        }
    }
    // stereo: the values are checked by the host query (the launch's own refusals), the combinations the kernel lacks up front;
    // --width / --height stay per eye (ew x eh, what the launch takes), w x h becomes the composite that is sharded and written
    const bool use_stereo = stereo_layout != 0;
    const int ew = w, eh = h;
    if (!use_stereo && (stereo_base || stereo_conv || stereo_merge)) {
        fprintf(stderr, "usage: --stereo-base / --convergence / --pole-merge need --stereo top-bottom | side-by-side\n"); return 2;
    }
    if (use_stereo) {
        stereo.layout = stereo_layout;
        if (projection == RRT_PROJ_FISHEYE) { fprintf(stderr, "usage: --stereo: pinhole or equirect (no stereo fisheye domes)\n"); return 2; }
        if (motion > 1) { fprintf(stderr, "usage: --stereo renders one instant per frame (--motion-blur 1)\n"); return 2; }
        if (use_glow) { fprintf(stderr, "usage: --stereo: not with --glow\n"); return 2; }
        if (stereo_conv && projection != RRT_PROJ_PINHOLE) { fprintf(stderr, "usage: --convergence: pinhole only\n"); return 2; }
        if (stereo_merge && projection != RRT_PROJ_EQUIRECT) { fprintf(stderr, "usage: --pole-merge: equirect only\n"); return 2; }
        const rrt_camera c0 = {};
        float o[3], d[3];
        if (rrt_stereo_ray(&proj, &stereo, 1, 1, RRT_EYE_LEFT, 0, 0, &c0, o, d, nullptr) != RRT_OK) {
            fprintf(stderr, "usage: --stereo-base B >= 0, --convergence Z >= 0, --pole-merge FROM TO with 0 <= FROM <= TO <= 90\n"); return 2;
        }
        if (stereo_layout == RRT_STEREO_SIDE_BY_SIDE) w = 2 * ew; else h = 2 * eh;
    }
    // adaptive supersampling needs the whole frame on one device (the mask looks at every pixel's neighbours; no _tiles form)
    if (use_adaptive) {
        if (supersample <= 1) { fprintf(stderr, "usage: --adaptive needs --supersample 2 | 4 | 8\n"); return 2; }
        if (gpus > 1 || force_collective) { fprintf(stderr, "usage: --adaptive renders on one GPU only (--gpus 1)\n"); return 2; }
        if (motion > 1) { fprintf(stderr, "usage: --adaptive renders one instant per frame (--motion-blur 1)\n"); return 2; }
        if (use_stereo) { fprintf(stderr, "usage: --adaptive: not with --stereo\n"); return 2; }
    }
    // depth of field: a thin lens in front of the pinhole camera; its K samples are the shutter's sub-frames when there are any
    if (!use_dof && (dof_focus_given || dof_samples != 0)) { fprintf(stderr, "usage: --focus / --dof-samples need --dof APERTURE\n"); return 2; }
    int dof_k = 0;
    float dof_xy[32];
    if (use_dof) {
        if (pano) { fprintf(stderr, "usage: --dof: a thin lens in front of a pinhole camera, not with --projection equirect | fisheye\n"); return 2; }
        if (use_stereo) { fprintf(stderr, "usage: --dof: not with --stereo\n"); return 2; }
        if (use_adaptive) { fprintf(stderr, "usage: --dof: not with --adaptive\n"); return 2; }
        if (motion > 1 && dof_samples != 0 && dof_samples != motion) {
            fprintf(stderr, "usage: --dof-samples: with --motion-blur M > 1 the lens samples are the shutter's sub-frames (K = M)\n"); return 2;
        }
        dof_k = motion > 1 ? motion : (dof_samples != 0 ? dof_samples : 8);
        float spiral[32];
        if (rrt_lens_points(dof_aperture, dof_k, 0.0f, spiral) != RRT_OK) { fprintf(stderr, "usage: --dof APERTURE: the lens radius in scene units, >= 0\n"); return 2; }
        for (int m = 0; m < dof_k; ++m) {       // sample m looks through lens point bitrev_K(m): the spiral's radius grows with its index
            int r = 0;
            for (int b = 1, v = m; b < dof_k; b <<= 1, v >>= 1) r = (r << 1) | (v & 1);
            dof_xy[2 * m] = spiral[2 * r]; dof_xy[2 * m + 1] = spiral[2 * r + 1];
        }
    }
    // a supersampled launch is always the single kernel in the static order (include/rrt.h): no pool, no path choice, no tile order
    if (supersample > 1 || motion > 1 || use_glow || use_exposure || pano || use_stereo || use_dof) { workspace_gib = 0; path_window = -1; tile_order = 0; }
    int n_dev = 0, rc;
    if ((rc = rrt_device_count(&n_dev)) != RRT_OK) return fail("no GPU", rc);
    if (gpus > n_dev) { fprintf(stderr, "rrt_headless: --gpus %d but %d device(s) visible\n", gpus, n_dev); return 2; }
    const bool collective = gpus > 1 || force_collective;
    trace("start");
    std::thread dog(watchdog, init_timeout, frame_timeout);
    struct DogStop { std::thread& t; ~DogStop() { g_tr.stop.store(true); t.join(); } } dog_stop{dog};      // every return path
    // the RCCL library's pages, read sequentially in the background while the per-device resources are set up
    std::thread warm;
    if (collective && !getenv("RRT_NO_LIBRARY_WARMUP")) warm = std::thread(warm_library_pages, (const void*)&ncclCommInitAll);
    struct WarmJoin { std::thread& t; ~WarmJoin() { if (t.joinable()) t.join(); } } warm_join{warm};
    // a failing communicator says why (RCCL prints nothing below WARN); the caller's setting wins
    if (collective) setenv("NCCL_DEBUG", "WARN", 0);
    // one process, one node: RCCL's bootstrap and RAS sockets need no interface but the loopback (by default it picks
    // the first non-loopback one -- in a container a veth whose state is not this program's business)
    if (collective) setenv("NCCL_SOCKET_IFNAME", "lo", 0);

    // the recording clock (main.cpp:511-516) says which times the sequence reaches; the tables slide along it
    float seq_end = 0.0f;
    { float unused = 0.0f; rrt_recording_clock(frames, fps, &seq_end, &unused); seq_end += 1.0f; }
    const size_t table_budget = table_gib > 0.0 ? (size_t)(table_gib * (double)(1ull << 30)) : 0;
    if (table_budget == 0) use_table = 0;
    int table_builds = 0, table_frames = 0, arith_frames = 0, coarsest = RRT_TABLE_FULL;
    size_t table_peak = 0;
    bool table_warned = false;
    float win_t0 = 0.0f, win_t1 = -1.0f;         // the window the devices' tables (or the remembered failure) cover; empty at first
    bool win_has_table = false;

    std::vector<uint8_t> sky;
    int sky_w = 2048, sky_h = 1024;
    if (sky_path.empty()) sky = synthetic_sky(sky_w, sky_h, sky_seed);
    else if (!load_sky_raw(sky_path, sky, sky_w, sky_h)) return 2;
    rrt_effects fx; rrt_effects_default(&fx);
    fx.use_chromatic_aberration = (uint8_t)all_fx;

    // ---- per-device resources
    std::vector<Device> dev(gpus);
    size_t shard_stride = 0;                       // bytes between shards in the gathered buffer
    for (int d = 0; d < gpus; ++d) {
        int rows = 0;
        rrt_tile_shard_rows(h, tile_rows, d, gpus, &rows);
        dev[d].shard_rows = rows;
        if ((size_t)rows * w * 4 > shard_stride) shard_stride = (size_t)rows * w * 4;
    }
    shard_stride = (shard_stride + 255) & ~(size_t)255;
    for (int d = 0; d < gpus; ++d) {
        Device& D = dev[d];
        D.id = d;
        HIPCHK(hipSetDevice(d));
        const int rows = collective ? D.shard_rows : h;            // image rows of one launch on this device
        if ((rc = rrt_sky_create(sky.data(), sky_w, sky_h, &D.sky)) != RRT_OK) return fail("sky", rc);
        HIPCHK(hipMalloc(&D.probe, 256 * (size_t)(gpus + 1)));
        HIPCHK(hipEventCreateWithFlags(&D.comm_free, hipEventDisableTiming));
        // the path is a choice only where a launch could take either: a pool, a share under RRT_PATH_AUTO's threshold, frames in
        // flight (one frame at a time the three-pass path's two chains win: DESIGN.md section 5)
        if (path_window >= 0 && kSlots >= 2 && workspace_gib > 0 && (long long)w * rows <= (long long)rrt_path_auto_max_rays()) {
            if ((rc = rrt_path_chooser_create(kSlots, path_window, &D.chooser)) != RRT_OK) return fail("path chooser", rc);
            for (int e = 0; e < 2 * kSlots; ++e) HIPCHK(hipEventCreate(&D.render_end[e]));
        }
        for (int s = 0; s < kSlots; ++s) {
            HIPCHK(hipStreamCreateWithFlags(&D.stream[s], hipStreamNonBlocking));
            HIPCHK(hipMalloc(&D.tiles[s], shard_stride));
            if (workspace_gib > 0 && (rc = rrt_workspace_create(((size_t)workspace_gib << 30) / kSlots, &D.pool[s])) != RRT_OK)
                return fail("workspace", rc);
            // every frame's wave tiles dispatched longest-first by what the slot's previous frame measured (the first frame: by
            // the library's probe of the view): worth it when the frames do not overlap (their drains are exposed) AND the
            // launch takes the single kernel; a wash when frames overlap, and measured harmful on the three-pass path's two
            // chains (it piles every expensive tile into the first chain: an eighth of a 4K frame 5.15 -> 5.45 ms, of a
            // disk-heavy one 7.7 -> 10.6; profiles/r04_shard_kernel_times_*.txt), which is what small launches with a pool take
            const bool three_pass_likely = workspace_gib > 0 && (long long)w * rows <= (long long)rrt_path_auto_max_rays();   // RRT_PATH_AUTO's own threshold
            if ((tile_order == 1 || (tile_order < 0 && kSlots == 1 && !three_pass_likely)) && (rc = rrt_tile_order_create(&D.order[s])) != RRT_OK)
                return fail("tile order", rc);
        }
    }
    trace("per-device resources ready");
    if (collective) {
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
    }
    // device 0: gathered shards + assembled frame, per slot; pinned host frames for the sink
    HIPCHK(hipSetDevice(0));
    void* gathered[kMaxSlots] = {};
    void* frame[kMaxSlots] = {};
    void* host[kMaxSlots] = {};
    void* hdr[kMaxSlots] = {};         // --glow / --exposure: each slot's linear frame; the glow's scratch
    void* glow_scratch[kMaxSlots] = {};
    // --auto-exposure: ONE state for the sequence.  The frames' renders overlap on their slots' streams; their exposure passes run in
    // frame order, each behind the event its predecessor recorded
    void* exposure_scratch = nullptr;
    size_t exposure_bytes = 0;
    hipEvent_t exposed = nullptr;
    const bool auto_exposure = use_exposure && exposure.mode == RRT_EXPOSURE_AUTO;
    if (auto_exposure) {
        if ((rc = rrt_exposure_scratch_bytes(&exposure_bytes)) != RRT_OK) return fail("exposure scratch", rc);
        HIPCHK(hipMalloc(&exposure_scratch, exposure_bytes));
        HIPCHK(hipEventCreateWithFlags(&exposed, hipEventDisableTiming));
        if ((rc = rrt_launch_exposure_reset(exposure_scratch, exposure_bytes, dev[0].stream[0])) != RRT_OK) return fail("exposure reset", rc);
    }
    void* ad_scratch[kMaxSlots] = {};  // --adaptive: each slot's list, and the pinned word its count is copied to
    void* ad_count[kMaxSlots] = {};
    size_t ad_bytes = 0;
    if (use_adaptive && (rc = rrt_adaptive_scratch_bytes(w, h, &ad_bytes)) != RRT_OK) return fail("adaptive scratch", rc);
    unsigned long long refined_total = 0;
    hipEvent_t done[kMaxSlots];
    const size_t frame_bytes = (size_t)w * h * 4;
    for (int s = 0; s < kSlots; ++s) {
        HIPCHK(hipMalloc(&gathered[s], shard_stride * gpus));
        HIPCHK(hipMalloc(&frame[s], frame_bytes));
        if (use_glow || use_exposure) HIPCHK(hipMalloc(&hdr[s], frame_bytes * sizeof(float)));
        if (use_glow) HIPCHK(hipMalloc(&glow_scratch[s], glow_bytes));
        if (use_adaptive) { HIPCHK(hipMalloc(&ad_scratch[s], ad_bytes)); HIPCHK(hipHostMalloc(&ad_count[s], 4, hipHostMallocDefault)); }
        HIPCHK(hipEventCreateWithFlags(&done[s], hipEventDisableTiming));
    }
    FILE* f = out_path.empty() ? nullptr : fopen(out_path.c_str(), "wb");
    if (!out_path.empty() && !f) { perror("fopen"); return 1; }
    if (f) for (int s = 0; s < kSlots; ++s) HIPCHK(hipHostMalloc(&host[s], frame_bytes, hipHostMallocDefault));

    rrt_camera cam;
    const float start_pos[3] = {0.0f, 10.0f, -60.0f};
    rrt_camera_from_angles(start_pos, 0.0f, -10.0f, &cam);
    const char* path_name = "";
    if (path >= 0 && (rc = rrt_path_info(path, &path_name, nullptr, nullptr)) != RRT_OK) return fail("path", rc);

    // write frame `k`'s pixels once its copy has landed (called one frame late, so that the copy overlaps the next render)
    // (without a sink the wait still happens: the host never runs more than kSlots frames ahead of the device, a device
    // fault is reported at the frame it belongs to, and the watchdog sees frames complete)
    int delivered = 0;
    auto deliver = [&](int slot) -> int {
        HIPCHK(hipEventSynchronize(done[slot]));
        trace("frame complete", ++delivered);
        if (use_adaptive) refined_total += *static_cast<const uint32_t*>(ad_count[slot]);
        // frame `delivered` has been rendered on every device (the gather waited for all shards): its sustained time on a device =
        // the interval between the ends of frame delivered - 1's and its own render there
        if (delivered >= 2) for (int d = 0; d < gpus; ++d) if (dev[d].chooser) {
            float ms = 0.0f;
            HIPCHK(hipSetDevice(d));
            if (hipEventElapsedTime(&ms, dev[d].render_end[(delivered - 1) % (2 * kSlots)], dev[d].render_end[delivered % (2 * kSlots)]) == hipSuccess)
                rrt_path_chooser_report(dev[d].chooser, delivered, ms > 0.0f ? ms : 0.0f);   // (a frame that ended before its predecessor: 0)
        }
        if (f && fwrite(host[slot], 1, frame_bytes, f) != frame_bytes) fprintf(stderr, "Warning: Frame write incomplete\n");
        return 0;
    };

    for (int d = 0; d < gpus; ++d) { HIPCHK(hipSetDevice(d)); HIPCHK(hipDeviceSynchronize()); }
    trace("bring-up complete; rendering");
    g_tr.in_frames.store(true);
    auto t0 = std::chrono::steady_clock::now();
    for (int k = 1; k <= frames; ++k) {
        const int slot = k % kSlots;
        float sim_t = 0.0f, path_t = 0.0f;
        rrt_recording_clock(k, fps, &sim_t, &path_t);
        if (path >= 0 && (rc = rrt_path_camera_at(path, path_t, &cam)) != RRT_OK) return fail("camera", rc);
        // motion blur: the shutter's sub-times and the path camera at each; the noise table's window is fitted from the earliest
        float sub_t[16], sub_p[16];
        rrt_camera sub_cam[16];
        float fit_t = sim_t;
        if (motion > 1) {
            rrt_motion_clock(k, fps, shutter, motion, sub_t, sub_p);
            for (int m = 0; m < motion; ++m) {
                sub_cam[m] = cam;
                if (path >= 0 && (rc = rrt_path_camera_at(path, sub_p[m], &sub_cam[m])) != RRT_OK) return fail("camera", rc);
            }
            fit_t = sub_t[0];
        }
        // depth of field: without a shutter the K samples share the frame's instant; --focus hole: the camera position's distance to
        // the origin, the double root of the sum of the exact squares in x, y, z order, rounded to float (headless.py's)
        float focus = dof_focus;
        if (use_dof) {
            if (motion <= 1) for (int m = 0; m < dof_k; ++m) { sub_t[m] = sim_t; sub_cam[m] = cam; }
            if (focus == 0.0f) {
                const double x = cam.pos[0], y = cam.pos[1], z = cam.pos[2];
                focus = (float)std::sqrt(x * x + y * y + z * z);
            }
        }
        trace("frame", k);
        // slot reuse: frame k-kSlots used the same buffers; its host copy must have been written out
        if (k > kSlots && deliver(slot)) return 1;
        // 0. noise tables: when the clock has left the window, every device builds the next one (after its frames in
        //    flight, which may still read the old table, have drained).  The window is ONE decision for all devices: if it
        //    cannot be built on any of them (nothing fits the budget, out of memory) it is dropped on all of them and
        //    REMEMBERED -- no new fit, no device synchronise, no retry until the clock has left it (retrying
        //    every frame serialised the frames in flight and rebuilt the other devices' tables for nothing).
        const bool in_window = fit_t >= win_t0 && fit_t <= win_t1;
        if (use_table && !in_window) {
            float t1 = fit_t; int cov = RRT_TABLE_FULL; size_t bytes = 0;
            // trace points around the rebuild: it synchronises every device and creates a table on each, which on a
            // starved box takes time that must neither count against --frame-timeout under the name of the last frame nor
            // leave the watchdog's notices pointing at the wrong phase
            trace("noise table window: fitting", k);
            rrt_noise_table_fit_window(fit_t, seq_end > fit_t ? seq_end : fit_t, table_budget, &t1, &cov, &bytes);
            bool ok = bytes != 0;
            for (int d = 0; d < gpus; ++d) {
                Device& D = dev[d];
                HIPCHK(hipSetDevice(d));
                trace("noise table window: draining and rebuilding on device", d);
                HIPCHK(hipDeviceSynchronize());
                if (D.noise_table) { rrt_noise_table_destroy(D.noise_table); D.noise_table = 0; }
                if (ok && (rc = rrt_noise_table_create_window(fit_t, t1, cov, &D.noise_table)) != RRT_OK) {
                    D.noise_table = 0;
                    ok = false;
                    if (!table_warned) {
                        fprintf(stderr, "rrt_headless: noise table [%g, %g] not built on device %d: %s (%s); hashing arithmetically\n",
                                fit_t, t1, d, rrt_status_string(rc), rrt_last_hip_error());
                        table_warned = true;
                    }
                }
            }
            if (!ok) {      // all or nothing: the devices must agree on which kernels a frame runs for the timing to mean anything
                for (int d = 0; d < gpus; ++d) if (dev[d].noise_table) { HIPCHK(hipSetDevice(d)); rrt_noise_table_destroy(dev[d].noise_table); dev[d].noise_table = 0; }
                if (bytes == 0) t1 = fit_t + 5.0f;          // nothing fits: look again after 5 s of sim time
            }
            win_t0 = fit_t; win_t1 = t1; win_has_table = ok;
            trace("noise table window: done", k);
            if (ok) { ++table_builds; if (cov > coarsest) coarsest = cov; if (bytes > table_peak) table_peak = bytes; }
        }
        if (use_table && win_has_table) ++table_frames; else ++arith_frames;
        // 1. every device renders its tiles
        for (int d = 0; d < gpus; ++d) {
            Device& D = dev[d];
            HIPCHK(hipSetDevice(d));
            rrt_params prm; rrt_params_default(&prm);
            prm.spin = spin; prm.arith_mode = arith;
            prm.workspace = D.pool[slot]; prm.noise_table = D.noise_table; prm.tile_order = D.order[slot];
            // frames in flight fill each other's drains: ONE chain per launch (the second chain's streams only compete with the other
            // frames: 2-7 % per frame, profiles/r05_sustained_chains.txt).  The plain single kernel would be faster still on most views,
            // but its longest wavefront (up to 19 ms on a disk-grazing view) bounds a slot's frame rate; a moving camera keeps the
            // path that is never slow
            prm.pass_chains = kSlots >= 2 ? 1 : 0;
            // ... per window, by measurement: rrt_path_chooser (csrc/rrt_path_chooser.cpp) tries the single kernel for a few frames
            // of a window, keeps it where it sustains the faster frames, and drops it at once on a frame that takes > 1.5 x the
            // three-pass median (same bytes either way)
            if (D.chooser) { int pol = RRT_PATH_AUTO; rrt_path_chooser_policy(D.chooser, k, &pol); prm.path_policy = pol; }
            else if (path_policy >= 0) prm.path_policy = path_policy;
            void* dst = collective ? D.tiles[slot] : frame[slot];
            // the stereo / defocused / panorama / blurred / supersampled launch (_stereo, _dof, _pano, _mb, _ss): this device's tiles, or the whole frame and
            // its HDR (may be NULL)
            auto launch_sampled = [&](bool tiles, float* lin) {
                if (use_stereo) return tiles ? rrt_launch_raymarch_stereo_tiles(dst, ew, eh, supersample, tile_rows, d, gpus, &proj, &stereo, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot])
                                             : rrt_launch_raymarch_stereo(dst, lin, ew, eh, supersample, &proj, &stereo, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot]);
                if (use_dof) return tiles ? rrt_launch_raymarch_dof_tiles(dst, w, h, supersample, tile_rows, d, gpus, dof_k, sub_t, sub_cam, dof_xy, focus, D.sky, &fx, &prm, D.stream[slot])
                                          : rrt_launch_raymarch_dof(dst, lin, w, h, supersample, dof_k, sub_t, sub_cam, dof_xy, focus, D.sky, &fx, &prm, D.stream[slot]);
                if (pano) return tiles ? rrt_launch_raymarch_pano_tiles(dst, w, h, supersample, tile_rows, d, gpus, &proj, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot])
                                       : rrt_launch_raymarch_pano(dst, lin, w, h, supersample, &proj, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot]);
                if (motion > 1) return tiles ? rrt_launch_raymarch_mb_tiles(dst, w, h, supersample, tile_rows, d, gpus, motion, sub_t, sub_cam, D.sky, &fx, &prm, D.stream[slot])
                                             : rrt_launch_raymarch_mb(dst, lin, w, h, supersample, motion, sub_t, sub_cam, D.sky, &fx, &prm, D.stream[slot]);
                return tiles ? rrt_launch_raymarch_ss_tiles(dst, w, h, supersample, tile_rows, d, gpus, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot])
                             : rrt_launch_raymarch_ss(dst, lin, w, h, supersample, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot]);
            };
            // --adaptive: one device (checked above), the whole frame and its HDR (may be NULL); the count of refined pixels follows
            // in a 4-byte asynchronous copy, read when the frame is delivered
            auto launch_adaptive = [&](float* lin) {
                const int st = rrt_launch_raymarch_adaptive(dst, lin, w, h, supersample, pano ? &proj : nullptr, &adaptive, sim_t, &cam, D.sky,
                                                            &fx, &prm, ad_scratch[slot], ad_bytes, D.stream[slot]);
                if (st == RRT_OK && hipMemcpyAsync(ad_count[slot], ad_scratch[slot], 4, hipMemcpyDeviceToHost, D.stream[slot]) != hipSuccess)
                    return (int)RRT_ERR_HIP;
                return st;
            };
            if (use_glow || use_exposure) {     // one device (checked above): the slot's HDR through launch_sampled, then the post passes on the same stream
                float* lin = static_cast<float*>(hdr[slot]);
                rc = use_adaptive ? launch_adaptive(lin) : launch_sampled(false, lin);
                if (rc == RRT_OK && use_exposure) {     // the bytes -- or, in front of the glow, the scaled HDR in place
                    if (auto_exposure) HIPCHK(hipStreamWaitEvent(D.stream[slot], exposed, 0));
                    rc = rrt_launch_exposure(use_glow ? nullptr : dst, use_glow ? lin : nullptr, lin, w, h, &exposure, exposure_scratch,
                                             exposure_bytes, D.stream[slot]);
                    if (auto_exposure) HIPCHK(hipEventRecord(exposed, D.stream[slot]));
                }
                if (rc == RRT_OK && use_glow) rc = rrt_launch_glow(dst, lin, w, h, &glow, glow_scratch[slot], glow_bytes, D.stream[slot]);
            }
            else if (use_adaptive) rc = launch_adaptive(nullptr);
            else if (use_stereo || use_dof || pano || motion > 1 || supersample > 1) rc = launch_sampled(collective, nullptr);
            else if (collective) rc = rrt_launch_raymarch_tiles(dst, w, h, tile_rows, d, gpus, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot]);
            else rc = rrt_launch_raymarch(dst, w, h, sim_t, &cam, D.sky, &fx, &prm, D.stream[slot]);
            if (rc != RRT_OK) return fail("launch", rc);
            if (D.chooser) HIPCHK(hipEventRecord(D.render_end[k % (2 * kSlots)], D.stream[slot]));
        }
        // 2. one gather: every device sends its shard, device 0 receives all of them (its own included)
        if (collective) {
            // Successive frames use the SAME communicators from DIFFERENT streams (slot k mod kSlots).  RCCL orders the
            // operations of one communicator by itself; the event chain states that order in the stream graph as well:
            // a device's part of exchange k starts after its part of exchange k-1 has finished, whatever streams they ran on.
            if (k > 1) for (int d = 0; d < gpus; ++d) { HIPCHK(hipSetDevice(d)); HIPCHK(hipStreamWaitEvent(dev[d].stream[slot], dev[d].comm_free, 0)); }
            NCCLCHK(ncclGroupStart());
            for (int d = 0; d < gpus; ++d) {
                const size_t bytes = (size_t)dev[d].shard_rows * w * 4;
                if (bytes == 0) continue;
                NCCLCHK(ncclSend(dev[d].tiles[slot], bytes, ncclUint8, 0, dev[d].comm, dev[d].stream[slot]));
                NCCLCHK(ncclRecv(static_cast<uint8_t*>(gathered[slot]) + (size_t)d * shard_stride, bytes, ncclUint8, d, dev[0].comm,
                                 dev[0].stream[slot]));
            }
            NCCLCHK(ncclGroupEnd());
            for (int d = 0; d < gpus; ++d) { HIPCHK(hipSetDevice(d)); HIPCHK(hipEventRecord(dev[d].comm_free, dev[d].stream[slot])); }
            // 3. device 0 scatters the shards into the bottom-up frame
            HIPCHK(hipSetDevice(0));
            if ((rc = rrt_assemble_all_tiles(frame[slot], gathered[slot], shard_stride, w, h, tile_rows, gpus, dev[0].stream[slot])) != RRT_OK)
                return fail("assemble", rc);
        }
        // 4. hand the frame to the sink: asynchronous copy now, the write happens one frame later
        HIPCHK(hipSetDevice(0));
        if (f) HIPCHK(hipMemcpyAsync(host[slot], frame[slot], frame_bytes, hipMemcpyDeviceToHost, dev[0].stream[slot]));
        HIPCHK(hipEventRecord(done[slot], dev[0].stream[slot]));
    }
    trace("all frames enqueued; draining");
    // drain: the last min(frames, kSlots) frames, oldest first
    for (int k = frames - kSlots + 1; k <= frames; ++k)
        if (k >= 1 && deliver(k % kSlots)) return 1;
    for (int d = 0; d < gpus; ++d) { HIPCHK(hipSetDevice(d)); HIPCHK(hipDeviceSynchronize()); }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (f) fclose(f);
    std::string choice = "null";
    if (dev[0].chooser) {
        choice = "[";
        for (int d = 0; d < gpus; ++d) {
            rrt_path_chooser_stats st;
            rrt_path_chooser_get_stats(dev[d].chooser, &st);
            char buf[256];
            snprintf(buf, sizeof(buf), "%s{\"device\": %d, \"frames_three_pass\": %d, \"frames_single_kernel\": %d, \"windows\": %d, \"trials\": %d, "
                     "\"trials_aborted\": %d, \"switches\": %d, \"outliers\": %d}", d ? ", " : "", d, st.frames[0], st.frames[1], st.windows, st.trials,
                     st.trials_aborted, st.switches, st.outliers);
            choice += buf;
        }
        choice += "]";
    }
    std::string glow_json = "null";
    if (use_glow) {
        char buf[160];
        snprintf(buf, sizeof(buf), "{\"radius\": %g, \"lobes\": %d, \"threshold\": %g, \"intensity\": %g}", glow.radius, glow.lobes,
                 glow.threshold, glow.intensity);
        glow_json = buf;
    }
    std::string exposure_json = "null";
    if (use_exposure) {     // the final EV: one 4-byte read of the state, after the last frame
        float final_ev = exposure.ev;
        if (auto_exposure) HIPCHK(hipMemcpy(&final_ev, static_cast<const uint8_t*>(exposure_scratch) + RRT_EXPOSURE_STATE_OFFSET, 4, hipMemcpyDeviceToHost));
        char buf[400];
        snprintf(buf, sizeof(buf), "{\"mode\": \"%s\", \"ev\": %.9g, \"key\": %.9g, \"low_permille\": %d, \"high_permille\": %d, \"min_ev\": %.9g, "
                 "\"max_ev\": %.9g, \"adapt_up\": %.9g, \"adapt_down\": %.9g, \"final_ev\": %.9g}", auto_exposure ? "auto" : "manual", exposure.ev,
                 exposure.key, exposure.low_permille, exposure.high_permille, exposure.min_ev, exposure.max_ev, exposure.adapt_up,
                 exposure.adapt_down, final_ev);
        exposure_json = buf;
    }
    const char* proj_name = projection == RRT_PROJ_EQUIRECT ? "equirect" : (projection == RRT_PROJ_FISHEYE ? "fisheye" : "pinhole");
    char fov_json[32] = "null", vfov_json[32] = "null";
    if (pano) snprintf(fov_json, sizeof(fov_json), "%g", proj.fov_deg);
    if (projection == RRT_PROJ_EQUIRECT) snprintf(vfov_json, sizeof(vfov_json), "%g", proj.vfov_deg);
    std::string stereo_json = "null";
    if (use_stereo) {
        char buf[200];
        snprintf(buf, sizeof(buf), "{\"layout\": \"%s\", \"base\": %.17g, \"convergence\": %.17g, \"pole_merge_deg\": [%.17g, %.17g]}",
                 stereo_layout == RRT_STEREO_TOP_BOTTOM ? "top-bottom" : "side-by-side", stereo.base, stereo.convergence,
                 stereo.pole_merge_from_deg, stereo.pole_merge_to_deg);
        stereo_json = buf;
    }
    std::string adaptive_json = "null";
    if (use_adaptive) {
        char buf[128];
        snprintf(buf, sizeof(buf), "{\"threshold\": %d, \"refined_fraction\": %.9g}", adaptive.threshold,
                 frames > 0 ? (double)refined_total / ((double)frames * w * h) : 0.0);
        adaptive_json = buf;
    }
    std::string dof_json = "null";
    if (use_dof) {
        char buf[160], z[40];
        if (dof_focus == 0.0f) snprintf(z, sizeof(z), "\"hole\""); else snprintf(z, sizeof(z), "%.9g", dof_focus);
        snprintf(buf, sizeof(buf), "{\"aperture\": %.9g, \"focus\": %s, \"samples\": %d}", dof_aperture, z, dof_k);
        dof_json = buf;
    }
    /* which path the frames took through each device's march cache (launches without a workspace: one GPU, or --workspace-gib 0) */
    std::string cache_json = "[";
    for (int d = 0; d < gpus; ++d) {
        rrt_march_cache_info mc = {};
        (void)rrt_march_cache_stats(d, &mc);
        char buf[256];
        snprintf(buf, sizeof(buf), "%s{\"device\": %d, \"fills\": %llu, \"hits\": %llu, \"drops\": %llu, \"misses\": %llu, \"uncacheable\": %llu, "
                 "\"bytes\": %llu, \"max_bytes\": %llu}", d ? ", " : "", d, (unsigned long long)mc.fills, (unsigned long long)mc.hits,
                 (unsigned long long)mc.drops, (unsigned long long)mc.misses, (unsigned long long)mc.uncacheable, (unsigned long long)mc.bytes,
                 (unsigned long long)mc.max_bytes);
        cache_json += buf;
    }
    cache_json += "]";
    printf("{\"frames\": %d, \"width\": %d, \"height\": %d, \"n_gpus\": %d, \"seconds\": %.4f, \"fps\": %.3f, \"Mrays_per_s\": %.3f, "
           "\"path\": \"%s\", \"spin\": %g, \"arith_mode\": \"%s\", \"noise_tables\": {\"builds\": %d, \"table_frames\": %d, "
           "\"arith_frames\": %d, \"coarsest_coverage\": %d, \"peak_bytes\": %zu, \"budget_bytes\": %zu}, \"tile_order\": %s, \"collective\": \"%s\", "
           "\"path_choice\": %s, \"supersample\": %d, \"motion_blur\": %d, \"shutter\": %g, \"glow\": %s, "
           "\"projection\": \"%s\", \"fov_deg\": %s, \"vfov_deg\": %s, \"stereo\": %s, \"dof\": %s, \"adaptive\": %s, \"exposure\": %s, "
           "\"march_cache\": %s}\n",
           frames, w, h, gpus, dt, frames / dt, (double)frames * w * h / dt / 1e6, path_name, spin,
           arith == RRT_ARITH_FAST ? "fast" : (arith == RRT_ARITH_FMAD ? "fmad" : "strict"),
           table_builds, table_frames, arith_frames, coarsest, table_peak, table_budget, dev[0].order[0] ? "true" : "false",
           collective ? "rccl grouped send/recv gather" : "none", choice.c_str(), supersample, motion, shutter, glow_json.c_str(),
           proj_name, fov_json, vfov_json, stereo_json.c_str(), dof_json.c_str(), adaptive_json.c_str(), exposure_json.c_str(),
           cache_json.c_str());

    for (int d = 0; d < gpus; ++d) {
        Device& D = dev[d];
        HIPCHK(hipSetDevice(d));
        if (D.comm) ncclCommDestroy(D.comm);
        (void)hipFree(D.probe);
        (void)hipEventDestroy(D.comm_free);
        if (D.chooser) { rrt_path_chooser_destroy(D.chooser); for (int e = 0; e < 2 * kSlots; ++e) (void)hipEventDestroy(D.render_end[e]); }
        for (int s = 0; s < kSlots; ++s) {
            if (D.pool[s]) rrt_workspace_destroy(D.pool[s]);
            if (D.order[s]) rrt_tile_order_destroy(D.order[s]);
            (void)hipFree(D.tiles[s]);
            (void)hipStreamDestroy(D.stream[s]);
        }
        if (D.noise_table) rrt_noise_table_destroy(D.noise_table);
        rrt_sky_destroy(D.sky);
    }
    HIPCHK(hipSetDevice(0));
    (void)hipFree(exposure_scratch);
    if (exposed) (void)hipEventDestroy(exposed);
    for (int s = 0; s < kSlots; ++s) {
        (void)hipFree(gathered[s]); (void)hipFree(frame[s]); (void)hipFree(hdr[s]); (void)hipFree(glow_scratch[s]);
        (void)hipFree(ad_scratch[s]);
        if (ad_count[s]) (void)hipHostFree(ad_count[s]);
        if (host[s]) (void)hipHostFree(host[s]);
    }
    return 0;
}
