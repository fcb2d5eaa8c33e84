#!/usr/bin/env python3
"""dev tool (GPU box): what the march cache does to the frames of the plain call site (launch_raymarch, no workspace).

    python tools/march_cache_frames.py still  [N] [W H]   N frames of ONE key (the bench view), time = 1.0 + 0.016 k, HIP events around
                                                         each launch: frame 1 marches, frame 2 fills, frames 3.. are replays
    python tools/march_cache_frames.py moving [N] [W H]   N frames of camera path 0, a new camera every frame (every launch a miss):
                                                         wall ms per frame with the launches queued back to back
    python tools/march_cache_frames.py beside [N] [W H]   the still key's replays, N per set, HIP events per frame: queued back to back
                                                         or synchronised one at a time, alone or with rrt.clock_probe (one sleeping
                                                         wavefront) on a side stream spanning the set; each of the four sets twice

One JSON line each.  Runs against a build without the cache too (the statistics are then null): `moving` is the A/B of "a moving
camera must never pay" -- the per-launch cost of the cache's mutex, capture query and key compare against the parent.
RRT_MARCH_CACHE=0 switches the cache off.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    mode = sys.argv[1] if len(sys.argv) > 1 else "still"
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    w, h = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (3840, 2160)
    tex = rrt.SkyTexture(synthetic_sky(2048, 1024, seed=1))
    nt = rrt.NoiseTable(32.0)
    fx = rrt.CameraEffects()
    prm = rrt.RenderParams(spin=0.9, volumetrics=1, noise_table=nt.id)
    out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    tiny = torch.zeros(16 * 16 * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(tiny, 16, 16, 1.0, rrt.CameraState.default(), tex, fx, rrt.RenderParams(spin=0.9, max_steps=4))   # code object
    torch.cuda.synchronize()
    stats = getattr(rrt, "march_cache_stats", None)
    free0 = torch.cuda.mem_get_info()[0]
    res = {"mode": mode, "frames": n, "width": w, "height": h}
    if mode == "still":
        cam = rrt.CameraState.default()
        ms = []
        for k in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); rrt.launch_raymarch(out, w, h, 1.0 + 0.016 * k, cam, tex, fx, prm); e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 3))
        res["ms"] = ms
    elif mode == "beside":
        cam = rrt.CameraState.default()
        side = torch.cuda.Stream()
        cbuf = torch.zeros(2, dtype=torch.int64, device="cuda")
        it = [0]

        def frame():
            rrt.launch_raymarch(out, w, h, 1.0 + 0.016 * it[0], cam, tex, fx, prm)
            it[0] += 1

        for _ in range(4):                     # miss, fill, two replays
            frame()
        torch.cuda.synchronize()
        sets = {}
        for rep in range(2):                   # every set twice: the order of the sets must not be what is measured
            for name, sync_each, probe in (("queued", False, False), ("queued_probe", False, True),
                                           ("synced", True, False), ("synced_probe", True, True)):
                frame()                        # the probe goes out BEHIND a frame, as in bench.py (a chip that only sleeps drops its clocks)
                if probe:
                    rrt.clock_probe(cbuf, int(n * (8000 if sync_each else 4000)), stream=side)
                ev = []
                for _ in range(n):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); frame(); e1.record()
                    if sync_each:
                        e1.synchronize()
                    ev.append((e0, e1))
                torch.cuda.current_stream().synchronize()
                ms = [round(a.elapsed_time(b), 3) for a, b in ev]
                torch.cuda.synchronize()       # the probe's end
                sets.setdefault(name, []).append(ms)
        res["ms"] = sets
    else:
        from relativisticraytracer_amd import camera_paths
        path = camera_paths.CameraPath(0)
        cams = [path.camera_at(0.05 * k) for k in range(n)]
        runs = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                rrt.launch_raymarch(out, w, h, 1.0 + 0.016 * k, cams[k], tex, fx, prm)
            torch.cuda.synchronize()
            runs.append(round((time.perf_counter() - t0) * 1e3 / n, 4))
        res["ms_per_frame_runs"] = runs
    res["march_cache"] = stats() if stats else None
    res["device_bytes_taken"] = free0 - torch.cuda.mem_get_info()[0]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
