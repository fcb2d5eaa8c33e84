#!/usr/bin/env python3
"""dev tool (GPU box): what the march cache does to the frames of the plain call site (launch_raymarch, no workspace).

    python tools/march_cache_frames.py still  [N] [W H]   N frames of ONE key (the bench view), time = 1.0 + 0.016 k, HIP events around
                                                         each launch: frame 1 marches, frame 2 fills, frames 3.. are replays
    python tools/march_cache_frames.py moving [N] [W H]   N frames of camera path 0, a new camera every frame (every launch a miss):
                                                         wall ms per frame with the launches queued back to back

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
