#!/usr/bin/env python3
"""Cost of full-size panoramas (launch_raymarch_pano) next to the 4K pinhole frame (HIP events, one JSON line).

    python tools/panorama_time.py [--views equirect:4096x2048 fisheye:4096x4096 pinhole:3840x2160] [--cameras default path0]
                                  [--arith strict fmad] [--reps 5 --warmup 1] [--spin 0.9 --time 1.0 --path-time 5.0]
                                  [--step-timeout 600]

Every (view, camera) is measured in a fresh child process (this script with --one) under `timeout -k 10 <step-timeout>`; the
first child that fails, faults or runs out of time ends the run (its exit status is reported, nothing else is started).  A child
renders the frame with a noise table over the clock, strict and FMAD, `warmup` untimed launches then `reps` timed ones, and reports
the medians, the rays (a fisheye's inside the disc) and Mrays/s.  pinhole:WxH is rrt_launch_raymarch_ss at s = 1, i.e. the bytes of
launch_raymarch in the single kernel's static order -- the bench frame's path.  Cameras: default = the reference's start-up view,
path0 = path 0 ("Gargantua Fly-By") at --path-time.  Per-kernel times: run a child under `rocprofv3 --kernel-trace --stats`.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def one(args):
    import numpy as np
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import camera_paths as cp
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    kind, size = args.one.split(":")
    w, h = (int(v) for v in size.split("x"))
    proj = rrt.Projection(kind)
    cam = rrt.CameraState.default() if args.camera == "default" else cp.CameraPath(0).camera_at(args.path_time)
    tex = rrt.SkyTexture(synthetic_sky())
    nt = rrt.NoiseTable(max(4.0, args.time + 1.0))
    fx = rrt.CameraEffects()
    out = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rays = w * h
    if kind == "fisheye":
        x = (2.0 * (np.arange(w, dtype=np.float32) + 0.5) - w) / h
        y = (2.0 * (np.arange(h, dtype=np.float32) + 0.5) - h) / h
        rays = int(((x[None, :] * x[None, :] + y[:, None] * y[:, None]) <= 1.0).sum())
    res = {"view": args.one, "camera": args.camera, "rays": rays}
    for arith in args.arith:
        prm = rrt.RenderParams(spin=args.spin, arith_mode={"strict": 0, "fast": 1, "fmad": 2}[arith], noise_table=nt.id)
        run = lambda: rrt.launch_raymarch_pano(out, w, h, 1, proj, args.time, cam, tex, fx, prm)
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        med = statistics.median(ms)
        res[arith] = {"ms": round(med, 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3), "Mrays_per_s": round(rays / med / 1e3, 1)}
    nt.destroy()
    tex.destroy()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", nargs="+", default=["equirect:4096x2048", "fisheye:4096x4096", "pinhole:3840x2160"])
    ap.add_argument("--cameras", nargs="+", default=["default", "path0"], choices=("default", "path0"))
    ap.add_argument("--arith", nargs="+", default=["strict", "fmad"], choices=("strict", "fmad", "fast"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--time", type=float, default=1.0)
    ap.add_argument("--path-time", type=float, default=5.0)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--camera", default="default", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args)
    common = ["--arith"] + args.arith + ["--reps", str(args.reps), "--warmup", str(args.warmup), "--spin", str(args.spin),
                                         "--time", str(args.time), "--path-time", str(args.path_time)]
    results, failed = [], None
    for cam in args.cameras:
        for view in args.views:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", view,
                   "--camera", cam] + common
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                failed = {"view": view, "camera": cam, "exit": r.returncode, "stderr": r.stderr[-1500:]}
                break
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if failed:
            break
    print(json.dumps({"tool": "panorama_time", "spin": args.spin, "time": args.time, "path_time": args.path_time, "noise_table": True,
                      "reps": args.reps, "warmup": args.warmup, "results": results, "failed": failed}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
