#!/usr/bin/env python3
"""Cost of adaptively supersampled frames (launch_raymarch_adaptive) next to the 1x and the full s x s frame (HIP events, one JSON line).

    python tools/adaptive_time.py [--sizes 1920x1080 3840x2160] [--samples 2 4] [--cameras default path0] [--arith strict fmad]
                                  [--threshold 8] [--reps 5 --warmup 1] [--spin 0.9 --time 1.0 --path-time 5.0] [--step-timeout 900]

Per (size, camera) a fresh child process (this script with --one) under `timeout -k 10 <step-timeout>`; the first child that fails,
faults or runs out of time ends the run (its exit status is reported, nothing else is started).  A child renders with a noise table
over the clock and measures, per arithmetic mode and s, four launches ALTERNATING -- a, b, c, d, a, b, ... -- `warmup` untimed rounds,
then `reps` timed ones, medians reported:
    a   launch_raymarch_ss at s = 1                     (a launch the 1x frame has had all along: the baseline)
    b   launch_raymarch_ss at s                         (the full supersampled frame: what the adaptive frame replaces)
    c   launch_raymarch_adaptive at --threshold         (base pass, zero, mask, refine)
    d   launch_raymarch_adaptive at threshold 255       (nothing refined: d - a is the mask pass and the empty refine pass)
and f, the refined fraction of c's frame (the count at the head of the scratch), c / b, and c / (a + f b): how far the packed,
scattered pixels fall from the ideal of paying f of the full frame on top of the base frame.  Cameras: default = the reference's
start-up view, path0 = path 0 ("Gargantua Fly-By") at --path-time.
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
    w, h = (int(v) for v in args.one.split("x"))
    cam = rrt.CameraState.default() if args.camera == "default" else cp.CameraPath(0).camera_at(args.path_time)
    tex = rrt.SkyTexture(synthetic_sky())
    nt = rrt.NoiseTable(max(4.0, args.time + 1.0))
    fx = rrt.CameraEffects()
    out = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(rrt.adaptive_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"size": args.one, "camera": args.camera, "pixels": w * h, "threshold": args.threshold, "rows": []}
    for arith in args.arith:
        prm = rrt.RenderParams(spin=args.spin, arith_mode={"strict": 0, "fast": 1, "fmad": 2}[arith], noise_table=nt.id)
        for s in args.samples:
            at_t, at_255 = rrt.AdaptiveSettings(args.threshold), rrt.AdaptiveSettings(255)
            runs = {"a": lambda: rrt.launch_raymarch_ss(out, w, h, 1, args.time, cam, tex, fx, prm),
                    "b": lambda: rrt.launch_raymarch_ss(out, w, h, s, args.time, cam, tex, fx, prm),
                    "c": lambda: rrt.launch_raymarch_adaptive(out, w, h, s, None, at_t, args.time, cam, tex, fx, scratch, prm),
                    "d": lambda: rrt.launch_raymarch_adaptive(out, w, h, s, None, at_255, args.time, cam, tex, fx, scratch, prm)}
            ms = {k: [] for k in runs}
            count = 0
            for rep in range(args.warmup + args.reps):
                for k, run in runs.items():
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    if rep >= args.warmup:
                        ms[k].append(e0.elapsed_time(e1))
                    if k == "c":
                        count = int(scratch[:4].cpu().numpy().view(np.uint32)[0])
            med = {k: statistics.median(v) for k, v in ms.items()}
            f = count / (w * h)
            res["rows"].append({"arith": arith, "s": s, "a_ms": round(med["a"], 3), "b_ms": round(med["b"], 3), "c_ms": round(med["c"], 3),
                                "d_ms": round(med["d"], 3), "spread_ms": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
                                "refined": count, "f": round(f, 5), "overhead_ms": round(med["d"] - med["a"], 3),
                                "c_over_b": round(med["c"] / med["b"], 4), "c_over_ideal": round(med["c"] / (med["a"] + f * med["b"]), 4)})
    nt.destroy()
    tex.destroy()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--samples", nargs="+", type=int, default=[2, 4], choices=(2, 4, 8))
    ap.add_argument("--cameras", nargs="+", default=["default", "path0"], choices=("default", "path0"))
    ap.add_argument("--arith", nargs="+", default=["strict", "fmad"], choices=("strict", "fmad", "fast"))
    ap.add_argument("--threshold", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--time", type=float, default=1.0)
    ap.add_argument("--path-time", type=float, default=5.0)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--camera", default="default", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args)
    common = ["--arith"] + args.arith + ["--samples"] + [str(s) for s in args.samples] + [
        "--threshold", str(args.threshold), "--reps", str(args.reps), "--warmup", str(args.warmup), "--spin", str(args.spin),
        "--time", str(args.time), "--path-time", str(args.path_time)]
    results, failed = [], None
    for cam in args.cameras:
        for size in args.sizes:
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", size,
                   "--camera", cam] + common
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                failed = {"size": size, "camera": cam, "exit": r.returncode, "stderr": r.stderr[-1500:]}
                break
            results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        if failed:
            break
    print(json.dumps({"tool": "adaptive_time", "spin": args.spin, "time": args.time, "path_time": args.path_time, "noise_table": True,
                      "reps": args.reps, "warmup": args.warmup, "results": results, "failed": failed}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
