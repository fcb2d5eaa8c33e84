#!/usr/bin/env python3
"""Cost of depth-of-field frames (launch_raymarch_dof) next to the motion-blurred frame of the same samples (HIP events, one JSON line).

    python tools/dof_time.py [--sizes 1920x1080] [--k 4 8] [--samples 1 2] [--arith strict fmad] [--apertures 0.25 1.0]
                             [--reps 5 --warmup 1] [--spin 0.9 --time 1.0 --dt 0.01 --step 0.05] [--step-timeout 900]

Per size a fresh child process (this script with --one) under `timeout -k 10 <step-timeout>`; the first child that fails, faults or
runs out of time ends the run (its exit status is reported, nothing else is started).  A child renders the reference's start-up view
with a noise table over the clock; sample k is at time + k dt, its camera --step scene units further along `right`.  Per arithmetic
mode, K and s it measures the launches ALTERNATING -- a, b, c0, c1, a, b, ... -- `warmup` untimed rounds, then `reps` timed ones,
medians reported:
    a    launch_raymarch_mb                                   (code the depth of field does not touch: the baseline, in the same run)
    b    launch_raymarch_dof, every lens point (0, 0)         (the same rays as a: b / a is the new kernel's own cost)
    c_i  launch_raymarch_dof, lens_points(aperture_i, K)      (focused at the camera's distance to the origin: c / b is what the
                                                               less coherent wavefronts cost)
"""
import argparse
import json
import math
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
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    w, h = (int(v) for v in args.one.split("x"))
    base = rrt.CameraState.default().as_array()
    focus = float(np.float32(math.sqrt(sum(float(v) ** 2 for v in base[0]))))
    tex = rrt.SkyTexture(synthetic_sky())
    nt = rrt.NoiseTable(max(4.0, args.time + 16 * args.dt + 1.0))
    fx = rrt.CameraEffects()
    out = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    res = {"size": args.one, "pixels": w * h, "focus": focus, "apertures": args.apertures, "rows": []}
    for arith in args.arith:
        prm = rrt.RenderParams(spin=args.spin, arith_mode={"strict": 0, "fast": 1, "fmad": 2}[arith], noise_table=nt.id)
        for K in args.k:
            times = [args.time + args.dt * k for k in range(K)]
            cams = [rrt.CameraState([base[0][i] + np.float32(args.step * k) * base[2][i] for i in range(3)], *base[1:]) for k in range(K)]
            zero = np.zeros((K, 2), np.float32)
            for s in args.samples:
                def dof(lens):
                    return lambda: rrt.launch_raymarch_dof(out, w, h, s, times, cams, lens, focus, tex, fx, prm)
                runs = {"a": lambda: rrt.launch_raymarch_mb(out, w, h, s, times, cams, tex, fx, prm), "b": dof(zero)}
                for i, ap in enumerate(args.apertures):
                    runs["c%d" % i] = dof(rrt.lens_points(ap, K))
                ms = {k: [] for k in runs}
                for rep in range(args.warmup + args.reps):
                    for k, run in runs.items():
                        e0.record()
                        run()
                        e1.record()
                        e1.synchronize()
                        if rep >= args.warmup:
                            ms[k].append(e0.elapsed_time(e1))
                med = {k: statistics.median(v) for k, v in ms.items()}
                row = {"arith": arith, "K": K, "s": s}
                row.update({k + "_ms": round(v, 3) for k, v in med.items()})
                row["spread_ms"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}
                row["b_over_a"] = round(med["b"] / med["a"], 4)
                row["c_over_b"] = [round(med["c%d" % i] / med["b"], 4) for i in range(len(args.apertures))]
                res["rows"].append(row)
    nt.destroy()
    tex.destroy()
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080"])
    ap.add_argument("--k", nargs="+", type=int, default=[4, 8], choices=(1, 2, 4, 8, 16))
    ap.add_argument("--samples", nargs="+", type=int, default=[1, 2], choices=(1, 2, 4, 8))
    ap.add_argument("--arith", nargs="+", default=["strict", "fmad"], choices=("strict", "fmad", "fast"))
    ap.add_argument("--apertures", nargs="+", type=float, default=[0.25, 1.0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--time", type=float, default=1.0)
    ap.add_argument("--dt", type=float, default=0.01)
    ap.add_argument("--step", type=float, default=0.05)
    ap.add_argument("--step-timeout", type=int, default=900)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args)
    common = ["--arith"] + args.arith + ["--k"] + [str(k) for k in args.k] + ["--samples"] + [str(s) for s in args.samples] + [
        "--apertures"] + [str(a) for a in args.apertures] + ["--reps", str(args.reps), "--warmup", str(args.warmup),
                                                             "--spin", str(args.spin), "--time", str(args.time), "--dt", str(args.dt),
                                                             "--step", str(args.step)]
    results, failed = [], None
    for size in args.sizes:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", size] + common
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            failed = {"size": size, "exit": r.returncode, "stderr": r.stderr[-1500:]}
            break
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps({"tool": "dof_time", "spin": args.spin, "time": args.time, "dt": args.dt, "step": args.step, "noise_table": True,
                      "reps": args.reps, "warmup": args.warmup, "results": results, "failed": failed}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
