#!/usr/bin/env python3
"""Cost of full-size stereo composites (launch_raymarch_stereo) next to the mono frame with the same rays (HIP events, one JSON line).

    python tools/stereo_time.py [--pairs tb-equirect:4096x2048 sbs-pinhole:1920x1080] [--cameras default path0]
                                [--arith strict fmad] [--reps 5 --warmup 1] [--spin 0.9 --time 1.0 --path-time 5.0]
                                [--base 1.0] [--convergence 12.0] [--step-timeout 600]

A pair LAYOUT-KIND:WxH is the stereo composite of two W x H eyes (tb = top-bottom, sbs = side-by-side; kind equirect = ODS with
--base, pinhole = off-axis with --base and --convergence) next to the mono frame of the composite's size and so the same ray count
(tb: W x 2H, sbs: 2W x H) through the launch the eyes are defined by (launch_raymarch_pano for equirect, launch_raymarch_ss at
s = 1 for pinhole).  Every (pair, camera, stereo | mono) is measured in a fresh child process (this script with --one) under
`timeout -k 10 <step-timeout>`; the first child that fails, faults or runs out of time ends the run (its exit status is reported,
nothing else is started).  A child renders with a noise table over the clock, strict and FMAD, `warmup` untimed launches then
`reps` timed ones, and reports the medians and Mrays/s; the parent adds stereo / mono ratios of the medians.  The mono frame of the
composite's size is not always the same picture: a 3840 x 1080 pinhole frame is a wider view than two 1920 x 1080 eyes, with less
of its area on the costly disk and shadow.  So a third frame, "eyes", times the mono frame of one eye's size twice (two launches,
the same views as the pair) and the parent adds stereo / eyes ratios too.  Cameras: default =
the reference's start-up view, path0 = path 0 ("Gargantua Fly-By") at --path-time.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def parse_pair(pair):
    """(layout, kind, w, h) of LAYOUT-KIND:WxH"""
    name, size = pair.split(":")
    layout, kind = name.split("-")
    w, h = (int(v) for v in size.split("x"))
    return {"tb": "top-bottom", "sbs": "side-by-side"}[layout], kind, w, h


def one(args):
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import camera_paths as cp
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    layout, kind, w, h = parse_pair(args.one)
    proj = rrt.Projection(kind)
    st = rrt.Stereo(layout, args.base, args.convergence if kind == "pinhole" else 0.0)
    cw, ch = st.composite(w, h)
    cam = rrt.CameraState.default() if args.camera == "default" else cp.CameraPath(0).camera_at(args.path_time)
    tex = rrt.SkyTexture(synthetic_sky())
    nt = rrt.NoiseTable(max(4.0, args.time + 1.0))
    fx = rrt.CameraEffects()
    out = torch.empty(ch * cw * 4, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rays = cw * ch
    res = {"pair": args.one, "camera": args.camera, "frame": args.frame, "rays": rays}
    for arith in args.arith:
        prm = rrt.RenderParams(spin=args.spin, arith_mode={"strict": 0, "fast": 1, "fmad": 2}[arith], noise_table=nt.id)
        mono = (lambda W, H, o=out: rrt.launch_raymarch_pano(o, W, H, 1, proj, args.time, cam, tex, fx, prm)) if kind == "equirect" \
            else (lambda W, H, o=out: rrt.launch_raymarch_ss(o, W, H, 1, args.time, cam, tex, fx, prm))
        if args.frame == "stereo":
            run = lambda: rrt.launch_raymarch_stereo(out, w, h, 1, proj, st, args.time, cam, tex, fx, prm)
        elif args.frame == "mono":
            run = lambda: mono(cw, ch)
        else:                                   # "eyes": the mono frame of one eye's size twice, i.e. the same views
            run = lambda: (mono(w, h), mono(w, h, out[w * h * 4:]))
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
    ap.add_argument("--pairs", nargs="+", default=["tb-equirect:4096x2048", "sbs-pinhole:1920x1080"])
    ap.add_argument("--cameras", nargs="+", default=["default", "path0"], choices=("default", "path0"))
    ap.add_argument("--arith", nargs="+", default=["strict", "fmad"], choices=("strict", "fmad", "fast"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--time", type=float, default=1.0)
    ap.add_argument("--path-time", type=float, default=5.0)
    ap.add_argument("--base", type=float, default=1.0)
    ap.add_argument("--convergence", type=float, default=12.0)
    ap.add_argument("--step-timeout", type=int, default=600)
    ap.add_argument("--one", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--camera", default="default", help=argparse.SUPPRESS)
    ap.add_argument("--frame", default="stereo", choices=("stereo", "mono", "eyes"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.one:
        return one(args)
    common = ["--arith"] + args.arith + ["--reps", str(args.reps), "--warmup", str(args.warmup), "--spin", str(args.spin),
                                         "--time", str(args.time), "--path-time", str(args.path_time), "--base", str(args.base),
                                         "--convergence", str(args.convergence)]
    results, failed = [], None
    for cam in args.cameras:
        for pair in args.pairs:
            got = {}
            for frame in ("mono", "eyes", "stereo"):
                cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--one", pair,
                       "--camera", cam, "--frame", frame] + common
                r = subprocess.run(cmd, capture_output=True, text=True)
                if r.returncode != 0:
                    failed = {"pair": pair, "camera": cam, "frame": frame, "exit": r.returncode, "stderr": r.stderr[-1500:]}
                    break
                got[frame] = json.loads(r.stdout.strip().splitlines()[-1])
                results.append(got[frame])
            if failed:
                break
            results.append({"pair": pair, "camera": cam,
                            "ratio": {a: round(got["stereo"][a]["ms"] / got["mono"][a]["ms"], 4) for a in args.arith},
                            "ratio_to_eyes": {a: round(got["stereo"][a]["ms"] / got["eyes"][a]["ms"], 4) for a in args.arith}})
        if failed:
            break
    print(json.dumps({"tool": "stereo_time", "spin": args.spin, "time": args.time, "path_time": args.path_time, "noise_table": True,
                      "base": args.base, "convergence": args.convergence, "reps": args.reps, "warmup": args.warmup,
                      "results": results, "failed": failed}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
