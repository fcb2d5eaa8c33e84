#!/usr/bin/env python3
"""Cost of a motion-blurred frame against its K sub-frames rendered one launch each (HIP events, one JSON line).

    python tools/motion_blur_time.py [--width 1920 --height 1080] [--times 2 4 8] [--samples 1 2] [--arith strict fmad]
                                     [--no-noise-table] [--reps 5 --warmup 1] [--spin 0.9 --time 1.0 --shutter 0.5]

For every (K, s, arith mode) it times launch_raymarch_mb(w, h, s, K sub-frames) and K launch_raymarch_ss(w, h, s) at the same
times and cameras (the default view moving 1 unit per sub-frame along its right vector), alternately, and reports the medians and
their ratio.  The rays are the same; a difference is the blurred kernel's K-times-longer waves (their tail) or its loop.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--times", type=int, nargs="+", default=[2, 4, 8], choices=(1, 2, 4, 8, 16))
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 2], choices=(1, 2, 4, 8))
    ap.add_argument("--arith", nargs="+", default=["strict", "fmad"], choices=("strict", "fmad", "fast"))
    ap.add_argument("--no-noise-table", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--time", type=float, default=1.0)
    ap.add_argument("--shutter", type=float, default=0.5)
    args = ap.parse_args()

    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    w, h = args.width, args.height
    tex = rrt.SkyTexture(synthetic_sky())
    nt = None if args.no_noise_table else rrt.NoiseTable(max(4.0, args.time + 1.0))
    fx = rrt.CameraEffects()
    base = rrt.CameraState.default()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = []
    out_mb = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    out_ss = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    for n in args.times:
        # sub-frames spread over the trailing shutter interval of a 24 fps frame at args.time, the camera moving with them
        times = [args.time - args.shutter / 24.0 * ((n - m) - 0.5) / n for m in range(n)]
        cams = [rrt.CameraState([base.pos[i] + float(m) * base.right[i] for i in range(3)], list(base.forward), list(base.right),
                                list(base.up)) for m in range(n)]
        for s in args.samples:
            for arith in args.arith:
                prm = rrt.RenderParams(spin=args.spin, arith_mode={"strict": 0, "fast": 1, "fmad": 2}[arith], noise_table=nt.id if nt else 0)

                def mb():
                    rrt.launch_raymarch_mb(out_mb, w, h, s, times, cams, tex, fx, prm)

                def sep():
                    for t, c in zip(times, cams):
                        rrt.launch_raymarch_ss(out_ss, w, h, s, t, c, tex, fx, prm)

                for _ in range(args.warmup):
                    timed(mb)
                    timed(sep)
                t_mb, t_sep = [], []
                for _ in range(args.reps):               # alternately: clock and thermal drift fall on both alike
                    t_mb.append(timed(mb))
                    t_sep.append(timed(sep))
                m_mb, m_sep = statistics.median(t_mb), statistics.median(t_sep)
                results.append({"n_times": n, "samples": s, "arith": arith, "mb_ms": round(m_mb, 3), "separate_ss_ms": round(m_sep, 3),
                                "ratio": round(m_mb / m_sep, 4), "mb_ms_min": round(min(t_mb), 3), "separate_ss_ms_min": round(min(t_sep), 3),
                                "Mrays_per_s": round(n * s * s * w * h / m_mb / 1e3, 1)})
    print(json.dumps({"tool": "motion_blur_time", "width": w, "height": h, "spin": args.spin, "time": args.time, "shutter": args.shutter,
                      "noise_table": nt is not None, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                      "results": results}), flush=True)
    if nt:
        nt.destroy()
    tex.destroy()


if __name__ == "__main__":
    main()
