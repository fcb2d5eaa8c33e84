#!/usr/bin/env python3
"""Cost of a supersampled frame against the 1x frame of the same ray count (HIP events, one JSON line).

    python tools/supersample_time.py [--width 1920 --height 1080] [--samples 2 4] [--arith strict fmad] [--no-noise-table]
                                     [--reps 7 --warmup 2] [--spin 0.9 --time 1.0]

For every (s, arith mode) it times launch_raymarch_ss(w, h, s) and launch_raymarch at (s w) x (s h) -- the same rays in the same
wave tiles, single kernel, static order -- alternately, on the reference's default view, and reports the medians and their ratio.
The two should cost the same: a supersampled wave is a wave of the big frame plus a few lane shuffles after its march.
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
    ap.add_argument("--samples", type=int, nargs="+", default=[2, 4], choices=(1, 2, 4, 8))
    ap.add_argument("--arith", nargs="+", default=["strict", "fmad"], choices=("strict", "fmad", "fast"))
    ap.add_argument("--no-noise-table", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--spin", type=float, default=0.9)
    ap.add_argument("--time", type=float, default=1.0)
    args = ap.parse_args()

    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    w, h = args.width, args.height
    tex = rrt.SkyTexture(synthetic_sky())
    nt = None if args.no_noise_table else rrt.NoiseTable(max(4.0, args.time + 1.0))
    cam, fx = rrt.CameraState.default(), rrt.CameraEffects()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for s in args.samples:
        W, H = s * w, s * h
        out_ss = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
        out_1x = torch.empty(H * W * 4, dtype=torch.uint8, device="cuda")
        for arith in args.arith:
            prm = rrt.RenderParams(spin=args.spin, arith_mode={"strict": 0, "fast": 1, "fmad": 2}[arith], noise_table=nt.id if nt else 0)
            ss = lambda: rrt.launch_raymarch_ss(out_ss, w, h, s, args.time, cam, tex, fx, prm)
            one = lambda: rrt.launch_raymarch(out_1x, W, H, args.time, cam, tex, fx, prm)
            for _ in range(args.warmup):
                timed(ss)
                timed(one)
            t_ss, t_1x = [], []
            for _ in range(args.reps):               # alternately: clock and thermal drift fall on both alike
                t_ss.append(timed(ss))
                t_1x.append(timed(one))
            m_ss, m_1x = statistics.median(t_ss), statistics.median(t_1x)
            results.append({"samples": s, "arith": arith, "ss_ms": round(m_ss, 3), "same_rays_1x_ms": round(m_1x, 3),
                            "ratio": round(m_ss / m_1x, 4), "ss_ms_min": round(min(t_ss), 3), "same_rays_1x_ms_min": round(min(t_1x), 3),
                            "virtual_frame": f"{W}x{H}", "Mrays_per_s": round(W * H / m_ss / 1e3, 1)})
        del out_ss, out_1x
    print(json.dumps({"tool": "supersample_time", "width": w, "height": h, "spin": args.spin, "time": args.time,
                      "noise_table": nt is not None, "reps": args.reps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                      "results": results}), flush=True)
    if nt:
        nt.destroy()
    tex.destroy()


if __name__ == "__main__":
    main()
