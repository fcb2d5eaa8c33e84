#!/usr/bin/env python3
"""Cost of the HDR glow pass (rrt_launch_glow) next to the frame it decorates (HIP events, one JSON line).

    python tools/glow_time.py [--sizes 1920x1080:2 3840x2160:1] [--reps 30 --warmup 5 --runs 2] [--frame-reps 3]
                              [--radius 0.004 --lobes 4 --threshold 1.0 --intensity 0.25]

For every WxH:S it renders the default view (a = 0.9) supersampled S x S with its linear HDR, then times the glow alone on that
HDR (`runs` runs of `reps` launches each: per-run medians and their spread) and the supersampled frame itself.  It also reports
the glow's arithmetic: lane-operations = 2 passes x w x h x sum_l (2 R_l + 1) taps x 3 channels x 2 (multiply, add), and their
time at the FP32 VALU issue rate (256 CUs x 4 SIMDs x 32 lanes per clock x 2.4 GHz = 78.6 T lane-ops/s) as a share of the
measured median.  Kernel times: run it under `rocprofv3 --kernel-trace --stats` (tools/time_passes.sh) in a separate run.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

VALU_LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080:2", "3840x2160:1"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--frame-reps", type=int, default=3)
    ap.add_argument("--radius", type=float, default=0.004)
    ap.add_argument("--lobes", type=int, default=4)
    ap.add_argument("--threshold", type=float, default=1.0)
    ap.add_argument("--intensity", type=float, default=0.25)
    args = ap.parse_args()

    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    tex = rrt.SkyTexture(synthetic_sky())
    fx = rrt.CameraEffects()
    prm = rrt.RenderParams(spin=0.9)
    cam = rrt.CameraState.default()
    g = rrt.GlowSettings(radius=args.radius, lobes=args.lobes, threshold=args.threshold, intensity=args.intensity)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for spec in args.sizes:
        size, s = spec.split(":")
        w, h = (int(v) for v in size.split("x"))
        s = int(s)
        out = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
        hdr = torch.empty(h * w * 4, dtype=torch.float32, device="cuda")
        scratch = torch.empty(rrt.glow_scratch_bytes(w, h, g), dtype=torch.uint8, device="cuda")
        frame = lambda: rrt.launch_raymarch_ss(out, w, h, s, 1.0, cam, tex, fx, prm, hdr=hdr)
        frame_ms = [timed(frame) for _ in range(1 + args.frame_reps)][1:]
        run = lambda: rrt.launch_glow(out, hdr, w, h, g, scratch)
        for _ in range(args.warmup):
            run()
        medians = []
        for _ in range(args.runs):
            medians.append(statistics.median(timed(run) for _ in range(args.reps)))
        radii = [(rrt.glow_weights(g, h, l).size - 1) // 2 for l in range(g.lobes)]
        taps = sum(2 * r + 1 for r in radii)
        lane_ops = 2 * w * h * taps * 3 * 2
        bound_ms = lane_ops / VALU_LANE_OPS_PER_S * 1e3
        med = statistics.median(medians)
        results.append({"width": w, "height": h, "samples": s, "radii": radii, "taps_per_direction": taps,
                        "glow_ms_run_medians": [round(m, 4) for m in medians], "glow_ms": round(med, 4),
                        "glow_spread_ms": round(max(medians) - min(medians), 4),
                        "frame_ms_median": round(statistics.median(frame_ms), 3), "glow_share_of_frame": round(med / statistics.median(frame_ms), 4),
                        "lane_ops": lane_ops, "valu_bound_ms": round(bound_ms, 4), "valu_bound_share": round(bound_ms / med, 3),
                        "scratch_bytes": scratch.numel()})
    print(json.dumps({"tool": "glow_time", "glow": g.info(), "results": results}), flush=True)
    tex.destroy()


if __name__ == "__main__":
    main()
