#!/usr/bin/env python3
"""Cost of the HDR10 packing (include/rrt_yuv.h, "HDR10 output") next to the SDR packing of the same HDR frame, a plain copy of the
same traffic and the pinned copy of the planes that follows it (HIP events, one JSON line).

    python tools/hdr10_time.py [--sizes 1920x1080 3840x2160 7680x4320] [--reps 30 --warmup 5 --runs 2] [--out profiles/hdr10_time.json]

For every size, 4:2:0 limited range, 10 bits, from the linear HDR of the rendered default view (a = 0.9, at 1920x1080 and a tiling of it
at the larger sizes, scaled by 4 so that the shoulder is exercised), it times, alternating within a run:

    hdr10        rrt_launch_yuv_hdr10_from_hdr, d_light NULL: one kernel
    hdr10_meter  the same with a light-level state: the pack kernel's reduction and atomics, and the one-thread fold kernel
    sdr          rrt_launch_yuv_from_hdr, 10 bits                                   (the nearest equivalent: the same loads and stores)
    d2d          a device-to-device copy_ of (bytes read + bytes written) / 2 bytes   (yardstick: the same traffic, done by a copy)
    yuv_d2h      the packed frame's device-to-host copy into pinned memory            (what follows the launch in a driver)

`runs` runs of `reps` launches each after `warmup`; per-run medians and their median.  The buffers are reused from launch to launch: at
1920x1080 the input (33 MB) and the planes (6 MB) fit the 256 MB last-level cache, at 7680x4320 (531 MB) they do not; which level
served them was not measured.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160", "7680x4320"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    tex = rrt.SkyTexture(synthetic_sky())
    bw, bh = 1920, 1080
    base8 = torch.empty(bh * bw * 4, dtype=torch.uint8, device="cuda")
    base_hdr = torch.empty(bh * bw * 4, dtype=torch.float32, device="cuda")
    rrt.launch_raymarch_ss(base8, bw, bh, 1, 1.0, rrt.CameraState.default(), tex, rrt.CameraEffects(), rrt.RenderParams(spin=0.9), hdr=base_hdr)
    base_hdr *= 4.0
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    fmt, settings = rrt.YuvFormat(420, "limited", 10), rrt.Hdr10Settings()
    light = torch.zeros(rrt.yuv_hdr10_light_bytes(), dtype=torch.uint8, device="cuda")
    results = []
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        hdr = base_hdr.view(bh, bw, 4).repeat((h + bh - 1) // bh, (w + bw - 1) // bw, 1)[:h, :w].contiguous().view(-1)
        n, in_bytes = rrt.yuv_frame_bytes(fmt, w, h), w * h * 16
        yuv = torch.empty(n, dtype=torch.uint8, device="cuda")
        yuv_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
        half = (in_bytes + n) // 2
        a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        arms = {"hdr10": lambda: rrt.launch_yuv_hdr10_from_hdr(yuv, hdr, w, h, fmt, settings, None),
                "hdr10_meter": lambda: rrt.launch_yuv_hdr10_from_hdr(yuv, hdr, w, h, fmt, settings, light),
                "sdr": lambda: rrt.launch_yuv_from_hdr(yuv, hdr, w, h, fmt),
                "d2d": lambda: b.copy_(a),
                "yuv_d2h": lambda: yuv_host.copy_(yuv, non_blocking=True)}
        rrt.launch_yuv_hdr10_light_reset(light)
        for _ in range(args.warmup):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        medians = {k: [] for k in arms}
        for _ in range(args.runs):
            ms = {k: [] for k in arms}
            for _ in range(args.reps):          # alternating: the arms see the same clocks and neighbours
                for k, fn in arms.items():
                    ms[k].append(timed(fn))
            for k in arms:
                medians[k].append(statistics.median(ms[k]))
        med = {k: statistics.median(v) for k, v in medians.items()}
        levels = rrt.yuv_hdr10_light_levels(light.cpu().numpy(), w, h)
        results.append({"width": w, "height": h, "chroma": 420, "bits": 10, "wide_path": rrt.yuv_launch_geometry(fmt, w, h)["wide"],
                        "bytes_read": in_bytes, "bytes_written": n,
                        **{k + "_ms": round(med[k], 4) for k in arms},
                        **{k + "_ms_run_medians": [round(m, 4) for m in medians[k]] for k in arms},
                        "hdr10_GBps": round((in_bytes + n) / med["hdr10"] / 1e6, 1),
                        "hdr10_over_sdr": round(med["hdr10"] / med["sdr"], 3),
                        "hdr10_over_d2d": round(med["hdr10"] / med["d2d"], 3),
                        "meter_over_no_meter": round(med["hdr10_meter"] / med["hdr10"], 3),
                        "meter_cost_ms": round(med["hdr10_meter"] - med["hdr10"], 4),
                        "metered_launch_costs_more_than_yuv_d2h": bool(med["hdr10_meter"] > med["yuv_d2h"]),
                        "levels": levels})
        del hdr, yuv, yuv_host, a, b
    doc = {"tool": "hdr10_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup,
           "memory_level": "not measured: the buffers are reused from launch to launch; at 1920x1080 they fit the last-level cache, at 7680x4320 they do not",
           "results": results}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
