#!/usr/bin/env python3
"""Cost of the Y'CbCr packing (include/rrt_yuv.h) next to the copies it replaces and to a plain copy (HIP events, one JSON line).

    python tools/yuv_time.py [--sizes 1920x1080 3840x2160 7680x4320] [--reps 30 --warmup 5 --runs 2] [--out profiles/yuv_time.json]

For every size, 4:2:0 and 4:4:4, 8 and 10 bits, from the RGBA8 frame and from its linear HDR (the rendered default view, a = 0.9, at
1920x1080 and a tiling of it at the larger sizes: the pass does the same work per pixel whatever the picture), it times, alternating
within a run:

    convert    rrt_launch_yuv_from_rgba8 / rrt_launch_yuv_from_hdr, limited range
    yuv_d2h    the packed frame's device-to-host copy into pinned memory            (what a --y4m frame costs after the kernel)
    rgba_d2h   the RGBA8 frame's device-to-host copy into pinned memory             (what --out costs per frame: the path --y4m replaces)
    d2d        a device-to-device copy_ of (bytes read + bytes written) / 2 bytes   (yardstick: the same traffic, done by a copy)

`runs` runs of `reps` launches each after `warmup`; per-run medians and their median.  The claim this file is there to check, in the
record as `claim_4k_420_8`: at 3840x2160, 4:2:0 8-bit from RGBA8, convert + yuv_d2h takes less time than rgba_d2h, in the same run.
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
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def tiled(base, w, h):
        t = base.view(bh, bw, 4).repeat((h + bh - 1) // bh, (w + bw - 1) // bw, 1)[:h, :w]
        return t.contiguous().view(-1)

    results, claim = [], None
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        rgba, hdr = tiled(base8, w, h), tiled(base_hdr, w, h)
        rgba_host = torch.empty(w * h * 4, dtype=torch.uint8, pin_memory=True)
        for chroma in (420, 444):
            for bits in (8, 10):
                fmt = rrt.YuvFormat(chroma, "limited", bits)
                n = rrt.yuv_frame_bytes(fmt, w, h)
                yuv = torch.empty(n, dtype=torch.uint8, device="cuda")
                yuv_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
                for source, src, launch, in_bytes in (("rgba8", rgba, rrt.launch_yuv_from_rgba8, w * h * 4),
                                                      ("hdr", hdr, rrt.launch_yuv_from_hdr, w * h * 16)):
                    half = (in_bytes + n) // 2
                    a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                    arms = {"convert": lambda: launch(yuv, src, w, h, fmt),
                            "yuv_d2h": lambda: yuv_host.copy_(yuv, non_blocking=True),
                            "rgba_d2h": lambda: rgba_host.copy_(rgba, non_blocking=True),
                            "d2d": lambda: b.copy_(a)}
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
                    row = {"width": w, "height": h, "chroma": chroma, "bits": bits, "source": source,
                           "wide_path": rrt.yuv_launch_geometry(fmt, w, h)["wide"], "bytes_read": in_bytes, "bytes_written": n,
                           **{k + "_ms": round(med[k], 4) for k in arms},
                           **{k + "_ms_run_medians": [round(m, 4) for m in medians[k]] for k in arms},
                           "convert_GBps": round((in_bytes + n) / med["convert"] / 1e6, 1),
                           "convert_over_d2d": round(med["convert"] / med["d2d"], 3),
                           "convert_plus_yuv_d2h_ms": round(med["convert"] + med["yuv_d2h"], 4)}
                    results.append(row)
                    if (w, h, chroma, bits, source) == (3840, 2160, 420, 8, "rgba8"):
                        claim = {"convert_plus_yuv_d2h_ms": row["convert_plus_yuv_d2h_ms"], "rgba_d2h_ms": row["rgba_d2h_ms"],
                                 "holds": bool(med["convert"] + med["yuv_d2h"] < med["rgba_d2h"])}
                    del a, b
        del rgba, hdr, rgba_host
    doc = {"tool": "yuv_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup, "claim_4k_420_8": claim, "results": results}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
