#!/usr/bin/env python3
"""Cost of the exposure pass (rrt_launch_exposure) next to the glow and to a plain copy of the frame (HIP events, one JSON line).

    python tools/exposure_time.py [--sizes 1920x1080 3840x2160] [--reps 30 --warmup 5 --runs 2] [--out profiles/exposure_time.json]

For every size and each of three inputs -- the rendered default view (a = 0.9), a flat frame (every pixel in one bin: the meter's
one-add path) and a random-luma frame (log-uniform over the histogram's 32 octaves: the worst spread over the bins, every LDS add
its own) -- it times, alternating within a run:

    auto      rrt_launch_exposure in auto mode (zero + meter + resolve + apply), RGBA8 out
    manual    rrt_launch_exposure in manual mode (apply alone), RGBA8 out
    glow      rrt_launch_glow at its defaults on the same HDR            (yardstick: the auto launch must cost less)
    copy      a device-to-device copy of the frame's HDR, 16 B / pixel   (yardstick: what reading and writing the frame once costs)

`runs` runs of `reps` launches each after `warmup`; per-run medians, their median and spread, and the ratios auto / glow and
auto / copy.  The auto launch reads the HDR twice (meter, apply) and writes 4 B / pixel; the copy reads and writes 16 B / pixel.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import numpy as np
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    tex = rrt.SkyTexture(synthetic_sky())
    fx, prm, cam = rrt.CameraEffects(), rrt.RenderParams(spin=0.9), rrt.CameraState.default()
    g = rrt.GlowSettings()
    auto, manual = rrt.ExposureSettings(mode="auto"), rrt.ExposureSettings(ev=1.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        n = w * h
        out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
        copy_dst = torch.empty(n * 4, dtype=torch.float32, device="cuda")
        glow_scratch = torch.empty(rrt.glow_scratch_bytes(w, h, g), dtype=torch.uint8, device="cuda")
        scratch = torch.empty(rrt.exposure_scratch_bytes(), dtype=torch.uint8, device="cuda")
        rendered = torch.empty(n * 4, dtype=torch.float32, device="cuda")
        rrt.launch_raymarch_ss(out, w, h, 1, 1.0, cam, tex, fx, prm, hdr=rendered)
        flat = torch.tensor([0.3, 0.2, 0.1, 1.0], dtype=torch.float32, device="cuda").repeat(n)
        rng = np.random.default_rng(w)
        rnd = (2.0 ** rng.uniform(-16.0, 16.0, (n, 1)) * np.ones((1, 4))).astype(np.float32)
        random = torch.from_numpy(rnd.ravel()).cuda()
        for name, hdr in (("rendered", rendered), ("flat", flat), ("random", random)):
            rrt.launch_exposure_reset(scratch)
            arms = {"auto": lambda: rrt.launch_exposure(out, None, hdr, w, h, auto, scratch),
                    "manual": lambda: rrt.launch_exposure(out, None, hdr, w, h, manual),
                    "glow": lambda: rrt.launch_glow(out, hdr, w, h, g, glow_scratch),
                    "copy": lambda: copy_dst.copy_(hdr)}
            for _ in range(args.warmup):
                for fn in arms.values():
                    fn()
            medians = {k: [] for k in arms}
            for _ in range(args.runs):
                ms = {k: [] for k in arms}
                for _ in range(args.reps):          # alternating: the arms see the same clocks and neighbours
                    for k, fn in arms.items():
                        ms[k].append(timed(fn))
                for k in arms:
                    medians[k].append(statistics.median(ms[k]))
            torch.cuda.synchronize()
            state = scratch[rrt.EXPOSURE_STATE_OFFSET:rrt.EXPOSURE_STATE_OFFSET + 24].cpu().numpy()
            med = {k: statistics.median(v) for k, v in medians.items()}
            results.append({"width": w, "height": h, "input": name,
                            "metered_pixels": int(state[16:24].view(np.uint64)[0]), "ev": float(state[0:4].view(np.float32)[0]),
                            **{k + "_ms": round(med[k], 4) for k in arms},
                            **{k + "_ms_run_medians": [round(m, 4) for m in medians[k]] for k in arms},
                            "auto_over_glow": round(med["auto"] / med["glow"], 4), "auto_over_copy": round(med["auto"] / med["copy"], 3),
                            "manual_over_copy": round(med["manual"] / med["copy"], 3)})
    doc = {"tool": "exposure_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup, "glow": g.info(), "results": results}
    text = json.dumps(doc)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
