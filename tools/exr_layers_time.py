#!/usr/bin/env python3
"""Cost of the EXR data layers (include/rrt_exr.h, the second block comment): HIP events and the drivers' own clocks, one JSON line.

    python tools/exr_layers_time.py [--sizes 1920x1080 3840x2160] [--reps 30 --warmup 5 --runs 2] [--frames 6] [--out profiles/exr_layers_time.json]

From one debug launch of the default view (a = 0.9, volumetrics) at 1920x1080, tiled at the larger sizes -- the pass does the same
work per pixel whatever the picture --, per size, alternating within a run:

  (a) `bgr`: the {B, G, R} layer set through rrt_launch_exr_layers against rrt_launch_exr_from_hdr on the same HDR plane, for half/none,
      half/zip and float/zip.  `slower_than_spread`: the generic kernel's median exceeds the dedicated one's by more than the spread
      between the generic kernel's own two run medians.
  (b) `all`: the standard set of 15 channels (half beauty, zip and none): the pack, the bytes it reads and writes per second, and pack +
      the payload's pinned device-to-host copy against the pinned copies of the six source planes the payload replaces.
  (c) `driver`: per-frame time of the C++ headless driver over --frames frames with `--exr f.%04d.exr --exr-layers all` against plain
      `--exr`, same session, files written to a temporary directory (--no-noise-table; zip, level 4).  The debug kernel is compiled
      for fewer waves per SIMD than the frame kernel, so this ratio is not one of pack times.

`runs` runs of `reps` launches each after `warmup`; per-run medians and their median.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LAYERS = ("steps", "horizon", "transmittance", "emission", "direction", "position")
SHAPES = {"hdr": ("float32", 4), "rad": ("float32", 4), "pos": ("float32", 3), "vel": ("float32", 3), "steps": ("int32", 1), "hit": ("int32", 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--frames", type=int, default=6, help="frames of each driver run of (c); 0 skips it")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import build, headless
    from relativisticraytracer_amd.sky import synthetic_sky
    assert torch.cuda.is_available(), "needs a GPU"
    tex = rrt.SkyTexture(synthetic_sky())
    bw, bh = 1920, 1080
    base = {k: torch.zeros(bh * bw * n, dtype=getattr(torch, d), device="cuda") for k, (d, n) in SHAPES.items()}
    rrt.launch_raymarch_debug(torch.empty(bh * bw * 4, dtype=torch.uint8, device="cuda"), bw, bh, 1.0, rrt.CameraState.default(), tex,
                              rrt.CameraEffects(), rrt.RenderParams(spin=0.9, volumetrics=1), **base)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(fn):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def tiled(key, w, h):
        n = SHAPES[key][1]
        return base[key].view(bh, bw, n).repeat((h + bh - 1) // bh, (w + bw - 1) // bw, 1)[:h, :w].contiguous().view(-1)

    def measure(arms):
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
        return {k: statistics.median(v) for k, v in medians.items()}, medians

    bgr, all_rows, driver = [], [], []
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        planes = {k: tiled(k, w, h) for k in SHAPES}
        # (a) the generic kernel on the dedicated kernel's job
        for type_, compression in (("half", "none"), ("half", "zip"), ("float", "zip")):
            fmt = rrt.ExrFormat(type_, compression)
            L = rrt.ExrLayers(fmt, w, h, headless.exr_layer_list((), type_, planes["hdr"], planes))
            n = rrt.exr_frame_bytes(fmt, w, h)
            assert n == rrt.exr_layers_frame_bytes(L)
            out_a, out_b = (torch.empty(n, dtype=torch.uint8, device="cuda") for _ in range(2))
            med, runs = measure({"layers": lambda: rrt.launch_exr_layers(out_a, L), "dedicated": lambda: rrt.launch_exr_from_hdr(out_b, planes["hdr"], w, h, fmt)})
            assert torch.equal(out_a, out_b), "the {B, G, R} layer set is the dedicated launch's payload"
            spread = max(runs["layers"]) - min(runs["layers"])
            bgr.append({"width": w, "height": h, "type": type_, "compression": compression, "bytes_read": w * h * 16, "bytes_written": n,
                        "layers_ms": round(med["layers"], 4), "dedicated_ms": round(med["dedicated"], 4),
                        "layers_ms_run_medians": [round(m, 4) for m in runs["layers"]], "dedicated_ms_run_medians": [round(m, 4) for m in runs["dedicated"]],
                        "layers_over_dedicated": round(med["layers"] / med["dedicated"], 3),
                        "slower_than_spread": bool(med["layers"] - med["dedicated"] > spread),
                        "geometry": rrt.exr_layers_launch_geometry(L, L.address_bits(out_a))})
            del out_a, out_b
        # (b) the whole standard set
        hosts = {k: torch.empty(v.numel(), dtype=v.dtype, pin_memory=True) for k, v in planes.items()}
        in_bytes = sum(v.numel() * 4 for v in planes.values())
        for compression in ("zip", "none"):
            fmt = rrt.ExrFormat("half", compression)
            L = rrt.ExrLayers(fmt, w, h, headless.exr_layer_list(LAYERS, "half", planes["hdr"], planes))
            n = rrt.exr_layers_frame_bytes(L)
            payload = torch.empty(n, dtype=torch.uint8, device="cuda")
            payload_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)

            def planes_d2h():
                for k, v in planes.items():
                    hosts[k].copy_(v, non_blocking=True)
            med, runs = measure({"pack": lambda: rrt.launch_exr_layers(payload, L), "payload_d2h": lambda: payload_host.copy_(payload, non_blocking=True),
                                 "planes_d2h": planes_d2h})
            all_rows.append({"width": w, "height": h, "beauty": "half", "compression": compression, "channels": L.n_channels, "sources": L.n_sources,
                             "bytes_read": in_bytes, "bytes_written": n, **{k + "_ms": round(v, 4) for k, v in med.items()},
                             **{k + "_ms_run_medians": [round(m, 4) for m in v] for k, v in runs.items()},
                             "pack_GBps": round((in_bytes + n) / med["pack"] / 1e6, 1),
                             "pack_plus_payload_d2h_ms": round(med["pack"] + med["payload_d2h"], 4),
                             "pack_plus_payload_d2h_over_planes_d2h": round((med["pack"] + med["payload_d2h"]) / med["planes_d2h"], 3),
                             "geometry": rrt.exr_layers_launch_geometry(L, L.address_bits(payload))})
            del payload, payload_host
        del planes, hosts
        torch.cuda.empty_cache()
        # (c) the driver, frame by frame
        if args.frames > 0:
            exe = build.build_headless()
            row = {"width": w, "height": h, "frames": args.frames}
            for tag, extra in (("layers", ["--exr-layers", "all"]), ("plain", []), ("layers_again", ["--exr-layers", "all"]), ("plain_again", [])):
                with tempfile.TemporaryDirectory() as d:        # a run's files go when it is done
                    r = subprocess.run([exe, "--width", str(w), "--height", str(h), "--frames", str(args.frames), "--spin", "0.9", "--path", "0",
                                        "--no-noise-table", "--exr", os.path.join(d, tag + ".%04d.exr")] + extra, capture_output=True, text=True, timeout=900)
                    assert r.returncode == 0, r.stderr[-2000:]
                    row[tag + "_ms_per_frame"] = round(json.loads(r.stdout.strip().splitlines()[-1])["seconds"] * 1e3 / args.frames, 3)
                    row[tag + "_file_bytes"] = os.path.getsize(os.path.join(d, tag + ".0001.exr"))
            row["layers_over_plain"] = round(statistics.median([row["layers_ms_per_frame"], row["layers_again_ms_per_frame"]])
                                             / statistics.median([row["plain_ms_per_frame"], row["plain_again_ms_per_frame"]]), 3)
            driver.append(row)
    doc = {"tool": "exr_layers_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup, "bgr": bgr, "all": all_rows, "driver": driver}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
