#!/usr/bin/env python3
"""Cost of the EXR packing (include/rrt_exr.h) next to the copy it replaces (HIP events and a host clock, one JSON line).

    python tools/exr_time.py [--sizes 1920x1080 3840x2160] [--reps 30 --warmup 5 --runs 2] [--deflate-reps 3] [--out profiles/exr_time.json]

For every size and for half/none, half/zip and float/zip, from the frame's linear HDR (the rendered default view, a = 0.9, at
1920x1080 and a tiling of it at the larger sizes: the pass does the same work per pixel whatever the picture), it times, alternating
within a run:

    pack         rrt_launch_exr_from_hdr
    payload_d2h  the payload's device-to-host copy into pinned memory            (what an --exr frame costs after the kernel)
    hdr_d2h      the float4 HDR plane's device-to-host copy into pinned memory   (the only other way to get the frame out: 16 B / pixel)
    d2d          a device-to-device copy_ of (bytes read + bytes written) / 2 bytes   (yardstick: the same traffic, done by a copy)

and, on the host clock, `deflate`: one frame's chunks through EXRSink's thread pool (zlib level 4, the pool's default size; raw
fall-back included, no file written), the median of --deflate-reps.  `runs` runs of `reps` launches each after `warmup`; per-run
medians and their median.  The claim this file is there to check, per size, in the record as `claims`: pack + payload_d2h takes
less time than hdr_d2h in the same run -- 6 (half) against 16 bytes per pixel over PCIe.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

FORMATS = (("half", "none"), ("half", "zip"), ("float", "zip"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--deflate-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import sinks
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

    results, claims = [], []
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        hdr = tiled(base_hdr, w, h)
        hdr_host = torch.empty(w * h * 4, dtype=torch.float32, pin_memory=True)
        in_bytes = w * h * 16
        for fmt_names in FORMATS:
            fmt = rrt.ExrFormat(*fmt_names)
            n = rrt.exr_frame_bytes(fmt, w, h)
            payload = torch.empty(n, dtype=torch.uint8, device="cuda")
            payload_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            half = (in_bytes + n) // 2
            a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            arms = {"pack": lambda: rrt.launch_exr_from_hdr(payload, hdr, w, h, fmt),
                    "payload_d2h": lambda: payload_host.copy_(payload, non_blocking=True),
                    "hdr_d2h": lambda: hdr_host.copy_(hdr, non_blocking=True),
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
            row = {"width": w, "height": h, "type": fmt_names[0], "compression": fmt_names[1],
                   "geometry": rrt.exr_launch_geometry(fmt, w, h, payload.data_ptr() | hdr.data_ptr()), "bytes_read": in_bytes, "bytes_written": n,
                   **{k + "_ms": round(med[k], 4) for k in arms},
                   **{k + "_ms_run_medians": [round(m, 4) for m in medians[k]] for k in arms},
                   "pack_GBps": round((in_bytes + n) / med["pack"] / 1e6, 1),
                   "pack_over_d2d": round(med["pack"] / med["d2d"], 3),
                   "pack_plus_payload_d2h_ms": round(med["pack"] + med["payload_d2h"], 4),
                   "pack_plus_payload_d2h_over_hdr_d2h": round((med["pack"] + med["payload_d2h"]) / med["hdr_d2h"], 3)}
            if fmt_names[1] != "none":              # the host's share: deflate of the frame just copied, at the sink's pool size
                sink = sinks.EXRSink("unused.%d.exr", w, h, 24, fmt)
                torch.cuda.synchronize()
                data = memoryview(payload_host.numpy()).cast("B")
                pieces = [data[off:off + k] for _, off, k in sink.chunks]
                secs, out_bytes = [], 0
                for _ in range(args.deflate_reps):
                    t0 = time.perf_counter()
                    done = list(sink.pool.map(sink._chunk, pieces)) if sink.pool is not None else [sink._chunk(p) for p in pieces]
                    secs.append(time.perf_counter() - t0)
                    out_bytes = sum(len(p) for p in done)
                row.update({"deflate_ms": round(statistics.median(secs) * 1e3, 2), "deflate_threads": sink.threads, "deflate_level": sink.level,
                            "deflated_bytes": out_bytes, "chunks": len(pieces)})
                sink.close()
            results.append(row)
            claims.append({"width": w, "height": h, "type": fmt_names[0], "compression": fmt_names[1],
                           "pack_plus_payload_d2h_ms": row["pack_plus_payload_d2h_ms"], "hdr_d2h_ms": row["hdr_d2h_ms"],
                           "ratio": row["pack_plus_payload_d2h_over_hdr_d2h"], "holds": bool(med["pack"] + med["payload_d2h"] < med["hdr_d2h"])})
            del a, b, payload, payload_host
        del hdr, hdr_host
    doc = {"tool": "exr_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup, "deflate_reps": args.deflate_reps,
           "claims": claims, "results": results}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
