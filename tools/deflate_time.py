#!/usr/bin/env python3
"""Cost of the device deflate (include/rrt_deflate.h) next to the host path it replaces (HIP events and a host clock, one JSON line).

    python tools/deflate_time.py [--sizes 1920x1080 3840x2160] [--reps 20 --warmup 3 --runs 2] [--host-reps 3] [--out profiles/deflate_time.json]

For every size and for depth 8 and depth 16, on the adaptive payload of the rendered default view (a = 0.9; at 1920x1080, a tiling of
it at the larger sizes), cut into PNGSink's slices, it times, alternating within a run:

    deflate        rrt_launch_deflate: its three kernels                                                        (a)
    deflate_d2h    the launch, the pinned copy of the sizes, a wait, the pinned copy of exactly the streams     (b)
    d2d            a device-to-device copy_ of the payload's bytes                                              (d)

and, on the host clock in the same run, the median of --host-reps of `host`: the pinned copy of the payload plus one frame's slices
through PNGSink's thread pool at level 4, Z_FILTERED (c) -- what `--png-deflate device` replaces; its two parts are listed as well.
Sizes: the device's streams, (c)'s, and zlib's at level 4, Z_RLE with a full flush at the device's cuts.  `runs` runs of `reps`
launches each after `warmup`; per-run medians and their median.  The streams are inflated once and compared with the payload."""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()

    import numpy as np
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

    results = []
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        for depth in (8, 16):
            fmt = rrt.PngFormat(depth, "adaptive")
            src = tiled(base8 if depth == 8 else base_hdr, w, h)
            n, stride, table = rrt.png_frame_bytes(fmt, w, h, layout=True)
            payload = torch.empty(n, dtype=torch.uint8, device="cuda")
            sums = torch.empty(table, dtype=torch.uint8, device="cuda")
            (rrt.launch_png_from_rgba8 if depth == 8 else rrt.launch_png_from_hdr)(payload, sums, src, w, h, fmt)
            del src
            sink = sinks.PNGSink("unused.%d.png", w, h, fmt)
            cut = sink.rows_per_slice * sink.stride
            plan = rrt.deflate_plan(n, cut)
            out = torch.empty(plan["out_bound"], dtype=torch.uint8, device="cuda")
            sizes = torch.empty(plan["streams"], dtype=torch.int32, device="cuda")
            scratch = torch.empty(plan["scratch_bytes"], dtype=torch.uint8, device="cuda")
            out_host = torch.empty(plan["out_bound"], dtype=torch.uint8, pin_memory=True)
            sizes_host = torch.empty(plan["streams"], dtype=torch.int32, pin_memory=True)
            payload_host = torch.empty(n, dtype=torch.uint8, pin_memory=True)
            other = torch.empty(n, dtype=torch.uint8, device="cuda")

            def deflate():
                rrt.launch_deflate(out, sizes, scratch, payload, n, cut, True)

            def deflate_d2h():
                deflate()
                sizes_host.copy_(sizes, non_blocking=False)
                total = int(sizes_host.sum())
                out_host[:total].copy_(out[:total], non_blocking=False)
                return total

            arms = {"deflate": deflate, "deflate_d2h": deflate_d2h, "d2d": lambda: other.copy_(payload)}
            for _ in range(args.warmup):
                for fn in arms.values():
                    fn()
            torch.cuda.synchronize()
            view = memoryview(payload_host.numpy()).cast("B")
            jobs = [(view[i * cut:(i + 1) * cut], i == sink.n_slices - 1) for i in range(sink.n_slices)]

            def host():
                t0 = time.perf_counter()
                payload_host.copy_(payload, non_blocking=False)
                t1 = time.perf_counter()
                pieces = list(sink.pool.map(sink._slice, jobs)) if sink.pool is not None else [sink._slice(j) for j in jobs]
                return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, sum(len(p) for p in pieces)

            medians = {k: [] for k in arms}
            host_ms = []
            for _ in range(args.runs):
                ms = {k: [] for k in arms}
                for i in range(args.reps):          # alternating: the arms see the same clocks and neighbours
                    for k, fn in arms.items():
                        ms[k].append(timed(fn))
                for k in ms:
                    medians[k].append(statistics.median(ms[k]))
                for _ in range(args.host_reps):     # the host path in the same run
                    host_ms.append(host())
            med = {k: statistics.median(v) for k, v in medians.items()}
            copy_ms, zlib_ms = statistics.median(v[0] for v in host_ms), statistics.median(v[1] for v in host_ms)
            host_total = statistics.median(v[0] + v[1] for v in host_ms)
            total = deflate_d2h()
            lens = sizes_host.numpy().astype(np.int64)
            data, raw, at = out_host.numpy(), payload_host.numpy().tobytes(), 0
            rle_bytes = 0
            for j, length in enumerate(lens.tolist()):          # every stream inflates to its slice; zlib's Z_RLE size at the same cuts
                z = zlib.decompressobj(-15)
                piece = raw[j * cut:(j + 1) * cut]
                assert z.decompress(data[at:at + length].tobytes()) == piece and z.eof == (j == len(lens) - 1)
                at += length
                c = zlib.compressobj(4, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
                for a in range(0, len(piece), 32768):
                    rle_bytes += len(c.compress(piece[a:a + 32768])) + len(c.flush(zlib.Z_FINISH if (j == len(lens) - 1 and a + 32768 >= len(piece)) else zlib.Z_FULL_FLUSH))
            results.append({"width": w, "height": h, "depth": depth, "payload_bytes": n, "slices": sink.n_slices, "segments": plan["segments"],
                            "geometry": rrt.deflate_launch_geometry(n, cut, payload.data_ptr()),
                            **{k + "_ms": round(med[k], 4) for k in medians},
                            **{k + "_ms_run_medians": [round(m, 4) for m in medians[k]] for k in medians},
                            "host_payload_d2h_ms": round(copy_ms, 3), "host_zlib_ms": round(zlib_ms, 3), "host_ms": round(host_total, 3),
                            "host_threads": sink.threads, "host_level": sink.level,
                            "deflate_GBps": round(n / med["deflate"] / 1e6, 1), "deflate_over_d2d": round(med["deflate"] / med["d2d"], 2),
                            "deflate_d2h_over_host": round(med["deflate_d2h"] / host_total, 3),
                            "device_bytes": int(total), "host_bytes": int(host_ms[-1][2]), "zlib_rle_bytes": int(rle_bytes),
                            "device_over_host_bytes": round(total / host_ms[-1][2], 4), "device_over_zlib_rle_bytes": round(total / rle_bytes, 4)})
            sink.close()
            del payload, sums, out, sizes, scratch, out_host, sizes_host, payload_host, other
    doc = {"tool": "deflate_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup, "host_reps": args.host_reps, "results": results}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
