#!/usr/bin/env python3
"""Cost of the PNG filtering (include/rrt_png.h) next to the copies it replaces and the host's share (HIP events and a host clock, one
JSON line).

    python tools/png_time.py [--sizes 1920x1080 3840x2160] [--reps 30 --warmup 5 --runs 2] [--host-reps 3] [--out profiles/png_time.json]

For every size, for depth 8 (from the RGBA8 frame) and depth 16 (from the linear HDR) and for the filters adaptive and up -- the
rendered default view, a = 0.9, at 1920x1080 and a tiling of it at the larger sizes --, it times, alternating within a run:

    filter       rrt_launch_png_from_rgba8 / _from_hdr, the wide path
    narrow       the same launch into a payload one byte off the 16-byte grid: the narrow path (a fifth of the launches)
    payload_d2h  the payload's and the row sums' device-to-host copy into pinned memory   (what a --png frame costs after the kernel)
    input_d2h    the RGBA8 frame's (depth 8) or the float4 plane's (depth 16) copy into pinned memory   (the copy it replaces)
    d2d          a device-to-device copy_ of (bytes read + bytes written) / 2 bytes   (yardstick: the same traffic, done by a copy)

and, on the host clock, the median of --host-reps: `deflate` -- one frame's slices through PNGSink's thread pool at level 4, with
zlib's default strategy and with Z_FILTERED, sizes included; once per size and depth `whole`: one zlib.compress of the whole payload at
the same level (what the independent slices cost in bytes), and `pil`: Image.save(compress_level=4) of the same frame on the host,
time and size -- what a user does today.  `runs` runs of `reps` launches each after `warmup`; per-run medians and their median.
"""
import argparse
import io
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

CASES = ((8, "adaptive"), (8, "up"), (16, "adaptive"), (16, "up"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "3840x2160"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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

    def host_median(fn):
        secs, out = [], None
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            out = fn()
            secs.append(time.perf_counter() - t0)
        return round(statistics.median(secs) * 1e3, 2), out

    try:
        from PIL import Image
    except ImportError:
        Image = None

    results = []
    for size in args.sizes:
        w, h = (int(v) for v in size.split("x"))
        sources = {8: tiled(base8, w, h), 16: tiled(base_hdr, w, h)}
        once = {}
        for depth, filter_name in CASES:
            fmt = rrt.PngFormat(depth, filter_name)
            src = sources[depth]
            launch = rrt.launch_png_from_rgba8 if depth == 8 else rrt.launch_png_from_hdr
            n, stride, table = rrt.png_frame_bytes(fmt, w, h, layout=True)
            at = (n + 15) & ~15
            out = torch.empty(at + table + 16, dtype=torch.uint8, device="cuda")
            out_host = torch.empty(at + table, dtype=torch.uint8, pin_memory=True)
            in_bytes = src.numel() * src.element_size()
            in_host = torch.empty(src.numel(), dtype=src.dtype, pin_memory=True)
            half = (in_bytes + n) // 2
            a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
            off = torch.empty(n + 32, dtype=torch.uint8, device="cuda")
            shifted = off[(-off.data_ptr()) % 16 + 1:]
            assert not rrt.png_launch_geometry(fmt, w, h, shifted.data_ptr() | src.data_ptr())["wide"]
            arms = {"filter": lambda: launch(out, out[at:], src, w, h, fmt),
                    "payload_d2h": lambda: out_host.copy_(out[:at + table], non_blocking=True),
                    "input_d2h": lambda: in_host.copy_(src, non_blocking=True),
                    "d2d": lambda: b.copy_(a)}
            narrow = lambda: launch(shifted, out[at:], src, w, h, fmt)      # noqa: E731
            for _ in range(args.warmup):
                for fn in arms.values():
                    fn()
            narrow()
            torch.cuda.synchronize()
            medians = {k: [] for k in list(arms) + ["narrow"]}
            for _ in range(args.runs):
                ms = {k: [] for k in medians}
                for i in range(args.reps):          # alternating: the arms see the same clocks and neighbours
                    for k, fn in arms.items():
                        ms[k].append(timed(fn))
                    if i % 5 == 0:
                        ms["narrow"].append(timed(narrow))
                for k in ms:
                    medians[k].append(statistics.median(ms[k]))
            med = {k: statistics.median(v) for k, v in medians.items()}
            launch(out, out[at:], src, w, h, fmt)
            out_host.copy_(out[:at + table])
            torch.cuda.synchronize()
            data = out_host.numpy()
            payload, sums = data[:n], data[at:at + table].view(np.uint32)
            assert rrt.png_adler32(sums, fmt, w, h) == zlib.adler32(payload)
            row = {"width": w, "height": h, "depth": depth, "filter": filter_name,
                   "geometry": rrt.png_launch_geometry(fmt, w, h, out.data_ptr() | src.data_ptr()), "bytes_read": in_bytes, "bytes_written": n,
                   **{k + "_ms": round(med[k], 4) for k in medians},
                   **{k + "_ms_run_medians": [round(m, 4) for m in medians[k]] for k in medians},
                   "filter_GBps": round((in_bytes + n) / med["filter"] / 1e6, 1),
                   "filter_over_d2d": round(med["filter"] / med["d2d"], 3),
                   "narrow_over_filter": round(med["narrow"] / med["filter"], 2),
                   "filter_plus_payload_d2h_ms": round(med["filter"] + med["payload_d2h"], 4),
                   "filter_plus_payload_d2h_over_input_d2h": round((med["filter"] + med["payload_d2h"]) / med["input_d2h"], 3),
                   "types": np.bincount(payload.reshape(h, stride)[:, 0], minlength=5).tolist()}
            sink = sinks.PNGSink("unused.%d.png", w, h, fmt)
            view = memoryview(payload).cast("B")
            step = sink.rows_per_slice * sink.stride
            jobs = [(view[i * step:(i + 1) * step], i == sink.n_slices - 1) for i in range(sink.n_slices)]
            for name, strategy in (("default", zlib.Z_DEFAULT_STRATEGY), ("filtered", zlib.Z_FILTERED)):
                sink.STRATEGY = strategy
                ms, pieces = host_median(lambda: list(sink.pool.map(sink._slice, jobs)) if sink.pool is not None else [sink._slice(j) for j in jobs])
                row.update({f"deflate_{name}_ms": ms, f"deflate_{name}_bytes": sum(len(p) for p in pieces)})
            row.update({"deflate_threads": sink.threads, "deflate_level": sink.level, "slices": sink.n_slices})
            sink.close()
            t0 = time.perf_counter()
            row["whole_stream_bytes"] = len(zlib.compress(view, 4))
            row["whole_stream_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            row["sliced_over_whole"] = round(row["deflate_default_bytes"] / row["whole_stream_bytes"], 4)
            if Image is not None and depth == 8:      # what a user does today: the RGBA8 frame to the host, PIL filters and deflates on one core
                if depth not in once:
                    frame = sources[8].cpu().numpy().reshape(h, w, 4)[::-1, :, :3].copy()
                    def save():
                        buf = io.BytesIO()
                        Image.fromarray(frame).save(buf, format="PNG", compress_level=4)
                        return buf.tell()
                    once[depth] = host_median(save)
                row["pil_save_ms"], row["pil_bytes"] = once[depth]
            results.append(row)
            del a, b, out, out_host, in_host, off, shifted
        del sources
    doc = {"tool": "png_time", "reps": args.reps, "runs": args.runs, "warmup": args.warmup, "host_reps": args.host_reps, "results": results}
    print(json.dumps(doc), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(doc, indent=1) + "\n")
    tex.destroy()


if __name__ == "__main__":
    main()
