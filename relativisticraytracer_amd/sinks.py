"""Frame sinks for the headless driver (replaces the reference's ScreenRecorder,
src/main.cpp:29-124, which pipes glReadPixels() output into ffmpeg).

Frames arrive as (h, w, 4) uint8 arrays in the kernel's native order: RGBA, bottom-up rows
(raymarcher.cu:168) -- the same bytes glReadPixels hands the reference's recorder."""
import os
import re
import shutil
import struct
import subprocess
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np


class RawSink:
    """Concatenated raw RGBA frames, bottom-up -- byte-for-byte what the reference writes into the
    ffmpeg pipe (main.cpp:85-97).  Convert later with the reference's own arguments:
    ffmpeg -f rawvideo -pix_fmt rgba -s WxH -r 24 -i frames.rgba -vf vflip -c:v libx264 ..."""

    def __init__(self, path, width, height):
        self.f = open(path, "wb")
        self.width, self.height, self.frames = width, height, 0

    def write(self, frame):
        frame = np.ascontiguousarray(frame, np.uint8)
        if frame.shape != (self.height, self.width, 4):
            raise ValueError("frame shape mismatch")
        self.f.write(frame.tobytes())
        self.frames += 1

    def close(self):
        self.f.close()


class PPMSink:
    """One binary PPM per frame (RGB, top-down: the vertical flip the reference delegates to
    ffmpeg's `-vf vflip`, main.cpp:67, is applied here)."""

    def __init__(self, directory, width, height, prefix="frame"):
        os.makedirs(directory, exist_ok=True)
        self.dir, self.prefix = directory, prefix
        self.width, self.height, self.frames = width, height, 0

    def write(self, frame):
        frame = np.ascontiguousarray(frame, np.uint8)
        if frame.shape != (self.height, self.width, 4):
            raise ValueError("frame shape mismatch")
        self.frames += 1
        with open(os.path.join(self.dir, f"{self.prefix}_{self.frames:05d}.ppm"), "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (self.width, self.height))
            f.write(frame[::-1, :, :3].tobytes())

    def close(self):
        pass


class FFmpegSink:
    """The reference's recorder, argument for argument (main.cpp:60-72).  Only usable where an
    `ffmpeg` binary exists; raises otherwise (there is none in the build image)."""

    def __init__(self, path, width, height, fps=24):
        exe = shutil.which("ffmpeg")
        if exe is None:
            raise RuntimeError("ffmpeg not found in PATH (the reference prints the same complaint, main.cpp:76)")
        cmd = [exe, "-y", "-f", "rawvideo", "-pix_fmt", "rgba", "-s", f"{width}x{height}", "-r", str(fps),
               "-i", "-", "-vf", "vflip", "-c:v", "libx264", "-preset", "fast", "-crf", "18",
               "-pix_fmt", "yuv420p", path]
        self.p = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        self.width, self.height, self.frames = width, height, 0

    def write(self, frame):
        self.p.stdin.write(np.ascontiguousarray(frame, np.uint8).tobytes())
        self.frames += 1

    def close(self):
        self.p.stdin.close()
        self.p.wait()


class Y4MSink:
    """A YUV4MPEG2 stream (include/rrt_yuv.h, step 5): the header on open, then `FRAME` and one frame's planes per write -- the
    bytes launch_yuv_from_rgba8 / launch_yuv_from_hdr (or their *_host forms) produce, top-down already.  BT.709; a Y4M header
    carries no matrix tag, so a player is told: `mpv --vf=format=colormatrix=bt.709 x.y4m`.

    With hdr10 (an Hdr10Settings) the frames are launch_yuv_hdr10_from_hdr's -- PQ, BT.2020 -- and the header cannot say so either:
    close(levels) writes `<path>.hdr10.json` (step G's sidecar) with the settings, MaxCLL / MaxFALL and the encoder options."""

    def __init__(self, path, width, height, fps=24, fmt=None, hdr10=None):
        from . import yuv
        self.path, self.hdr10 = path, hdr10
        self.fmt = fmt if fmt is not None else yuv.YuvFormat()
        self.frame_bytes = yuv.yuv_frame_bytes(self.fmt, width, height)
        header = yuv.y4m_header(self.fmt, width, height, int(fps), 1)
        self.f = open(path, "wb")
        self.f.write(header)
        self.width, self.height, self.frames = width, height, 0

    def write(self, yuv_bytes):
        data = memoryview(np.ascontiguousarray(yuv_bytes)).cast("B")
        if data.nbytes != self.frame_bytes:
            raise ValueError(f"a {self.width}x{self.height} frame of this format is {self.frame_bytes} bytes, got {data.nbytes}")
        self.f.write(b"FRAME\n")
        self.f.write(data)
        self.frames += 1

    def close(self, levels=None):
        """levels: yuv_hdr10_light_levels' dict of the film -- needed, and only used, with hdr10"""
        if self.hdr10 is not None and levels is None:
            raise ValueError("an HDR10 sink closes with the film's light levels (yuv_hdr10_light_levels)")
        self.f.close()
        if self.hdr10 is not None:
            from . import yuv
            with open(self.path + ".hdr10.json", "wb") as f:
                f.write(yuv.y4m_hdr10_sidecar(self.hdr10, levels))


_FRAME_FIELD = re.compile(r"%(0\d+)?d")


def frame_fields(pattern):
    """how many frame fields (`%d`, `%04d`, ...) a file name pattern holds"""
    return len(_FRAME_FIELD.findall(pattern))


def frame_name(pattern, k):
    """the pattern with its frame fields filled with k (a plain name stays as it is)"""
    return _FRAME_FIELD.sub(lambda m: m.group(0) % k, pattern)


class EXRSink:
    """One OpenEXR file per frame (include/rrt_exr.h, step 5): scene-linear B, G, R scanlines, half or float.  `write` takes one
    frame's payload -- the bytes launch_exr_from_hdr (or exr_from_hdr_host) produce, chunk behind chunk, filtered already when the
    format compresses -- and is left with nothing but deflate: every chunk through zlib at `level`, the chunks side by side on a
    thread pool (zlib releases the GIL), and a chunk that deflate does not shrink stored raw, un-filtered, as the format asks.

    `pattern` holds exactly one frame field, `%d` or `%0Nd`, filled with the frame's number (1, 2, ... in the order written, or
    `index`); a plain name is accepted for a single frame.  A file is written as NAME.tmp and renamed when it is complete.
    threads: the pool's size (default: min(16, the CPUs this process may run on)); 1 deflates in the caller's thread.
    layers: an exr.ExrLayers -- the files hold its channels (data layers next to B, G, R) and `write` takes launch_exr_layers'
    payload; None: B, G, R of `fmt`, as ever."""

    def __init__(self, pattern, width, height, fps=24, fmt=None, level=4, threads=None, layers=None):
        from . import exr
        self.exr = exr
        if frame_fields(pattern) > 1:
            raise ValueError(f"{pattern!r}: one frame field (%d or %0Nd), not {frame_fields(pattern)}")
        if not 1 <= int(level) <= 9:
            raise ValueError("level: 1 ... 9")
        self.pattern, self.level = pattern, int(level)
        self.fmt = fmt if fmt is not None else exr.ExrFormat()
        if layers is not None:      # an exr.ExrLayers: its channel list, and its compression in place of fmt's
            if (layers.w, layers.h) != (width, height):
                raise ValueError(f"the layers are for {layers.w}x{layers.h} frames, not {width}x{height}")
            self.frame_bytes = exr.exr_layers_frame_bytes(layers)
            self.chunks = exr.exr_layers_chunks(layers)
            self.header = exr.exr_layers_header(layers, int(fps), 1)
            self.compressed = layers.compression != exr.NONE
        else:
            self.frame_bytes = exr.exr_frame_bytes(self.fmt, width, height)
            self.chunks = exr.exr_chunks(self.fmt, width, height)
            self.header = exr.exr_header(self.fmt, width, height, int(fps), 1)
            self.compressed = self.fmt.compression != exr.NONE
        workers = int(threads) if threads is not None else min(16, len(os.sched_getaffinity(0)))
        self.pool = ThreadPoolExecutor(workers) if self.compressed and workers > 1 and len(self.chunks) > 1 else None
        self.width, self.height, self.frames, self.threads = width, height, 0, max(workers, 1)
        self.stored_raw = 0          # chunks that deflate did not shrink, over all frames

    def _chunk(self, piece):
        z = zlib.compress(piece, self.level)
        return z if len(z) < len(piece) else self.exr.exr_unfilter_host(piece).tobytes()

    def write(self, payload, index=None):
        data = memoryview(np.ascontiguousarray(payload)).cast("B")
        if data.nbytes != self.frame_bytes:
            raise ValueError(f"a {self.width}x{self.height} frame of this format is {self.frame_bytes} bytes, got {data.nbytes}")
        k = self.frames + 1 if index is None else int(index)
        if self.frames > 0 and frame_fields(self.pattern) == 0:
            raise ValueError(f"{self.pattern!r} has no frame field: a second frame would overwrite the first")
        pieces = [data[off:off + n] for _, off, n in self.chunks]
        if self.compressed:
            pieces = list(self.pool.map(self._chunk, pieces)) if self.pool is not None else [self._chunk(p) for p in pieces]
            self.stored_raw += sum(len(p) == n for p, (_, _, n) in zip(pieces, self.chunks))
        at, table = len(self.header) + 8 * len(pieces), []
        for p in pieces:
            table.append(at)
            at += 8 + len(p)
        name = frame_name(self.pattern, k)
        with open(name + ".tmp", "wb") as f:
            f.write(self.header)
            f.write(struct.pack(f"<{len(table)}Q", *table))
            for (y, _, _), p in zip(self.chunks, pieces):
                f.write(struct.pack("<ii", y, len(p)))
                f.write(p)
        os.replace(name + ".tmp", name)
        self.frames += 1
        return name

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
            self.pool = None


class PNGSink:
    """One PNG file per frame (include/rrt_png.h, step 6): RGB, 8 or 16 bits.  `write` takes one frame's payload and row sums -- what
    launch_png_from_rgba8 / launch_png_from_hdr (or their *_host forms) produce: the scanlines filtered already, the Adler-32 a fold
    of the sums -- and is left with nothing but deflate: the payload in slices of png_slices rows, each a raw deflate stream of its
    own that ends on a byte boundary (sync flush; the last one finishes), one IDAT per slice, side by side on a thread pool (zlib
    releases the GIL).  The cut depends on the frame alone, so a file's bytes do not depend on `threads`.

    `write_streams` takes the slices deflated already (include/rrt_deflate.h) and writes the same file around them.

    `pattern`, NAME.tmp then rename, and `threads` as EXRSink's.  level: zlib's 1 ... 9; the strategy is STRATEGY for every file
    (rrt_headless uses the same; DESIGN.md section 4, "PNG output", has the sizes behind the choice)."""

    STRATEGY = zlib.Z_FILTERED

    def __init__(self, pattern, width, height, fmt=None, level=4, threads=None):
        from . import png
        self.png = png
        if frame_fields(pattern) > 1:
            raise ValueError(f"{pattern!r}: one frame field (%d or %0Nd), not {frame_fields(pattern)}")
        if not 1 <= int(level) <= 9:
            raise ValueError("level: 1 ... 9")
        self.pattern, self.level = pattern, int(level)
        self.fmt = fmt if fmt is not None else png.PngFormat()
        self.frame_bytes, self.stride, self.row_sum_bytes = png.png_frame_bytes(self.fmt, width, height, layout=True)
        self.rows_per_slice, self.n_slices = png.png_slices(self.fmt, width, height)
        self.header = png.png_header(self.fmt, width, height)
        workers = int(threads) if threads is not None else min(16, len(os.sched_getaffinity(0)))
        self.pool = ThreadPoolExecutor(workers) if workers > 1 and self.n_slices > 1 else None
        self.width, self.height, self.frames, self.threads = width, height, 0, max(workers, 1)

    def _slice(self, job):
        piece, last = job
        z = zlib.compressobj(self.level, zlib.DEFLATED, -15, 8, self.STRATEGY)
        return z.compress(piece) + z.flush(zlib.Z_FINISH if last else zlib.Z_SYNC_FLUSH)

    @staticmethod
    def _chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))

    def write(self, payload, row_sums, index=None):
        data = memoryview(np.ascontiguousarray(payload)).cast("B")
        if data.nbytes != self.frame_bytes:
            raise ValueError(f"a {self.width}x{self.height} frame of this format is {self.frame_bytes} bytes, got {data.nbytes}")
        k = self.frames + 1 if index is None else int(index)
        if self.frames > 0 and frame_fields(self.pattern) == 0:
            raise ValueError(f"{self.pattern!r} has no frame field: a second frame would overwrite the first")
        adler = self.png.png_adler32(row_sums, self.fmt, self.width, self.height)
        step = self.rows_per_slice * self.stride
        jobs = [(data[i * step:(i + 1) * step], i == self.n_slices - 1) for i in range(self.n_slices)]
        pieces = list(self.pool.map(self._slice, jobs)) if self.pool is not None else [self._slice(j) for j in jobs]
        return self._file(pieces, adler, k)

    def write_streams(self, streams, row_sums, index=None):
        """The same file from slices that are deflated already: `streams` holds one raw deflate stream per slice of png_slices, each
        ending on a byte boundary, the last one finished -- what launch_deflate (or deflate_host) makes of the payload with
        stream_bytes = rows_per_slice * stride.  Nothing is deflated here and no thread is used."""
        pieces = [bytes(s) for s in streams]
        if len(pieces) != self.n_slices:
            raise ValueError(f"a {self.width}x{self.height} frame of this format is {self.n_slices} streams, got {len(pieces)}")
        k = self.frames + 1 if index is None else int(index)
        if self.frames > 0 and frame_fields(self.pattern) == 0:
            raise ValueError(f"{self.pattern!r} has no frame field: a second frame would overwrite the first")
        return self._file(pieces, self.png.png_adler32(row_sums, self.fmt, self.width, self.height), k)

    def _file(self, pieces, adler, k):
        pieces[0] = b"\x78\x01" + pieces[0]
        pieces[-1] = pieces[-1] + struct.pack(">I", adler)
        name = frame_name(self.pattern, k)
        with open(name + ".tmp", "wb") as f:
            f.write(self.header)
            for p in pieces:
                f.write(self._chunk(b"IDAT", p))
            f.write(self._chunk(b"IEND", b""))
        os.replace(name + ".tmp", name)
        self.frames += 1
        return name

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()
            self.pool = None


def open_sink(spec, width, height, fps=24):
    """spec: None | 'x.rgba' | 'dir/' (PPM per frame) | 'x.mp4' (ffmpeg)."""
    if not spec:
        return None
    if spec.endswith(".rgba") or spec.endswith(".raw"):
        return RawSink(spec, width, height)
    if spec.endswith(".mp4"):
        return FFmpegSink(spec, width, height, fps)
    return PPMSink(spec, width, height)
