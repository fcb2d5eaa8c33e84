"""ctypes loader and wrappers for librrt_png.so (C ABI: include/rrt_png.h): a finished frame as the filtered scanlines of a PNG file --
8 bits from the RGBA8 frame, 16 bits from the linear HDR -- with the per-row sums its Adler-32 folds from, on the device
(launch_png_from_rgba8, launch_png_from_hdr) or on the host from the same source (png_from_rgba8_host, png_from_hdr_host), and the
host queries: the layout (png_frame_bytes, png_slices), the file's first chunks (png_header), the checksum (png_adler32) and the
inverse (png_unfilter_host).  sinks.PNGSink deflates and writes the files.

A library of its own with a loader of its own: nothing here is part of _lib.SYMBOLS.  Calls go through _lib.call(..., lib=...), so a
refusal raises the same RRTError as everywhere else, with the library's reason.  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import _ptr, _stream      # the package's own argument rules: a device tensor or a raw address; a stream or torch's current one
from ._lib import RRTError

LIB_PATH = os.path.join(_lib.PKG, "lib", "librrt_png.so")
NONE, SUB, UP, AVERAGE, PAETH, ADAPTIVE = range(6)      # the file format's filter type numbers, and the row-by-row choice
FILTERS = {"none": NONE, "sub": SUB, "up": UP, "average": AVERAGE, "paeth": PAETH, "adaptive": ADAPTIVE}
SLICE_BYTES, BAND_ROWS, SEGMENT_CHUNKS = 1 << 20, 4, 2024     # include/rrt_png.h's constants


class rrt_png_format(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("depth", C.c_int32), ("filter", C.c_int32)]


_vp, _i = C.c_void_p, C.c_int
_fmt = C.POINTER(rrt_png_format)
_sz = C.POINTER(C.c_size_t)
_i32 = C.POINTER(C.c_int32)
# every symbol include/rrt_png.h declares: (name, restype, argtypes)
PNG_SYMBOLS = [
    ("rrt_png_format_default", _i, [_fmt]),
    ("rrt_png_frame_bytes", _i, [_fmt, _i, _i, _sz, _sz, _sz]),
    ("rrt_png_slices", _i, [_fmt, _i, _i, _i32, _i32]),
    ("rrt_png_launch_geometry", _i, [_fmt, _i, _i, C.c_size_t, C.POINTER(C.c_int32 * 8)]),
    ("rrt_launch_png_from_rgba8", _i, [_vp, _vp, _vp, _i, _i, _fmt, _vp]),
    ("rrt_launch_png_from_hdr", _i, [_vp, _vp, _vp, _i, _i, _fmt, _vp]),
    ("rrt_png_from_rgba8_host", _i, [_vp, _vp, _vp, _i, _i, _fmt]),
    ("rrt_png_from_hdr_host", _i, [_vp, _vp, _vp, _i, _i, _fmt]),
    ("rrt_png_unfilter_host", _i, [_vp, _vp, _i, _i, _fmt]),
    ("rrt_png_adler32", _i, [_vp, _i, _i, _fmt, C.POINTER(C.c_uint32)]),
    ("rrt_png_header", _i, [_fmt, _i, _i, _vp, C.c_size_t, _sz]),
    ("rrt_png_last_error", C.c_char_p, []),
]

_png = None


def load():
    """Load librrt_png.so.  Raises if it has not been built (no fallback)."""
    global _png
    if _png is not None:
        return _png
    if not os.path.exists(LIB_PATH):
        raise RRTError(-1, "librrt_png.so is missing", f"expected {LIB_PATH}; run `python -m relativisticraytracer_amd.build`")
    try:  # share torch's HIP runtime when torch is in the process, as _lib.load does
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    _lib._bind(lib, PNG_SYMBOLS)
    _png = lib
    return lib


def _call(name, *args):
    lib = load()
    try:
        _lib.call(name, *args, lib=lib)
    except RRTError as e:
        why = lib.rrt_png_last_error().decode()
        if e.status == 3:       # RRT_ERR_HIP: the message is this library's, not librrt_hip.so's
            raise RRTError(3, name, "a HIP runtime call failed -- " + why) from None
        if e.status == 1 and why:
            raise RRTError(1, name, why) from None
        raise


class PngFormat(rrt_png_format):
    """rrt_png_format: depth 8 | 16, filter "adaptive" | "none" | "sub" | "up" | "average" | "paeth" (or 5 | 0 ... 4).  Values
    outside the lists are kept as given: the library refuses them."""

    def __init__(self, depth=8, filter="adaptive"):
        super().__init__()
        _call("rrt_png_format_default", C.byref(self))
        self.depth = int(depth)
        self.filter = FILTERS.get(filter, filter)

    @property
    def bpp(self):
        return 3 if self.depth == 8 else 6

    def info(self):
        names = {v: k for k, v in FILTERS.items()}
        return {"depth": self.depth, "filter": names.get(self.filter, self.filter)}


def _format(fmt):
    return C.byref(fmt if fmt is not None else PngFormat())


def png_frame_bytes(fmt, w, h, layout=False):
    """bytes of one w x h frame's payload; with layout=True (payload bytes, stride, bytes of the row-sum table)"""
    n, stride, table = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    _call("rrt_png_frame_bytes", _format(fmt), int(w), int(h), C.byref(n), C.byref(stride), C.byref(table))
    return (n.value, stride.value, table.value) if layout else n.value


def png_slices(fmt, w, h):
    """(rows per slice, slices): how the payload is cut for deflate -- by the frame alone"""
    rows, n = C.c_int32(0), C.c_int32(0)
    _call("rrt_png_slices", _format(fmt), int(w), int(h), C.byref(rows), C.byref(n))
    return rows.value, n.value


def png_launch_geometry(fmt, w, h, address_bits=0):
    """how a launch of this size is laid out (rrt_png_launch_geometry, host only).  address_bits: the payload's and the input's
    addresses OR-ed together (0: both 16-byte aligned).  "segments" > 1: a row is longer than the LDS staging."""
    out = (C.c_int32 * 8)()
    _call("rrt_png_launch_geometry", _format(fmt), int(w), int(h), int(address_bits), C.byref(out))
    return {"threads": out[0], "rows": out[1], "grid": out[2], "chunks": out[3], "segments": out[4], "lds_bytes": out[5],
            "wide": bool(out[6]), "segment_chunks": out[7]}


def png_header(fmt, w, h, cap=256):
    """the file's bytes from the signature through tEXt (rrt_png_header); the IDAT chunks follow"""
    buf, n = C.create_string_buffer(max(int(cap), 1)), C.c_size_t(0)
    _call("rrt_png_header", _format(fmt), int(w), int(h), buf, int(cap), C.byref(n))
    return buf.raw[:n.value]


def png_adler32(row_sums, fmt, w, h):
    """the zlib stream's Adler-32 from a frame's row-sum table (a host array of 2 * h uint32)"""
    a = np.ascontiguousarray(row_sums, np.uint32)
    if a.size != 2 * int(h):
        raise ValueError(f"a {w}x{h} frame has {2 * int(h)} row sums, got {a.size}")
    out = C.c_uint32(0)
    _call("rrt_png_adler32", a.ctypes.data_as(C.c_void_p), int(w), int(h), _format(fmt), C.byref(out))
    return out.value


def launch_png_from_rgba8(d_payload, d_row_sums, d_rgba8, w, h, fmt=None, stream=None):
    """The finished w x h RGBA8 frame at d_rgba8 (bottom-up rows) as an 8-bit PNG's filtered scanlines into d_payload
    (png_frame_bytes bytes) and their sums into d_row_sums (2 * h uint32).  Tensors or raw device addresses; one kernel on `stream`
    (default: torch's current stream)."""
    _call("rrt_launch_png_from_rgba8", _ptr(d_payload), _ptr(d_row_sums), _ptr(d_rgba8), int(w), int(h), _format(fmt), _stream(stream))


def launch_png_from_hdr(d_payload, d_row_sums, d_hdr, w, h, fmt=None, stream=None):
    """The same from the frame's linear HDR (w*h*4 float32, bottom-up rows: what `hdr=` and launch_exposure write), tone-mapped to
    16 bits; fmt.depth is 16."""
    _call("rrt_launch_png_from_hdr", _ptr(d_payload), _ptr(d_row_sums), _ptr(d_hdr), int(w), int(h), _format(fmt), _stream(stream))


def _host(name, frame, dtype, fmt):
    a = np.ascontiguousarray(frame, dtype)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an (h, w, 4) {np.dtype(dtype).name} frame, got {a.shape}")
    h, w = a.shape[:2]
    out, sums = np.empty(png_frame_bytes(fmt, w, h), np.uint8), np.empty(2 * h, np.uint32)
    _call(name, out.ctypes.data_as(C.c_void_p), sums.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), w, h, _format(fmt))
    return out, sums


def png_from_rgba8_host(frame, fmt=None):
    """(payload, row sums) of an (h, w, 4) uint8 frame on the host, from the source the kernels run"""
    return _host("rrt_png_from_rgba8_host", frame, np.uint8, fmt)


def png_from_hdr_host(frame, fmt):
    """(payload, row sums) of an (h, w, 4) float32 HDR frame on the host; fmt.depth is 16"""
    return _host("rrt_png_from_hdr_host", frame, np.float32, fmt)


def png_unfilter_host(payload, fmt, w, h):
    """the raw scanlines, an (h, w * bpp) uint8 array, top-down, of a payload: the inverse of the filters its rows name"""
    a = np.ascontiguousarray(np.frombuffer(payload, np.uint8) if isinstance(payload, (bytes, bytearray, memoryview)) else payload, np.uint8)
    n, stride, _ = png_frame_bytes(fmt, w, h, layout=True)
    if a.size != n:
        raise ValueError(f"a {w}x{h} frame of this format is {n} bytes, got {a.size}")
    out = np.empty((int(h), stride - 1), np.uint8)
    _call("rrt_png_unfilter_host", out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), int(w), int(h), _format(fmt))
    return out


__all__ = ["PngFormat", "png_frame_bytes", "png_slices", "png_launch_geometry", "png_header", "png_adler32", "launch_png_from_rgba8",
           "launch_png_from_hdr", "png_from_rgba8_host", "png_from_hdr_host", "png_unfilter_host"]
