"""ctypes loader and wrappers for librrt_exr.so (C ABI: include/rrt_exr.h): the frame's linear HDR packed as the scanline chunks of
an OpenEXR file -- half or float, raw or filtered for deflate -- on the device (launch_exr_from_hdr) or on the host from the same
source (exr_from_hdr_host), with the file's header (exr_header) and chunk layout (exr_frame_bytes, exr_chunks).  sinks.EXRSink
deflates and writes the files.

A library of its own with a loader of its own: nothing here is part of _lib.SYMBOLS.  Calls go through _lib.call(..., lib=...), so a
refusal raises the same RRTError as everywhere else, with the library's reason.  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import _ptr, _stream      # the package's own argument rules: a device tensor or a raw address; a stream or torch's current one
from ._lib import RRTError

LIB_PATH = os.path.join(_lib.PKG, "lib", "librrt_exr.so")
HALF, FLOAT = 1, 2                # the file format's own codes
NONE, ZIPS, ZIP = 0, 2, 3
TYPES = {"half": HALF, "float": FLOAT}
COMPRESSIONS = {"none": NONE, "zips": ZIPS, "zip": ZIP}


class rrt_exr_format(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("type", C.c_int32), ("compression", C.c_int32), ("half_max", C.c_float)]


_vp, _i = C.c_void_p, C.c_int
_fmt = C.POINTER(rrt_exr_format)
_sz = C.POINTER(C.c_size_t)
# every symbol include/rrt_exr.h declares: (name, restype, argtypes)
EXR_SYMBOLS = [
    ("rrt_exr_format_default", _i, [_fmt]),
    ("rrt_exr_frame_bytes", _i, [_fmt, _i, _i, _sz, C.POINTER(C.c_int32)]),
    ("rrt_exr_chunk", _i, [_fmt, _i, _i, _i, C.POINTER(C.c_int32), _sz, _sz]),
    ("rrt_exr_launch_geometry", _i, [_fmt, _i, _i, C.c_size_t, C.POINTER(C.c_int32 * 8)]),
    ("rrt_launch_exr_from_hdr", _i, [_vp, _vp, _i, _i, _fmt, _vp]),
    ("rrt_exr_from_hdr_host", _i, [_vp, _vp, _i, _i, _fmt]),
    ("rrt_exr_unfilter_host", _i, [_vp, _vp, C.c_size_t]),
    ("rrt_exr_header", _i, [_fmt, _i, _i, _i, _i, _vp, C.c_size_t, _sz]),
    ("rrt_exr_last_error", C.c_char_p, []),
]

_exr = None


def load():
    """Load librrt_exr.so.  Raises if it has not been built (no fallback)."""
    global _exr
    if _exr is not None:
        return _exr
    if not os.path.exists(LIB_PATH):
        raise RRTError(-1, "librrt_exr.so is missing", f"expected {LIB_PATH}; run `python -m relativisticraytracer_amd.build`")
    try:  # share torch's HIP runtime when torch is in the process, as _lib.load does
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    _lib._bind(lib, EXR_SYMBOLS)
    _exr = lib
    return lib


def _call(name, *args):
    lib = load()
    try:
        _lib.call(name, *args, lib=lib)
    except RRTError as e:
        why = lib.rrt_exr_last_error().decode()
        if e.status == 3:       # RRT_ERR_HIP: the message is this library's, not librrt_hip.so's
            raise RRTError(3, name, "a HIP runtime call failed -- " + why) from None
        if e.status == 1 and why:
            raise RRTError(1, name, why) from None
        raise


class ExrFormat(rrt_exr_format):
    """rrt_exr_format: type "half" | "float" (or 1 | 2), compression "none" | "zips" | "zip" (or 0 | 2 | 3), half_max: the clamp of
    the half conversion.  Values outside the lists are kept as given: the library refuses them."""

    def __init__(self, type="half", compression="zip", half_max=None):
        super().__init__()
        _call("rrt_exr_format_default", C.byref(self))
        self.type = TYPES.get(type, type)
        self.compression = COMPRESSIONS.get(compression, compression)
        if half_max is not None:
            self.half_max = float(half_max)

    def info(self):
        names = {v: k for k, v in TYPES.items()}, {v: k for k, v in COMPRESSIONS.items()}
        return {"type": names[0].get(self.type, self.type), "compression": names[1].get(self.compression, self.compression),
                "half_max": self.half_max}


def _format(fmt):
    return C.byref(fmt if fmt is not None else ExrFormat())


def exr_frame_bytes(fmt, w, h, chunks=False):
    """bytes of one w x h frame's payload; with chunks=True (bytes, n_chunks)"""
    n, k = C.c_size_t(0), C.c_int32(0)
    _call("rrt_exr_frame_bytes", _format(fmt), int(w), int(h), C.byref(n), C.byref(k))
    return (n.value, k.value) if chunks else n.value


def exr_chunks(fmt, w, h):
    """[(y, offset, bytes)] of every chunk of a w x h frame: its first row, its place in the payload, its raw (= filtered) size"""
    out = []
    for i in range(exr_frame_bytes(fmt, w, h, chunks=True)[1]):
        y, off, n = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
        _call("rrt_exr_chunk", _format(fmt), int(w), int(h), i, C.byref(y), C.byref(off), C.byref(n))
        out.append((y.value, off.value, n.value))
    return out


def exr_header(fmt, w, h, fps_num=24, fps_den=1, cap=1024):
    """the file's header as bytes: magic, version, attributes and the closing 0 (rrt_exr_header); the offset table follows it"""
    buf, n = C.create_string_buffer(max(int(cap), 1)), C.c_size_t(0)
    _call("rrt_exr_header", _format(fmt), int(w), int(h), int(fps_num), int(fps_den), buf, int(cap), C.byref(n))
    return buf.raw[:n.value]


def exr_launch_geometry(fmt, w, h, address_bits=0):
    """how a launch of this size is laid out (rrt_exr_launch_geometry, host only).  address_bits: the payload's and the HDR plane's
    addresses OR-ed together (0: both 16-byte aligned).  "passes" > 1: the grid's row dimension wraps."""
    out = (C.c_int32 * 8)()
    _call("rrt_exr_launch_geometry", _format(fmt), int(w), int(h), int(address_bits), C.byref(out))
    return {"threads": out[0], "block": (out[1], out[2]), "pixels": out[3], "grid": (out[4], out[5]), "wide": bool(out[6]), "passes": out[7]}


def launch_exr_from_hdr(d_payload, d_hdr, w, h, fmt=None, stream=None):
    """The w x h linear HDR frame at d_hdr (w*h*4 float32, bottom-up rows: what `hdr=` and launch_exposure write) as the chunks of an
    EXR file into d_payload (exr_frame_bytes bytes).  Tensors or raw device addresses; one kernel on `stream` (default: torch's
    current stream)."""
    _call("rrt_launch_exr_from_hdr", _ptr(d_payload), _ptr(d_hdr), int(w), int(h), _format(fmt), _stream(stream))


def exr_from_hdr_host(frame, fmt=None):
    """the payload (uint8 array) of an (h, w, 4) float32 HDR frame on the host, from the source the kernels run"""
    a = np.ascontiguousarray(frame, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an (h, w, 4) float32 frame, got {a.shape}")
    h, w = a.shape[:2]
    out = np.empty(exr_frame_bytes(fmt, w, h), np.uint8)
    _call("rrt_exr_from_hdr_host", out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), w, h, _format(fmt))
    return out


def exr_unfilter_host(filtered):
    """the raw bytes (uint8 array) of one filtered chunk: the inverse of the step in front of deflate"""
    a = np.ascontiguousarray(np.frombuffer(filtered, np.uint8) if isinstance(filtered, (bytes, bytearray, memoryview)) else filtered, np.uint8)
    out = np.empty(a.size, np.uint8)
    _call("rrt_exr_unfilter_host", out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), a.size)
    return out


__all__ = ["ExrFormat", "exr_frame_bytes", "exr_chunks", "exr_header", "launch_exr_from_hdr", "exr_from_hdr_host", "exr_unfilter_host",
           "exr_launch_geometry"]
