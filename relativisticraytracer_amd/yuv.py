"""ctypes loader and wrappers for librrt_yuv.so (C ABI: include/rrt_yuv.h): a frame packed as planar BT.709 Y'CbCr in the byte
layout of a YUV4MPEG2 frame, on the device (launch_yuv_from_rgba8, launch_yuv_from_hdr) or on the host from the same source
(yuv_from_rgba8_host, yuv_from_hdr_host).

A library of its own with a loader of its own: nothing here is part of _lib.SYMBOLS.  Calls go through _lib.call(..., lib=...), so a
refusal raises the same RRTError as everywhere else.  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import _ptr, _stream      # the package's own argument rules: a device tensor or a raw address; a stream or torch's current one
from ._lib import RRTError

LIB_PATH = os.path.join(_lib.PKG, "lib", "librrt_yuv.so")


class rrt_yuv_format(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("chroma", C.c_int32), ("range", C.c_int32), ("bits", C.c_int32)]


_vp, _i = C.c_void_p, C.c_int
_fmt = C.POINTER(rrt_yuv_format)
# every symbol include/rrt_yuv.h declares: (name, restype, argtypes)
YUV_SYMBOLS = [
    ("rrt_yuv_format_default", _i, [_fmt]),
    ("rrt_yuv_coefficients", _i, [_fmt, C.POINTER(C.c_int64 * 9), C.POINTER(C.c_int32 * 3)]),
    ("rrt_yuv_frame_bytes", _i, [_fmt, _i, _i, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t * 3)]),
    ("rrt_y4m_header", _i, [_fmt, _i, _i, _i, _i, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("rrt_yuv_launch_geometry", _i, [_fmt, _i, _i, C.POINTER(C.c_int32 * 4)]),
    ("rrt_launch_yuv_from_rgba8", _i, [_vp, _vp, _i, _i, _fmt, _vp]),
    ("rrt_launch_yuv_from_hdr", _i, [_vp, _vp, _i, _i, _fmt, _vp]),
    ("rrt_yuv_from_rgba8_host", _i, [_vp, _vp, _i, _i, _fmt]),
    ("rrt_yuv_from_hdr_host", _i, [_vp, _vp, _i, _i, _fmt]),
    ("rrt_yuv_last_error", C.c_char_p, []),
]

_yuv = None


def load():
    """Load librrt_yuv.so.  Raises if it has not been built (no fallback)."""
    global _yuv
    if _yuv is not None:
        return _yuv
    if not os.path.exists(LIB_PATH):
        raise RRTError(-1, "librrt_yuv.so is missing", f"expected {LIB_PATH}; run `python -m relativisticraytracer_amd.build`")
    try:  # share torch's HIP runtime when torch is in the process, as _lib.load does
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    _lib._bind(lib, YUV_SYMBOLS)
    _yuv = lib
    return lib


def _call(name, *args):
    lib = load()
    try:
        _lib.call(name, *args, lib=lib)
    except RRTError as e:
        if e.status == 3:       # RRT_ERR_HIP: the message is this library's, not librrt_hip.so's
            raise RRTError(3, name, "a HIP runtime call failed -- " + lib.rrt_yuv_last_error().decode()) from None
        raise


class YuvFormat(rrt_yuv_format):
    """rrt_yuv_format: chroma 420 | 444, range "limited" | "full" (or 0 | 1), bits 8 | 10.  Values outside the lists are kept as
    given: the library refuses them."""

    def __init__(self, chroma=420, range="limited", bits=8):
        super().__init__()
        _call("rrt_yuv_format_default", C.byref(self))
        self.chroma, self.bits = int(chroma), int(bits)
        self.range = {"limited": 0, "full": 1}.get(range, range)

    def info(self):
        return {"chroma": self.chroma, "range": "full" if self.range else "limited", "bits": self.bits}


def _format(fmt):
    return C.byref(fmt if fmt is not None else YuvFormat())


def yuv_coefficients(fmt=None):
    """(coef, off): the 3 x 3 int64 coefficients (rows Y, Cb, Cr; columns R, G, B) and the three int32 offsets of a format"""
    coef, off = (C.c_int64 * 9)(), (C.c_int32 * 3)()
    _call("rrt_yuv_coefficients", _format(fmt), C.byref(coef), C.byref(off))
    return np.array(coef, np.int64).reshape(3, 3), np.array(off, np.int32)


def yuv_frame_bytes(fmt, w, h, planes=False):
    """bytes of one w x h frame; with planes=True also the byte offsets of the Y, Cb and Cr planes: (bytes, (oy, ocb, ocr))"""
    n, offs = C.c_size_t(0), (C.c_size_t * 3)()
    _call("rrt_yuv_frame_bytes", _format(fmt), int(w), int(h), C.byref(n), C.byref(offs))
    return (n.value, tuple(offs)) if planes else n.value


def y4m_header(fmt, w, h, fps_num=24, fps_den=1, cap=160):
    """the stream header line as bytes, newline included (rrt_y4m_header); `cap`: the buffer offered to the library"""
    buf, n = C.create_string_buffer(max(int(cap), 1)), C.c_size_t(0)
    _call("rrt_y4m_header", _format(fmt), int(w), int(h), int(fps_num), int(fps_den), buf, int(cap), C.byref(n))
    return buf.raw[:n.value]


def yuv_launch_geometry(fmt, w, h):
    """how a launch of this size is laid out: {"threads", "strip_w", "strip_h", "wide"} (rrt_yuv_launch_geometry, host only)"""
    out = (C.c_int32 * 4)()
    _call("rrt_yuv_launch_geometry", _format(fmt), int(w), int(h), C.byref(out))
    return {"threads": out[0], "strip_w": out[1], "strip_h": out[2], "wide": bool(out[3])}


def launch_yuv_from_rgba8(d_yuv, d_rgba8, w, h, fmt=None, stream=None):
    """The w x h RGBA8 frame at d_rgba8 (bottom-up rows, as every launch writes it) as Y'CbCr planes into d_yuv (yuv_frame_bytes
    bytes; 16-byte aligned).  Tensors or raw device addresses; one kernel on `stream` (default: torch's current stream)."""
    _call("rrt_launch_yuv_from_rgba8", _ptr(d_yuv), _ptr(d_rgba8), int(w), int(h), _format(fmt), _stream(stream))


def launch_yuv_from_hdr(d_yuv, d_hdr, w, h, fmt=None, stream=None):
    """The same from the frame's linear HDR (w*h*4 float32, what `hdr=` and launch_exposure write): tone-mapped to 16 bits per
    channel, not to bytes, before the matrix -- the source of a 10-bit file."""
    _call("rrt_launch_yuv_from_hdr", _ptr(d_yuv), _ptr(d_hdr), int(w), int(h), _format(fmt), _stream(stream))


def _host(name, frame, dtype, fmt):
    a = np.ascontiguousarray(frame, dtype)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an (h, w, 4) {np.dtype(dtype).name} frame, got {a.shape}")
    h, w = a.shape[:2]
    out = np.empty(yuv_frame_bytes(fmt, w, h), np.uint8)
    _call(name, out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), w, h, _format(fmt))
    return out


def yuv_from_rgba8_host(frame, fmt=None):
    """the frame bytes (uint8 array) of an (h, w, 4) uint8 frame on the host, from the source the kernels run"""
    return _host("rrt_yuv_from_rgba8_host", frame, np.uint8, fmt)


def yuv_from_hdr_host(frame, fmt=None):
    """the frame bytes (uint8 array) of an (h, w, 4) float32 HDR frame on the host, from the source the kernels run"""
    return _host("rrt_yuv_from_hdr_host", frame, np.float32, fmt)


__all__ = ["YuvFormat", "yuv_coefficients", "yuv_frame_bytes", "y4m_header", "launch_yuv_from_rgba8", "launch_yuv_from_hdr",
           "yuv_from_rgba8_host", "yuv_from_hdr_host", "yuv_launch_geometry"]
