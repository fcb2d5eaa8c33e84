"""ctypes loader and wrappers for librrt_yuv.so (C ABI: include/rrt_yuv.h): a frame packed as planar BT.709 Y'CbCr in the byte
layout of a YUV4MPEG2 frame, on the device (launch_yuv_from_rgba8, launch_yuv_from_hdr) or on the host from the same source
(yuv_from_rgba8_host, yuv_from_hdr_host).  Its HDR10 leg -- the linear HDR as PQ BT.2020 with MaxCLL / MaxFALL metered on the
device -- is launch_yuv_hdr10_from_hdr, yuv_hdr10_from_hdr_host and their queries, further down.

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


class rrt_yuv_hdr10(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("white_nits", C.c_float), ("peak_nits", C.c_float), ("knee", C.c_float)]


class rrt_yuv_hdr10_light(C.Structure):
    """step F's state, as the device and the host conversions keep it: 32 bytes"""
    _fields_ = [("frame_sum", C.c_uint64), ("max_frame_sum", C.c_uint64), ("frame_max", C.c_uint32), ("max_cll", C.c_uint32),
                ("frames", C.c_uint32), ("reserved", C.c_uint32)]


_vp, _i = C.c_void_p, C.c_int
_fmt = C.POINTER(rrt_yuv_format)
_h10 = C.POINTER(rrt_yuv_hdr10)
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
    ("rrt_yuv_hdr10_default", _i, [_h10]),
    ("rrt_yuv_hdr10_coefficients", _i, [_fmt, C.POINTER(C.c_int64 * 9), C.POINTER(C.c_int32 * 3)]),
    ("rrt_yuv_hdr10_light_bytes", _i, [C.POINTER(C.c_size_t)]),
    ("rrt_launch_yuv_hdr10_from_hdr", _i, [_vp, _vp, _i, _i, _fmt, _h10, _vp, _vp]),
    ("rrt_launch_yuv_hdr10_light_reset", _i, [_vp, _vp]),
    ("rrt_yuv_hdr10_from_hdr_host", _i, [_vp, _vp, _i, _i, _fmt, _h10, _vp]),
    ("rrt_yuv_hdr10_light_levels", _i, [_vp, _i, _i, C.POINTER(C.c_uint32 * 3)]),
    ("rrt_y4m_hdr10_sidecar", _i, [_h10, C.POINTER(C.c_uint32 * 3), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]),
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


# ---- HDR10 output (include/rrt_yuv.h, "HDR10 output")

LIGHT_BYTES = C.sizeof(rrt_yuv_hdr10_light)
LIGHT_DTYPE = np.dtype([("frame_sum", "<u8"), ("max_frame_sum", "<u8"), ("frame_max", "<u4"), ("max_cll", "<u4"), ("frames", "<u4"),
                        ("reserved", "<u4")])


class Hdr10Settings(rrt_yuv_hdr10):
    """rrt_yuv_hdr10: the luminance of H = 1 (white_nits), the shoulder's asymptote (peak_nits) and where it starts as a fraction of
    the peak (knee).  Values out of range are kept as given: the library refuses them."""

    def __init__(self, white_nits=None, peak_nits=None, knee=None):
        super().__init__()
        _call("rrt_yuv_hdr10_default", C.byref(self))
        for name, v in (("white_nits", white_nits), ("peak_nits", peak_nits), ("knee", knee)):
            if v is not None:
                setattr(self, name, float(v))

    def info(self):
        return {"white_nits": self.white_nits, "peak_nits": self.peak_nits, "knee": self.knee}


def _hdr10(s):
    return C.byref(s if s is not None else Hdr10Settings())


def _fmt10(fmt):
    return C.byref(fmt if fmt is not None else YuvFormat(bits=10))


def yuv_hdr10_coefficients(fmt=None):
    """(coef, off) of a 10-bit format with BT.2020's Kr and Kb (fmt None: 4:2:0, limited)"""
    coef, off = (C.c_int64 * 9)(), (C.c_int32 * 3)()
    _call("rrt_yuv_hdr10_coefficients", _fmt10(fmt), C.byref(coef), C.byref(off))
    return np.array(coef, np.int64).reshape(3, 3), np.array(off, np.int32)


def yuv_hdr10_light_bytes():
    """the size of the light-level state a metered launch keeps on the device: 32"""
    n = C.c_size_t(0)
    _call("rrt_yuv_hdr10_light_bytes", C.byref(n))
    return n.value


def launch_yuv_hdr10_from_hdr(d_yuv, d_hdr, w, h, fmt=None, hdr10=None, d_light=None, stream=None):
    """The linear HDR frame at d_hdr as PQ BT.2020 Y'CbCr planes (10 bits) into d_yuv.  d_light: a 16-byte aligned device buffer of
    yuv_hdr10_light_bytes() bytes (a tensor or a raw address) that meters the frame -- the pack kernel, then a one-thread fold
    kernel -- or None: one kernel, nothing metered."""
    _call("rrt_launch_yuv_hdr10_from_hdr", _ptr(d_yuv), _ptr(d_hdr), int(w), int(h), _fmt10(fmt), _hdr10(hdr10),
          _ptr(d_light) if d_light is not None else None, _stream(stream))


def launch_yuv_hdr10_light_reset(d_light, stream=None):
    """zero the light-level state: once per film"""
    _call("rrt_launch_yuv_hdr10_light_reset", _ptr(d_light), _stream(stream))


def yuv_hdr10_from_hdr_host(frame, fmt=None, hdr10=None, light=None):
    """the frame bytes of an (h, w, 4) float32 HDR frame on the host, from the source the kernels run.  light: a 32-byte state
    (a LIGHT_DTYPE array of one element, or any writable 32-byte buffer) that the frame is metered and folded into, or None."""
    a = np.ascontiguousarray(frame, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an (h, w, 4) float32 frame, got {a.shape}")
    h, w = a.shape[:2]
    f = fmt if fmt is not None else YuvFormat(bits=10)
    out = np.empty(yuv_frame_bytes(f, w, h), np.uint8)
    lp = None
    if light is not None:
        la = np.asarray(light)
        if la.nbytes != LIGHT_BYTES or not la.flags.c_contiguous or not la.flags.writeable or la.ctypes.data % 8:
            raise ValueError(f"light: a writable, contiguous, 8-byte aligned buffer of {LIGHT_BYTES} bytes")
        lp = la.ctypes.data_as(C.c_void_p)
    _call("rrt_yuv_hdr10_from_hdr_host", out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), w, h, C.byref(f), _hdr10(hdr10), lp)
    return out


def yuv_hdr10_light_levels(state, w, h):
    """{"max_cll", "max_fall", "frames"} from a host copy of the state (32 bytes: a LIGHT_DTYPE array, a uint8 array or bytes)"""
    raw = bytes(state) if isinstance(state, (bytes, bytearray)) else np.ascontiguousarray(state).tobytes()
    if len(raw) != LIGHT_BYTES:
        raise ValueError(f"the state is {LIGHT_BYTES} bytes, got {len(raw)}")
    st = rrt_yuv_hdr10_light.from_buffer_copy(raw)
    out = (C.c_uint32 * 3)()
    _call("rrt_yuv_hdr10_light_levels", C.byref(st), int(w), int(h), C.byref(out))
    return {"max_cll": out[0], "max_fall": out[1], "frames": out[2]}


def y4m_hdr10_sidecar(hdr10, levels):
    """the bytes of <path>.hdr10.json (rrt_y4m_hdr10_sidecar): levels as yuv_hdr10_light_levels gives them"""
    lv = (C.c_uint32 * 3)(int(levels["max_cll"]), int(levels["max_fall"]), int(levels["frames"]))
    buf, n = C.create_string_buffer(1024), C.c_size_t(0)
    _call("rrt_y4m_hdr10_sidecar", _hdr10(hdr10), C.byref(lv), buf, 1024, C.byref(n))
    return buf.raw[:n.value]


__all__ = ["Hdr10Settings", "yuv_hdr10_coefficients", "yuv_hdr10_light_bytes", "launch_yuv_hdr10_from_hdr", "launch_yuv_hdr10_light_reset",
           "yuv_hdr10_from_hdr_host", "yuv_hdr10_light_levels", "y4m_hdr10_sidecar",
           "YuvFormat", "yuv_coefficients", "yuv_frame_bytes", "y4m_header", "launch_yuv_from_rgba8", "launch_yuv_from_hdr",
           "yuv_from_rgba8_host", "yuv_from_hdr_host", "yuv_launch_geometry"]
