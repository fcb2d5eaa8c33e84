"""ctypes loader and wrappers for librrt_exr.so (C ABI: include/rrt_exr.h): the frame's linear HDR packed as the scanline chunks of
an OpenEXR file -- half or float, raw or filtered for deflate -- on the device (launch_exr_from_hdr) or on the host from the same
source (exr_from_hdr_host), with the file's header (exr_header) and chunk layout (exr_frame_bytes, exr_chunks).  sinks.EXRSink
deflates and writes the files.  Data layers -- per-ray planes as further channels of the same scanlines -- go through ExrLayers and
launch_exr_layers / exr_layers_host, with their own header and chunk layout (exr_layers_header, _frame_bytes, _chunks).

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

# ---- data layers (include/rrt_exr.h, the second block comment)
UINT = 0
SRC_F32, SRC_I32 = 0, 1
MAX_SOURCES, MAX_CHANNELS = 8, 16
LAYER_TYPES = {"uint": UINT, "half": HALF, "float": FLOAT}


class rrt_exr_source(C.Structure):
    _fields_ = [("d_data", C.c_void_p), ("words", C.c_int32), ("kind", C.c_int32), ("bottom_up", C.c_int32), ("reserved", C.c_int32)]


class rrt_exr_channel(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("type", C.c_int32), ("source", C.c_int32), ("word", C.c_int32), ("reserved", C.c_int32)]


class rrt_exr_layers(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("compression", C.c_int32), ("half_max", C.c_float), ("n_sources", C.c_int32),
                ("n_channels", C.c_int32), ("reserved", C.c_int32), ("sources", rrt_exr_source * MAX_SOURCES),
                ("channels", rrt_exr_channel * MAX_CHANNELS)]


_lay = C.POINTER(rrt_exr_layers)
EXR_SYMBOLS += [
    ("rrt_exr_layers_default", _i, [_lay]),
    ("rrt_exr_layers_frame_bytes", _i, [_lay, _i, _i, _sz, C.POINTER(C.c_int32)]),
    ("rrt_exr_layers_chunk", _i, [_lay, _i, _i, _i, C.POINTER(C.c_int32), _sz, _sz]),
    ("rrt_exr_layers_launch_geometry", _i, [_lay, _i, _i, C.c_size_t, C.POINTER(C.c_int32 * 8)]),
    ("rrt_launch_exr_layers", _i, [_vp, _lay, _i, _i, _vp]),
    ("rrt_exr_layers_host", _i, [_vp, _lay, _i, _i]),
    ("rrt_exr_layers_header", _i, [_lay, _i, _i, _i, _i, _vp, C.c_size_t, _sz]),
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


# ---- data layers

def _plane(data, w, h):
    """(address, words, kind, the object to keep alive) of a layer's plane: a float32 / int32 tensor or array of w * h * words
    values, or a raw (address, words, kind)"""
    if isinstance(data, tuple):
        return int(data[0]), int(data[1]), int(data[2]), None
    if hasattr(data, "data_ptr"):
        name, n, addr = str(data.dtype).replace("torch.", ""), data.numel(), data.data_ptr()
        if not data.is_contiguous():
            raise ValueError("a layer's plane must be contiguous")
    else:
        data = np.ascontiguousarray(data)
        name, n, addr = data.dtype.name, data.size, data.ctypes.data
    if name not in ("float32", "int32"):
        raise ValueError(f"a layer's plane is float32 or int32, not {name}")
    if n % (w * h) != 0:
        raise ValueError(f"a layer's plane holds {n} values: not a multiple of {w} x {h}")
    return addr, n // (w * h), SRC_F32 if name == "float32" else SRC_I32, data


class ExrLayers(rrt_exr_layers):
    """rrt_exr_layers for w x h frames: the compression and half_max of `fmt` (its type is not used: every layer names its own) and a
    list of layers (name, type, plane, word, bottom_up) -- type "uint" | "half" | "float" (or 0 | 1 | 2); plane a float32 or int32
    tensor (device: launch_exr_layers) or array (host: exr_layers_host) of w * h * words values, or a raw (address, words, kind);
    word the 32-bit word of the plane's pixel; bottom_up whether the plane's rows run bottom-up, as the HDR plane's do.  Planes that
    are one buffer become one source.  The layers are sorted by name, as the file stores them; what breaks a rule is kept as
    given: the library refuses it."""

    def __init__(self, fmt, w, h, layers, sort=True):
        super().__init__()
        _call("rrt_exr_layers_default", C.byref(self))
        fmt = fmt if fmt is not None else ExrFormat()
        self.compression, self.half_max = fmt.compression, fmt.half_max
        self.w, self.h, self.keep, self.names = int(w), int(h), [], []
        layers = [(n.encode() if isinstance(n, str) else bytes(n), t, d, k, b) for n, t, d, k, b in layers]
        if sort:
            layers.sort(key=lambda entry: entry[0])
        if len(layers) > MAX_CHANNELS:
            raise ValueError(f"at most {MAX_CHANNELS} channels, got {len(layers)}")
        sources = {}
        for i, (name, type_, data, word, bottom_up) in enumerate(layers):
            addr, words, kind, keep = _plane(data, self.w, self.h)
            key = (addr, words, kind, bool(bottom_up))
            if key not in sources:
                if len(sources) == MAX_SOURCES:
                    raise ValueError(f"at most {MAX_SOURCES} sources")
                s = self.sources[len(sources)]
                s.d_data, s.words, s.kind, s.bottom_up = addr, words, kind, int(bool(bottom_up))
                sources[key] = len(sources)
                self.keep.append(keep)
            if len(name) > 31:
                raise ValueError(f"{name!r}: a channel's name is 1 ... 31 bytes")
            ch = self.channels[i]
            ch.name, ch.type, ch.source, ch.word = name, LAYER_TYPES.get(type_, type_), sources[key], int(word)
            self.names.append(name.decode("latin-1"))
        self.n_sources, self.n_channels = len(sources), len(layers)

    def address_bits(self, d_payload=0):
        """the OR of the payload's and every source's address: exr_layers_launch_geometry's argument"""
        bits = _ptr(d_payload).value or 0
        for s in self.sources[:self.n_sources]:
            bits |= s.d_data or 0
        return bits


def exr_layers_frame_bytes(layers, chunks=False):
    """bytes of one layered frame's payload; with chunks=True (bytes, n_chunks)"""
    n, k = C.c_size_t(0), C.c_int32(0)
    _call("rrt_exr_layers_frame_bytes", C.byref(layers), layers.w, layers.h, C.byref(n), C.byref(k))
    return (n.value, k.value) if chunks else n.value


def exr_layers_chunks(layers):
    """[(y, offset, bytes)] of every chunk of a layered frame, as exr_chunks"""
    out = []
    for i in range(exr_layers_frame_bytes(layers, chunks=True)[1]):
        y, off, n = C.c_int32(0), C.c_size_t(0), C.c_size_t(0)
        _call("rrt_exr_layers_chunk", C.byref(layers), layers.w, layers.h, i, C.byref(y), C.byref(off), C.byref(n))
        out.append((y.value, off.value, n.value))
    return out


def exr_layers_header(layers, fps_num=24, fps_den=1, cap=2048):
    """the layered file's header as bytes (rrt_exr_layers_header): exr_header's attributes around the layers' channel list"""
    buf, n = C.create_string_buffer(max(int(cap), 1)), C.c_size_t(0)
    _call("rrt_exr_layers_header", C.byref(layers), layers.w, layers.h, int(fps_num), int(fps_den), buf, int(cap), C.byref(n))
    return buf.raw[:n.value]


def exr_layers_launch_geometry(layers, address_bits=0):
    """how a layers launch is laid out (rrt_exr_layers_launch_geometry, host only), as exr_launch_geometry; "wide" is False (one
    sample per thread), 1 (16-byte stores throughout) or 2 (filtered 4-byte channels in 8-byte stores)"""
    out = (C.c_int32 * 8)()
    _call("rrt_exr_layers_launch_geometry", C.byref(layers), layers.w, layers.h, int(address_bits), C.byref(out))
    return {"threads": out[0], "block": (out[1], out[2]), "pixels": out[3], "grid": (out[4], out[5]), "wide": out[6] or False, "passes": out[7]}


def launch_exr_layers(d_payload, layers, stream=None):
    """The layers' device planes as the chunks of an EXR file into d_payload (exr_layers_frame_bytes bytes): one kernel on `stream`
    (default: torch's current stream)."""
    _call("rrt_launch_exr_layers", _ptr(d_payload), C.byref(layers), layers.w, layers.h, _stream(stream))


def exr_layers_host(layers):
    """the payload (uint8 array) of layers over HOST arrays, from the source the kernels run"""
    out = np.empty(exr_layers_frame_bytes(layers), np.uint8)
    _call("rrt_exr_layers_host", out.ctypes.data_as(C.c_void_p), C.byref(layers), layers.w, layers.h)
    return out


__all__ = ["ExrFormat", "exr_frame_bytes", "exr_chunks", "exr_header", "launch_exr_from_hdr", "exr_from_hdr_host", "exr_unfilter_host",
           "exr_launch_geometry", "ExrLayers", "exr_layers_frame_bytes", "exr_layers_chunks", "exr_layers_header",
           "exr_layers_launch_geometry", "launch_exr_layers", "exr_layers_host"]
