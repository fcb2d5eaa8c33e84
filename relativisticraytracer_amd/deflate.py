"""ctypes loader and wrappers for librrt_deflate.so (C ABI: include/rrt_deflate.h): raw deflate streams -- Huffman codes and distance-1
run lengths, in independent byte-aligned fragments of 32 KiB -- made on the device from bytes that are there already (launch_deflate),
or on the host from the same source (deflate_host), with the host queries: the cut and the buffers (deflate_plan), the launch's
layout (deflate_launch_geometry) and the code-length builder on its own (deflate_code_lengths).  sinks.PNGSink.write_streams wraps
the streams of a PNG payload into a file.

A library of its own with a loader of its own: nothing here is part of _lib.SYMBOLS.  Calls go through _lib.call(..., lib=...), so a
refusal raises the same RRTError as everywhere else, with the library's reason.  No fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import _ptr, _stream      # the package's own argument rules: a device tensor or a raw address; a stream or torch's current one
from ._lib import RRTError

LIB_PATH = os.path.join(_lib.PKG, "lib", "librrt_deflate.so")
SEGMENT_BYTES, THREADS, CHUNK_BYTES, LL_SYMBOLS, MAX_SYMBOLS = 32768, 256, 128, 286, 288      # include/rrt_deflate.h's constants

_vp, _i = C.c_void_p, C.c_int
_sz = C.POINTER(C.c_size_t)
# every symbol include/rrt_deflate.h declares: (name, restype, argtypes)
DEFLATE_SYMBOLS = [
    ("rrt_deflate_plan", _i, [C.c_size_t, C.c_size_t, _sz, _sz, _sz, _sz]),
    ("rrt_deflate_launch_geometry", _i, [C.c_size_t, C.c_size_t, C.c_size_t, C.POINTER(C.c_int32 * 12)]),
    ("rrt_deflate_code_lengths_host", _i, [_vp, _i, _i, _vp, C.POINTER(C.c_int32)]),
    ("rrt_launch_deflate", _i, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _i, _vp]),
    ("rrt_deflate_host", _i, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, _i, _sz]),
    ("rrt_deflate_last_error", C.c_char_p, []),
]

_deflate = None


def load():
    """Load librrt_deflate.so.  Raises if it has not been built (no fallback)."""
    global _deflate
    if _deflate is not None:
        return _deflate
    if not os.path.exists(LIB_PATH):
        raise RRTError(-1, "librrt_deflate.so is missing", f"expected {LIB_PATH}; run `python -m relativisticraytracer_amd.build`")
    try:  # share torch's HIP runtime when torch is in the process, as _lib.load does
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    _lib._bind(lib, DEFLATE_SYMBOLS)
    _deflate = lib
    return lib


def _call(name, *args):
    lib = load()
    try:
        _lib.call(name, *args, lib=lib)
    except RRTError as e:
        why = lib.rrt_deflate_last_error().decode()
        if e.status == 3:       # RRT_ERR_HIP: the message is this library's, not librrt_hip.so's
            raise RRTError(3, name, "a HIP runtime call failed -- " + why) from None
        if e.status == 1 and why:
            raise RRTError(1, name, why) from None
        raise


def deflate_plan(n, stream_bytes):
    """the cut and the buffers of n bytes in streams of stream_bytes: {"streams", "segments", "out_bound", "scratch_bytes"}"""
    v = [C.c_size_t(0) for _ in range(4)]
    _call("rrt_deflate_plan", int(n), int(stream_bytes), *[C.byref(x) for x in v])
    return dict(zip(("streams", "segments", "out_bound", "scratch_bytes"), (x.value for x in v)))


def deflate_launch_geometry(n, stream_bytes, address_bits=0):
    """how a launch of this size is laid out (rrt_deflate_launch_geometry, host only).  address_bits: the input's address (0: 16-byte
    aligned).  head_bytes / tail_bytes: what is loaded byte by byte at the input's ends; wide_loads: its whole 16-byte words."""
    out = (C.c_int32 * 12)()
    _call("rrt_deflate_launch_geometry", int(n), int(stream_bytes), int(address_bits), C.byref(out))
    kernels = {name: {"threads": out[3 * k], "grid": out[3 * k + 1], "lds_bytes": out[3 * k + 2]}
               for k, name in enumerate(("segments", "offsets", "gather"))}
    return dict(kernels, head_bytes=out[9], tail_bytes=out[10], wide_loads=out[11])


def deflate_code_lengths(counts, limit):
    """step 4 of the definition on its own: (lengths as a uint8 array, halvings) of a Huffman code over len(counts) symbols whose
    longest code is `limit` bits"""
    c = np.ascontiguousarray(counts, np.uint32)
    out, halvings = np.zeros(c.size, np.uint8), C.c_int32(0)
    _call("rrt_deflate_code_lengths_host", c.ctypes.data_as(C.c_void_p), int(c.size), int(limit), out.ctypes.data_as(C.c_void_p), C.byref(halvings))
    return out, halvings.value


def launch_deflate(d_out, d_stream_sizes, d_scratch, d_src, n, stream_bytes, finish=True, stream=None):
    """The n bytes at d_src as raw deflate streams of stream_bytes input bytes each: into d_out back to back (deflate_plan's out_bound
    bytes at the most), their sizes into d_stream_sizes (one uint32 per stream); d_scratch: deflate_plan's scratch_bytes, 16-byte
    aligned.  finish: the last stream ends the deflate stream; every other one ends as a sync flush does.  Tensors or raw device
    addresses; three kernels on `stream` (default: torch's current stream), capturable."""
    _call("rrt_launch_deflate", _ptr(d_out), _ptr(d_stream_sizes), _ptr(d_scratch), _ptr(d_src),
          int(n), int(stream_bytes), int(bool(finish)), _stream(stream))


def deflate_host(data, stream_bytes, finish=True):
    """the same streams on the host, from the source the kernels run: a list of bytes objects, one per stream"""
    a = np.ascontiguousarray(np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8).ravel()
    plan = deflate_plan(a.size, stream_bytes)
    out, sizes, total = np.empty(plan["out_bound"], np.uint8), np.empty(plan["streams"], np.uint32), C.c_size_t(0)
    _call("rrt_deflate_host", out.ctypes.data_as(C.c_void_p), sizes.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p) if a.size else 0,
          int(a.size), int(stream_bytes), int(bool(finish)), C.byref(total))
    assert int(sizes.sum()) == total.value
    ends = np.cumsum(sizes.astype(np.int64))
    return [out[e - s:e].tobytes() for s, e in zip(sizes.tolist(), ends.tolist())]


__all__ = ["deflate_plan", "deflate_launch_geometry", "deflate_code_lengths", "launch_deflate", "deflate_host"]
