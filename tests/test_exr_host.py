"""EXR output without a GPU: librrt_exr.so's host entry points (include/rrt_exr.h) against the numpy restatement (tests/exr_ref.py)
byte for byte -- the payload at odd and chunk-straddling sizes, the half conversion on chosen inputs, the filter and its inverse, the
header and a whole file against bytes written out by hand -- the refusals, the EXR sink read back through the restatement's reader,
both drivers' new refusals, the exports, and the shared source under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/exr/exr_exerciser.cpp, a program of its own).  Everything is byte equality."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import exr_ref as xr
from test_driver_refusals import CPP, PY, TWO_RANKS, refused  # noqa: F401

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID = 1
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it
F = np.float32
WIDTHS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65)
HEIGHTS = (1, 2, 15, 16, 17, 33)
IDS = dict(ids=lambda f: "-".join(f) if isinstance(f, tuple) else None)


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


def _fmt(fmt, half_max=None):
    return _rrt().ExrFormat(fmt[0], fmt[1], half_max)


def test_module_exports_and_the_other_libraries_are_untouched():
    from relativisticraytracer_amd import _lib, exr, yuv
    rrt = _rrt()
    names = ["ExrFormat", "exr_frame_bytes", "exr_chunks", "exr_header", "launch_exr_from_hdr", "exr_from_hdr_host", "exr_unfilter_host",
             "exr_launch_geometry"]
    for name in names:
        assert name in rrt.__all__ and getattr(rrt, name) is getattr(exr, name), name
    assert not [n for n, _, _ in _lib.SYMBOLS + _lib.TEST_SYMBOLS + yuv.YUV_SYMBOLS if "exr" in n]      # a library of its own
    assert C.sizeof(exr.rrt_exr_format) == 16
    f = rrt.ExrFormat()
    assert (f.struct_size, f.type, f.compression, f.half_max) == (16, 1, 3, 65504.0)
    assert (exr.HALF, exr.FLOAT, exr.NONE, exr.ZIPS, exr.ZIP) == (1, 2, 0, 2, 3)          # the file format's own codes


def test_library_exports_exactly_what_the_header_declares():
    from relativisticraytracer_amd import build, exr, yuv
    from test_capi import declared_functions
    build.build_lib()

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    declared = declared_functions("rrt_exr.h")
    assert exported(build.EXR_LIB) == declared
    assert declared == sorted(n for n, _, _ in exr.EXR_SYMBOLS)
    assert all(re.match(r"rrt_(exr|launch_exr)_", n) for n in declared), declared
    # the other libraries are what their headers say, as before: no export moved
    assert exported(build.YUV_LIB) == declared_functions("rrt_yuv.h") == sorted(n for n, _, _ in yuv.YUV_SYMBOLS)
    assert not [n for n in exported(build.LIB) if "exr" in n]
    needed = subprocess.run(["readelf", "-d", build.EXR_LIB], capture_output=True, text=True, check=True).stdout
    assert "libz" not in needed                                # the library does not deflate


@pytest.mark.parametrize("fmt", xr.FORMATS, **IDS)
def test_host_payload_equals_the_restatement(fmt):
    rrt, rng = _rrt(), np.random.default_rng(len(fmt[0]) * 7 + len(fmt[1]))
    bps = 2 if fmt[0] == "half" else 4
    lines = xr.lines_per_chunk(fmt[1])
    for w in WIDTHS:
        for h in HEIGHTS:
            hdr = xr.hdr_frame(rng, w, h)
            got = rrt.exr_from_hdr_host(hdr, _fmt(fmt))
            n, k = rrt.exr_frame_bytes(_fmt(fmt), w, h, chunks=True)
            assert got.size == n == w * h * 3 * bps and k == -(-h // lines)
            assert np.array_equal(got, xr.payload(hdr, fmt)), (w, h)
            chunks = rrt.exr_chunks(_fmt(fmt), w, h)
            assert [c[0] for c in chunks] == list(range(0, h, lines))
            assert [c[2] for c in chunks] == [min(lines, h - y) * w * 3 * bps for y in range(0, h, lines)]
            assert [c[1] for c in chunks] == [y * w * 3 * bps for y in range(0, h, lines)]


def test_flip_and_channel_order():
    """a frame whose values name their own (buffer row, column, channel): the file is top-down, B then G then R per scanline"""
    rrt = _rrt()
    w, h = 5, 3
    frame = np.zeros((h, w, 4), F)
    for c in range(3):
        frame[..., c] = np.arange(h)[:, None] * 100 + np.arange(w)[None, :] * 10 + c          # exact in half
    frame[..., 3] = 777.0
    got = rrt.exr_from_hdr_host(frame, _fmt(("half", "none"))).view("<f2").reshape(h, 3, w).astype(np.float64)
    for y in range(h):
        for k, c in enumerate((2, 1, 0)):        # B, G, R
            assert got[y, k].tolist() == [(h - 1 - y) * 100 + x * 10 + c for x in range(w)]
    assert 777.0 not in got                      # alpha is not written


def _check_conversion(bits, src, half_max):
    """bits: the uint16 samples the library made of the float32 values src"""
    mag = np.abs(src)
    sign = (src.view(np.uint32) >> 16).astype(np.uint16) & 0x8000
    top = np.array([half_max], np.float16).view(np.uint16)[0]
    with np.errstate(over="ignore"):
        rounded = src.astype(np.float16)         # numpy's own round-to-nearest-even, subnormals kept
    plain = np.isfinite(src) & (np.abs(rounded.astype(np.float64)) <= half_max)
    assert np.array_equal(bits[plain], rounded[plain].view(np.uint16))
    clamped = ~np.isnan(src) & ~plain
    assert clamped.sum() > 0 and np.array_equal(bits[clamped], sign[clamped] | top)
    assert np.all(bits[np.isnan(src)] == 0)                                    # NaN -> +0, whatever its sign and payload
    assert not np.any((bits & 0x7C00) == 0x7C00)                               # never an inf or a NaN from us
    assert np.array_equal(bits, xr.half_bits(src, half_max))
    return mag


@pytest.mark.parametrize("half_max", [65504.0, 1024.0])
def test_half_conversion_on_chosen_inputs(half_max):
    rrt = _rrt()
    vals = xr.conversion_inputs()
    assert vals.size > 3 * 65536 + 6 * 0x7C00
    frame = xr.frame_of(vals, 256)
    got = rrt.exr_from_hdr_host(frame, _fmt(("half", "none"), half_max)).view("<u2").reshape(frame.shape[0], 3, 256)
    src = np.ascontiguousarray(frame[::-1, :, 2::-1].transpose(0, 2, 1))
    _check_conversion(got, src, half_max)
    # a few spelled out
    one = lambda v: int(rrt.exr_from_hdr_host(np.full((1, 1, 4), v, F), _fmt(("half", "none"), half_max)).view("<u2")[0])      # noqa: E731
    top = int(np.array([half_max], np.float16).view(np.uint16)[0])
    assert one(np.inf) == top and one(-np.inf) == 0x8000 | top and one(np.nan) == 0 and one(-np.nan) == 0
    assert one(0.0) == 0 and one(-0.0) == 0x8000 and one(3.4028234663852886e38) == top
    assert one(2.0 ** -24) == 1 and one(2.0 ** -25) == 0 and one(np.nextafter(F(2.0 ** -25), F(1))) == 1 and one(2.0 ** -26) == 0
    assert one(1.0) == 0x3C00 and one(1.0 + 2.0 ** -11) == 0x3C00 and one(1.0 + 3 * 2.0 ** -11) == 0x3C02       # ties to even
    if half_max == 65504.0:
        assert one(65504.0) == 0x7BFF and one(65519.996) == 0x7BFF and one(65520.0) == 0x7BFF and one(65536.0) == 0x7BFF
    else:
        assert one(1024.0) == 0x6400 and one(1024.4) == 0x6400 and one(1024.6) == 0x6400 and one(-2047.0) == 0xE400 and one(1023.5) == 0x63FF


def test_the_restatements_half_is_numpys_where_no_clamp_applies():
    vals = xr.conversion_inputs()
    ok = np.isfinite(vals) & (np.abs(vals) < 65520.0)
    assert ok.sum() > 200000
    assert np.array_equal(xr.half_bits(vals)[ok], vals[ok].astype(np.float16).view(np.uint16))


def test_float_samples_are_the_bits_as_they_are():
    rrt = _rrt()
    vals = xr.conversion_inputs()[-600:]
    frame = xr.frame_of(vals, 8)
    got = rrt.exr_from_hdr_host(frame, _fmt(("float", "none"))).view("<u4").reshape(frame.shape[0], 3, 8)
    assert np.array_equal(got, np.ascontiguousarray(frame[::-1, :, 2::-1].transpose(0, 2, 1)).view(np.uint32))


def test_filter_round_trip():
    rrt, rng = _rrt(), np.random.default_rng(17)
    sizes = list(range(2, 66, 2)) + [126, 128, 130, 1000, 4094, 4096]
    for n in sizes:
        x = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        f = xr.filter(x)
        assert len(f) == n and xr.unfilter(f) == x
        assert rrt.exr_unfilter_host(f).tobytes() == x
    # the definition, spelled out on six bytes: even offsets, odd offsets, then differences + 128 across the seam
    assert xr.filter(bytes([10, 200, 13, 190, 9, 255])) == bytes([10, 131, 124, (200 - 9 + 128) & 255, 118, 193])


HEADER_2x1 = (
    b"\x76\x2f\x31\x01" b"\x02\x00\x00\x00"
    b"channels\0" b"chlist\0" b"\x37\x00\x00\x00"
    b"B\0" b"\x01\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\x01\0\0\0"
    b"G\0" b"\x01\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\x01\0\0\0"
    b"R\0" b"\x01\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\x01\0\0\0"
    b"\0"
    b"compression\0" b"compression\0" b"\x01\0\0\0" b"\0"
    b"dataWindow\0" b"box2i\0" b"\x10\0\0\0" b"\0\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\0\0\0\0"
    b"displayWindow\0" b"box2i\0" b"\x10\0\0\0" b"\0\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\0\0\0\0"
    b"lineOrder\0" b"lineOrder\0" b"\x01\0\0\0" b"\0"
    b"pixelAspectRatio\0" b"float\0" b"\x04\0\0\0" b"\0\0\x80\x3f"
    b"screenWindowCenter\0" b"v2f\0" b"\x08\0\0\0" b"\0\0\0\0" b"\0\0\0\0"
    b"screenWindowWidth\0" b"float\0" b"\x04\0\0\0" b"\0\0\x80\x3f"
    b"chromaticities\0" b"chromaticities\0" b"\x20\0\0\0"
    b"\x0a\xd7\x23\x3f" b"\xc3\xf5\xa8\x3e" b"\x9a\x99\x99\x3e" b"\x9a\x99\x19\x3f" b"\x9a\x99\x19\x3e" b"\x8f\xc2\x75\x3d"
    b"\x37\x1a\xa0\x3e" b"\xb0\x72\xa8\x3e"
    b"framesPerSecond\0" b"rational\0" b"\x08\0\0\0" b"\x18\0\0\0" b"\x01\0\0\0"
    b"software\0" b"string\0" b"\x19\0\0\0" b"relativisticraytracer_amd"
    b"\0")


def test_header_and_file_of_a_2x1_frame_written_out_by_hand(tmp_path):
    from relativisticraytracer_amd import sinks
    rrt, fmt = _rrt(), ("half", "none")
    assert rrt.exr_header(_fmt(fmt), 2, 1) == HEADER_2x1 == xr.header(fmt, 2, 1)
    assert rrt.exr_header(_fmt(fmt), 2, 1, cap=len(HEADER_2x1)) == HEADER_2x1             # an exact fit is enough
    with pytest.raises(rrt.RRTError) as e:
        rrt.exr_header(_fmt(fmt), 2, 1, cap=len(HEADER_2x1) - 1)
    assert e.value.status == INVALID and "cap" in str(e.value)
    assert rrt.exr_header(_fmt(("float", "zip")), 1920, 1080, 30000, 1001) == xr.header(("float", "zip"), 1920, 1080, 30000, 1001)
    # pixel 0: R 1.5, G 0.25, B -3; pixel 1: R 100, G 2, B 0.75 -- the scanline is B B, G G, R R, as little-endian halves
    frame = np.array([[[1.5, 0.25, -3.0, 1.0], [100.0, 2.0, 0.75, 1.0]]], F)
    scanline = b"\x00\xc2\x00\x3a" b"\x00\x34\x00\x40" b"\x00\x3e\x40\x56"
    whole = (HEADER_2x1 + struct.pack("<Q", len(HEADER_2x1) + 8)        # the offset table: one chunk, right behind it
             + b"\0\0\0\0" + b"\x0c\0\0\0" + scanline)                  # y = 0, 12 bytes
    sink = sinks.EXRSink(str(tmp_path / "one.exr"), 2, 1, 24, _fmt(fmt))
    sink.write(rrt.exr_from_hdr_host(frame, _fmt(fmt)))
    sink.close()
    assert (tmp_path / "one.exr").read_bytes() == whole == xr.write_file(frame, fmt)
    back = xr.read_file(whole)
    assert back["channels"]["R"].tolist() == [[1.5, 100.0]] and back["channels"]["B"].tolist() == [[-3.0, 0.75]]
    assert back["attributes"]["framesPerSecond"] == ("rational", struct.pack("<iI", 24, 1))
    assert back["attributes"]["software"] == ("string", b"relativisticraytracer_amd")


def _half_rounded(hdr):
    """what a half file of this frame holds, as float16 channels, top-down"""
    s = xr.samples(hdr, "half").view(np.float16)
    return {"B": s[:, 0], "G": s[:, 1], "R": s[:, 2]}


@pytest.mark.parametrize("fmt", xr.FORMATS, **IDS)
def test_sink_files_read_back_and_equal_the_restatements(fmt, tmp_path):
    from relativisticraytracer_amd import sinks
    rrt, rng = _rrt(), np.random.default_rng(23)
    w, h = 19, 17                                         # with zip the last chunk is one row
    frames = [np.exp2(rng.uniform(-10.0, 4.0, (h, w, 4))).astype(F) for _ in range(3)]
    files = {}
    for threads in (1, 4):
        pattern = str(tmp_path / f"t{threads}" / "f.%04d.exr")
        os.makedirs(os.path.dirname(pattern))
        sink = sinks.EXRSink(pattern, w, h, 24, _fmt(fmt), level=4, threads=threads)
        assert sink.threads == threads
        for f in frames:
            sink.write(rrt.exr_from_hdr_host(f, _fmt(fmt)))
        with pytest.raises(ValueError):
            sink.write(np.zeros(sink.frame_bytes - 1, np.uint8))
        sink.close()
        names = sorted(os.listdir(os.path.dirname(pattern)))
        assert names == ["f.0001.exr", "f.0002.exr", "f.0003.exr"]          # and no .tmp file is left
        files[threads] = [open(os.path.join(os.path.dirname(pattern), n), "rb").read() for n in names]
    assert files[1] == files[4]
    for f, data in zip(frames, files[1]):
        assert data == xr.write_file(f, fmt, 24, 4)
        back = xr.read_file(data)
        assert (back["width"], back["height"], back["type"], back["compression"]) == (w, h, fmt[0], fmt[1])
        want = _half_rounded(f) if fmt[0] == "half" else {"B": f[::-1, :, 2], "G": f[::-1, :, 1], "R": f[::-1, :, 0]}
        for c in "BGR":
            assert np.array_equal(back["channels"][c].view(np.uint16 if fmt[0] == "half" else np.uint32),
                                  np.ascontiguousarray(want[c]).view(np.uint16 if fmt[0] == "half" else np.uint32)), c
        if fmt[1] == "zip":
            assert struct.unpack_from("<i", data, struct.unpack_from("<Q", data, len(xr.header(fmt, w, h)) + 8)[0])[0] == 16      # chunk 1: y = 16


def test_sink_stores_raw_what_deflate_does_not_shrink(tmp_path):
    """random bits as floats do not deflate: the chunks are stored raw, un-filtered, and a reader sees size == n"""
    from relativisticraytracer_amd import sinks
    rrt, rng = _rrt(), np.random.default_rng(29)
    w, h = 24, 17
    frame = rng.integers(0, 2 ** 32, (h, w, 4), dtype=np.uint64).astype(np.uint32).view(F)
    for fmt in (("float", "zip"), ("float", "zips")):
        path = tmp_path / f"noise_{fmt[1]}.exr"
        sink = sinks.EXRSink(str(path), w, h, 24, _fmt(fmt), threads=2)
        sink.write(rrt.exr_from_hdr_host(frame, _fmt(fmt)))
        sink.close()
        data = path.read_bytes()
        assert data == xr.write_file(frame, fmt)
        back = xr.read_file(data)
        n_chunks = -(-h // xr.lines_per_chunk(fmt[1]))
        assert back["raw_chunks"] == n_chunks == sink.stored_raw
        assert np.array_equal(back["channels"]["G"].view(np.uint32), frame[::-1, :, 1].view(np.uint32))
        with pytest.raises(ValueError):          # a plain name holds one frame
            sinks.EXRSink(str(path), w, h, 24, _fmt(fmt)).write(np.zeros(1, np.uint8))
    plain = sinks.EXRSink(str(tmp_path / "plain.exr"), w, h, 24, _fmt(("half", "zip")))
    plain.write(rrt.exr_from_hdr_host(frame, _fmt(("half", "zip"))))
    with pytest.raises(ValueError):
        plain.write(rrt.exr_from_hdr_host(frame, _fmt(("half", "zip"))))
    plain.close()
    with pytest.raises(ValueError):
        sinks.EXRSink(str(tmp_path / "a.%d.%04d.exr"), w, h)
    assert sinks.frame_name("f.%04d.exr", 7) == "f.0007.exr" and sinks.frame_name("f.%d.exr", 12) == "f.12.exr"
    assert sinks.frame_fields("plain.exr") == 0 and sinks.frame_fields("a%db%03d") == 2


def test_sink_pool_is_sized_by_the_cpus_this_process_may_use():
    from relativisticraytracer_amd import sinks
    sink = sinks.EXRSink("unused.%d.exr", 8, 64, 24, _fmt(("half", "zip")))
    assert sink.threads == min(16, len(os.sched_getaffinity(0)))
    sink.close()


def _bad_formats():
    rrt = _rrt()
    out = []
    for field, value in (("type", 0), ("type", 3), ("compression", 1), ("compression", 4), ("compression", -1), ("struct_size", 12),
                         ("half_max", 0.0), ("half_max", -1.0), ("half_max", float("inf")), ("half_max", float("nan")),
                         ("half_max", 65520.0), ("half_max", 1024.5)):
        f = rrt.ExrFormat()
        setattr(f, field, value)
        out.append(f)
    return out


def test_refusals_without_a_device():
    """every refusal of include/rrt_exr.h, with made-up device addresses: a launch that passed the checks would fault on them"""
    from relativisticraytracer_amd import exr
    rrt, lib = _rrt(), exr.load()
    ok = rrt.ExrFormat()
    w, h = 64, 48
    out, src = FAKE, FAKE + (1 << 32)
    launch = lib.rrt_launch_exr_from_hdr
    n, k, y = C.c_size_t(0), C.c_int32(0), C.c_int32(0)
    g, head = (C.c_int32 * 8)(), (C.c_char * 1024)()

    def said():
        return lib.rrt_exr_last_error().decode()
    assert launch(None, src, w, h, C.byref(ok), None) == INVALID and "NULL" in said()
    assert launch(out, None, w, h, C.byref(ok), None) == INVALID
    assert launch(out, src, w, h, None, None) == INVALID and "fmt" in said()
    for bw, bh in ((0, h), (w, 0), (-1, h), (w, -5)):
        assert launch(out, src, bw, bh, C.byref(ok), None) == INVALID and "width" in said(), (bw, bh)
    assert launch(out, src, 22369622, 16, C.byref(ok), None) == INVALID and "2^31" in said()          # a chunk of 2^31 bytes
    for f in _bad_formats():
        assert launch(out, src, w, h, C.byref(f), None) == INVALID and said()
        assert lib.rrt_exr_frame_bytes(C.byref(f), w, h, C.byref(n), C.byref(k)) == INVALID
        assert lib.rrt_exr_chunk(C.byref(f), w, h, 0, C.byref(y), C.byref(n), C.byref(n)) == INVALID
        assert lib.rrt_exr_launch_geometry(C.byref(f), w, h, 0, C.byref(g)) == INVALID
        assert lib.rrt_exr_header(C.byref(f), w, h, 24, 1, head, 1024, C.byref(n)) == INVALID
    for off in (1, 2, 3):
        assert launch(out, src + off, w, h, C.byref(ok), None) == INVALID and "aligned" in said()      # d_hdr: 4-byte aligned
    # an output that overlaps the input: its first byte, its last, and the input inside the output
    total = rrt.exr_frame_bytes(ok, w, h)
    assert launch(src, src, w, h, C.byref(ok), None) == INVALID and "overlaps" in said()
    assert launch(src + w * h * 16 - 16, src, w, h, C.byref(ok), None) == INVALID
    assert launch(src - total + 16, src, w, h, C.byref(ok), None) == INVALID
    for bw, bh in ((0, h), (w, 0)):
        assert lib.rrt_exr_frame_bytes(C.byref(ok), bw, bh, C.byref(n), C.byref(k)) == INVALID
        assert lib.rrt_exr_launch_geometry(C.byref(ok), bw, bh, 0, C.byref(g)) == INVALID
        assert lib.rrt_exr_header(C.byref(ok), bw, bh, 24, 1, head, 1024, C.byref(n)) == INVALID
    assert lib.rrt_exr_frame_bytes(C.byref(ok), w, h, None, None) == INVALID
    assert lib.rrt_exr_frame_bytes(C.byref(ok), w, h, C.byref(n), None) == 0 and n.value == total and said() == ""
    assert lib.rrt_exr_chunk(C.byref(ok), w, h, 3, C.byref(y), C.byref(n), C.byref(n)) == INVALID      # 48 rows: chunks 0, 1, 2
    assert lib.rrt_exr_chunk(C.byref(ok), w, h, -1, C.byref(y), C.byref(n), C.byref(n)) == INVALID
    assert lib.rrt_exr_chunk(C.byref(ok), w, h, 0, None, C.byref(n), C.byref(n)) == INVALID
    assert lib.rrt_exr_launch_geometry(C.byref(ok), w, h, 0, None) == INVALID
    assert lib.rrt_exr_header(C.byref(ok), w, h, 24, 1, None, 1024, C.byref(n)) == INVALID
    assert lib.rrt_exr_header(C.byref(ok), w, h, 24, 1, head, 1024, None) == INVALID
    for num, den in ((0, 1), (24, 0), (-24, 1)):
        assert lib.rrt_exr_header(C.byref(ok), w, h, num, den, head, 1024, C.byref(n)) == INVALID
    assert lib.rrt_exr_format_default(None) == INVALID
    buf = np.zeros(4 * 4 * 16 + 64, np.uint8)
    p = buf.ctypes.data
    host = lib.rrt_exr_from_hdr_host
    assert host(None, p, 4, 4, C.byref(ok)) == INVALID and host(p, None, 4, 4, C.byref(ok)) == INVALID
    assert host(p, p, 4, 4, C.byref(ok)) == INVALID and host(p + 8, p, 4, 4, C.byref(ok)) == INVALID
    assert host(p, p + 1024, 0, 4, C.byref(ok)) == INVALID
    un = lib.rrt_exr_unfilter_host
    assert un(None, p, 8) == INVALID and un(p, None, 8) == INVALID and un(p, p + 64, 7) == INVALID and un(p, p + 64, 0) == INVALID
    assert un(p, p + 4, 8) == INVALID
    assert not buf.any()                              # nothing was written
    with pytest.raises(rrt.RRTError) as e:
        rrt.launch_exr_from_hdr(out, src + 2, w, h)
    assert e.value.status == INVALID and "rrt_launch_exr_from_hdr" in str(e.value) and "4-byte aligned" in str(e.value)
    half_max_ok = rrt.ExrFormat(half_max=2.0 ** -24)   # the smallest positive half is one
    assert rrt.exr_frame_bytes(half_max_ok, 1, 1) == 6


# ---- the shared source under the sanitizers

@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/exr/exr_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("exr")
    exe = str(d / "exr_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "exr", "exr_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case, text):
        path = d / (case + ".txt")
        path.write_text(text)
        r = subprocess.run([exe, case, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip().endswith(case + " ok"), (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.strip().splitlines()[:-1]
    return run


def test_shared_source_under_sanitizers_equals_the_restatement(exerciser):
    """odd sizes, input and output buffers sized exactly, through the source the library's host entry points and kernels run"""
    rng = np.random.default_rng(31)
    cases, text = [], []
    for fmt in xr.FORMATS:
        for w, h, half_max in ((1, 1, 65504.0), (1, 2, 65504.0), (2, 1, 1024.0), (3, 17, 65504.0), (9, 33, 65504.0), (65, 16, 2.0)):
            hdr = xr.hdr_frame(rng, w, h)
            cases += [xr.payload(hdr, fmt + (half_max,)).tobytes().hex(), xr.header(fmt, w, h).hex()]
            bits = int(np.array([half_max], F).view(np.uint32)[0])
            text.append(f"{xr.TYPES[fmt[0]]} {xr.COMPRESSIONS[fmt[1]]} {bits:x} {w} {h}\n"
                        + " ".join(f"{v:x}" for v in hdr.ravel().view(np.uint32)) + "\n")
    lines = exerciser("frames", "".join(text))
    assert lines == cases


def test_shared_source_refusals_under_sanitizers(exerciser):
    assert exerciser("refusals", "") == []


# ---- the drivers' refusals: a table of its own (tests/test_driver_refusals.py's is closed), same conventions

NEEDED = "--exr-type / --exr-compression / --exr-level need --exr PATTERN"
NO_GLOW = "--exr reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow"
NO_FIELD = "--exr PATTERN needs a frame field (%04d) when --frames > 1: the frames would overwrite one another"
EXR_ROWS = [
    (["--exr-type", "float"], None, NEEDED),
    (["--exr-compression", "none"], None, NEEDED),
    (["--exr-level", "6"], None, NEEDED),
    (["--exr-type", "double"], None, NEEDED),
    (["--exr", "f.%04d.exr", "--exr-type", "double"], None, "--exr-type half | float"),
    (["--exr", "f.%04d.exr", "--exr-compression", "piz"], None, "--exr-compression none | zips | zip"),
    (["--exr", "f.%04d.exr", "--exr-level", "0"], None, "--exr-level 1 ... 9"),
    (["--exr", "f.%04d.exr", "--exr-level", "10"], None, "--exr-level 1 ... 9"),
    (["--exr", "f.%04d.exr", "--exr-level", "fast"], None, "--exr-level 1 ... 9"),
    (["--exr", "f.%04d.exr", "--glow", "0.25"], None, NO_GLOW),
    (["--exr", "f.%04d.exr", "--exposure", "1", "--glow", "0.25"], None, NO_GLOW),
    (["--exr", "f.exr", "--frames", "2"], None, NO_FIELD),
    (["--exr", "f.exr"], None, NO_FIELD),                                   # --frames defaults to 24
    (["--exr", "f.%d.%04d.exr"], None, "--exr PATTERN: one frame field (%d or %0Nd)"),
    (["--exr", "f.%04d.exr", "--frames", "3", "--out", "f.0003.exr"], None, "--exr and --out name the same file"),
    (["--exr", "f.%04d.exr", "--frames", "3", "--out", "./sub/../f.0001.exr"], None, "--exr and --out name the same file"),
    (["--exr", "f.exr", "--frames", "1", "--out", "f.exr"], None, "--exr and --out name the same file"),
    (["--exr", "f.%d.y4m", "--frames", "12", "--y4m", "f.12.y4m"], None, "--exr and --y4m name the same file"),
]
PY_ONLY = [(["--exr", "f.%04d.exr"], TWO_RANKS, "--exr: one GPU only (WORLD_SIZE > 1)")]
CPP_ONLY = [(["--exr", "f.%04d.exr", "--gpus", "2"], None, "--exr: one GPU only (--gpus 1)"),
            (["--exr", "f.%04d.exr", "--force-collective"], None, "--exr: one GPU only (--gpus 1)"),
            (["--exr", "f.%04d.exr", "--exr-type"], None, "--exr-type half | float")]
ROW_IDS = dict(ids=lambda a: " ".join(a) if isinstance(a, list) else "")


@pytest.mark.parametrize("args,env,msg", EXR_ROWS + PY_ONLY, **ROW_IDS)
def test_python_driver_refuses(args, env, msg):
    refused(PY, args, msg, env)


@pytest.mark.parametrize("args,env,msg", EXR_ROWS + CPP_ONLY, **ROW_IDS)
def test_cpp_driver_refuses(args, env, msg):
    refused(CPP, args, "usage: " + msg, env)
