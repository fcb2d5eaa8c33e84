"""EXR data layers without a GPU: librrt_exr.so's layers entry points (include/rrt_exr.h, the second block comment) against the numpy
restatement (tests/exr_layers_ref.py) byte for byte -- payload, chunk table and header over odd and chunk-straddling sizes and five
kinds of layer set --, the {B, G, R} identity against the three existing functions in all six formats, the integer conversions on
chosen inputs, a header written out by hand, the EXR sink with layers read back through the restatement's reader, every refusal with
made-up device addresses, and the shared source under AddressSanitizer and UndefinedBehaviorSanitizer
(tests/exr/exr_layers_exerciser.cpp, a program of its own).  Everything is byte equality."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import exr_layers_ref as lr
import exr_ref as xr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID = 1
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it
F = np.float32
WIDTHS = (1, 2, 7, 8, 9, 16, 24, 65)
HEIGHTS = (1, 2, 15, 16, 17, 33)
SETS = ("bgr_half", "all_half", "all_float", "mixed", "uint")


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


def test_module_exports():
    from relativisticraytracer_amd import exr
    rrt = _rrt()
    for name in ("ExrLayers", "exr_layers_frame_bytes", "exr_layers_chunks", "exr_layers_header", "exr_layers_launch_geometry",
                 "launch_exr_layers", "exr_layers_host"):
        assert name in rrt.__all__ and getattr(rrt, name) is getattr(exr, name), name
    assert (exr.UINT, exr.SRC_F32, exr.SRC_I32, exr.MAX_SOURCES, exr.MAX_CHANNELS) == (0, 0, 1, 8, 16)
    assert (C.sizeof(exr.rrt_exr_source), C.sizeof(exr.rrt_exr_channel), C.sizeof(exr.rrt_exr_layers)) == (24, 48, 24 + 8 * 24 + 16 * 48)
    empty = exr.rrt_exr_layers()
    assert exr.load().rrt_exr_layers_default(C.byref(empty)) == 0
    assert (empty.struct_size, empty.compression, empty.half_max, empty.n_sources, empty.n_channels) == (984, 3, 65504.0, 0, 0)


@pytest.mark.parametrize("compression", lr.COMPRESSIONS)
@pytest.mark.parametrize("set_name", SETS)
def test_host_entry_points_equal_the_restatement(set_name, compression):
    rrt, rng = _rrt(), np.random.default_rng(len(set_name) * 11 + len(compression))
    channels = lr.LAYER_SETS[set_name]
    for w in WIDTHS:
        for h in HEIGHTS:
            planes = lr.random_planes(rng, w, h)
            L = lr.api_layers(rrt, channels, planes, w, h, compression)
            assert L.names == [c[0] for c in lr.ordered(channels)]              # ExrLayers sorts for the caller
            want = lr.payload(channels, planes, compression)
            got = rrt.exr_layers_host(L)
            n, k = rrt.exr_layers_frame_bytes(L, chunks=True)
            assert got.size == n == want.size == w * h * lr.bytes_per_pixel(channels) and k == -(-h // xr.lines_per_chunk(compression))
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (w, h, bad.size, bad[:8].tolist())
            assert rrt.exr_layers_chunks(L) == lr.chunk_table(channels, w, h, compression), (w, h)
            assert rrt.exr_layers_header(L) == lr.header(channels, w, h, compression), (w, h)
    assert rrt.exr_layers_header(lr.api_layers(rrt, channels, planes, w, h, compression), 30000, 1001) == lr.header(channels, w, h, compression, 30000, 1001)


@pytest.mark.parametrize("fmt", xr.FORMATS, ids="-".join)
def test_bgr_layers_are_the_existing_functions_bytes(fmt):
    """{B, G, R} from one 4-word bottom-up F32 source, words 2, 1, 0: payload, chunk table and header of the dedicated entry points"""
    rrt, rng = _rrt(), np.random.default_rng(41)
    for w, h, half_max in ((1, 1, None), (7, 3, None), (8, 16, None), (24, 17, 1024.0), (65, 33, None)):
        hdr = xr.hdr_frame(rng, w, h)
        f = rrt.ExrFormat(fmt[0], fmt[1], half_max)
        L = rrt.ExrLayers(f, w, h, [("R", fmt[0], hdr, 0, True), ("G", fmt[0], hdr, 1, True), ("B", fmt[0], hdr, 2, True)])
        assert (L.n_sources, L.n_channels, L.names) == (1, 3, ["B", "G", "R"])
        assert np.array_equal(rrt.exr_layers_host(L), rrt.exr_from_hdr_host(hdr, f)), (w, h)
        assert np.array_equal(rrt.exr_layers_host(L), xr.payload(hdr, fmt + ((half_max,) if half_max else ()))), (w, h)
        assert rrt.exr_layers_frame_bytes(L, chunks=True) == rrt.exr_frame_bytes(f, w, h, chunks=True)
        assert rrt.exr_layers_chunks(L) == rrt.exr_chunks(f, w, h)
        assert rrt.exr_layers_header(L, 30000, 1001) == rrt.exr_header(f, w, h, 30000, 1001) == xr.header(fmt, w, h, 30000, 1001)


def _one_channel(rrt, values, type_, half_max=None):
    """the stored samples of a (1, n) plane through a single-channel NONE layout"""
    a = np.ascontiguousarray(values).reshape(1, -1)
    L = rrt.ExrLayers(rrt.ExrFormat("half", "none", half_max), a.shape[1], 1, [("v", type_, a, 0, False)])
    return rrt.exr_layers_host(L).view("<u2" if type_ == "half" else "<u4")


def test_integer_conversions_on_chosen_inputs():
    rrt = _rrt()
    i32 = lambda *v: np.array(v, np.int64).astype(np.int32)      # noqa: E731
    top = 2 ** 31 - 1
    # I32 -> HALF: exact up to 2048, ties to even beyond, the clamp from 65520 on, the negatives alike
    vals = i32(0, 1, -1, 2047, 2048, 2049, 2050, 2051, 4097, 4098, 4099, 65504, 65519, 65520, 65536, top, -2047, -2049, -65504, -65520, -top - 1)
    got = _one_channel(rrt, vals, "half")
    want = [0.0, 1.0, -1.0, 2047.0, 2048.0, 2048.0, 2050.0, 2052.0, 4096.0, 4096.0, 4100.0, 65504.0, 65504.0, 65504.0, 65504.0, 65504.0,
            -2047.0, -2048.0, -65504.0, -65504.0, -65504.0]
    assert got.view(np.float16).astype(np.float64).tolist() == want
    assert np.array_equal(got, lr.convert(vals, "half"))
    assert _one_channel(rrt, i32(2047, 2048, top), "half", 1024.0).view(np.float16).tolist() == [1024.0, 1024.0, 1024.0]
    # I32 -> FLOAT: round to nearest even at 2^24 +- 1 and at the top
    vals = i32(2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 2, 2 ** 24 + 3, -(2 ** 24) - 1, top, top - 64, -top - 1, 0, -1)
    got = _one_channel(rrt, vals, "float")
    assert got.view(F).astype(np.float64).tolist() == [16777215.0, 16777216.0, 16777216.0, 16777218.0, 16777220.0, -16777216.0, 2147483648.0,
                                                       2147483520.0, -2147483648.0, 0.0, -1.0]
    assert np.array_equal(got, lr.convert(vals, "float")) and got[-2] == 0                     # +0, not -0
    # I32 -> UINT: a negative value becomes 0
    vals = i32(-1, 0, top, -top - 1, 1, 70000)
    got = _one_channel(rrt, vals, "uint")
    assert got.tolist() == [0, 0, top, 0, 1, 70000] and np.array_equal(got, lr.convert(vals, "uint"))
    # F32 -> HALF: the list the half conversion is pinned on, through a layer; F32 -> FLOAT: the bits as they are
    src = xr.conversion_inputs()
    for half_max in (65504.0, 1024.0):
        assert np.array_equal(_one_channel(rrt, src, "half", half_max), xr.half_bits(src, half_max))
    assert np.array_equal(_one_channel(rrt, src, "float"), src.view(np.uint32))


HEADER_2x1 = (
    b"\x76\x2f\x31\x01" b"\x02\x00\x00\x00"
    b"channels\0" b"chlist\0" b"\x29\x00\x00\x00"
    b"R\0" b"\x01\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\x01\0\0\0"
    b"steps\0" b"\x00\0\0\0" b"\0\0\0\0" b"\x01\0\0\0" b"\x01\0\0\0"
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


def test_header_and_file_of_a_2x1_two_channel_frame_written_out_by_hand(tmp_path):
    """one HALF and one UINT channel: R 1.5, 100 from a bottom-up HDR plane; steps -7 (stored as 0), 3 from a top-down int32 plane"""
    from relativisticraytracer_amd import sinks
    rrt = _rrt()
    hdr = np.array([[[1.5, 0.25, -3.0, 1.0], [100.0, 2.0, 0.75, 1.0]]], F)
    steps = np.array([[-7, 3]], np.int32)
    f = rrt.ExrFormat("half", "none")
    L = rrt.ExrLayers(f, 2, 1, [("steps", "uint", steps, 0, False), ("R", "half", hdr, 0, True)])
    assert rrt.exr_layers_header(L) == HEADER_2x1
    assert rrt.exr_layers_header(L, cap=len(HEADER_2x1)) == HEADER_2x1              # an exact fit is enough
    with pytest.raises(rrt.RRTError) as e:
        rrt.exr_layers_header(L, cap=len(HEADER_2x1) - 1)
    assert e.value.status == INVALID and "cap" in str(e.value)
    scanline = b"\x00\x3e\x40\x56" b"\0\0\0\0\x03\0\0\0"
    whole = HEADER_2x1 + struct.pack("<Q", len(HEADER_2x1) + 8) + b"\0\0\0\0" + b"\x0c\0\0\0" + scanline
    sink = sinks.EXRSink(str(tmp_path / "one.exr"), 2, 1, 24, f, layers=L)
    sink.write(rrt.exr_layers_host(L))
    sink.close()
    channels, planes = [("R", "half", "hdr", 0), ("steps", "uint", "steps", 0)], {"hdr": (hdr, True), "steps": (steps, False)}
    assert (tmp_path / "one.exr").read_bytes() == whole == lr.write_file(channels, planes, "none")
    back = lr.read_file(whole)
    assert back["names"] == ["R", "steps"] and back["types"] == {"R": "half", "steps": "uint"}
    assert back["channels"]["R"].tolist() == [[1.5, 100.0]] and back["channels"]["steps"].tolist() == [[0, 3]]


# FLOAT and UINT channels of random bits: nothing deflate can shrink
NOISE = [("n.X", "float", "vel", 0), ("n.Y", "float", "vel", 1), ("n.Z", "float", "vel", 2), ("u", "uint", "steps", 0)]


@pytest.mark.parametrize("compression", lr.COMPRESSIONS)
@pytest.mark.parametrize("set_name", ("all_half", "mixed", "noise"))
def test_sink_files_with_layers_read_back_and_equal_the_restatements(set_name, compression, tmp_path):
    from relativisticraytracer_amd import sinks
    rrt, rng = _rrt(), np.random.default_rng(53)
    w, h = 19, 17                                         # with zip the last chunk is one row
    channels = NOISE if set_name == "noise" else lr.LAYER_SETS[set_name]
    if set_name == "noise":
        planes = {"vel": (rng.integers(0, 2 ** 32, (h, w, 3), dtype=np.uint64).astype(np.uint32).view(F), False),
                  "steps": (rng.integers(0, 2 ** 31, (h, w), dtype=np.int64).astype(np.int32), False)}
    else:       # a picture's values: few distinct ones, which deflate
        planes = {k: (np.floor(rng.uniform(0.0, 8.0, a.shape)).astype(a.dtype), up) for k, (a, up) in lr.random_planes(rng, w, h).items()}
    L = lr.api_layers(rrt, channels, planes, w, h, compression)
    files = {}
    for threads in (1, 3):
        pattern = str(tmp_path / f"t{threads}.%04d.exr")
        sink = sinks.EXRSink(pattern, w, h, 24, rrt.ExrFormat("half", compression), level=4, threads=threads, layers=L)
        assert sink.frame_bytes == rrt.exr_layers_frame_bytes(L)
        sink.write(rrt.exr_layers_host(L))
        with pytest.raises(ValueError):
            sink.write(np.zeros(sink.frame_bytes - 1, np.uint8))
        sink.close()
        files[threads] = open(pattern % 1, "rb").read()
    data = files[1]
    assert data == files[3] == lr.write_file(channels, planes, compression, 24, 4)
    back = lr.read_file(data)
    assert (back["width"], back["height"], back["compression"]) == (w, h, compression)
    assert back["names"] == [c[0] for c in lr.ordered(channels)]
    for name, type_, want in lr.samples(channels, planes):
        assert back["types"][name] == type_
        assert np.array_equal(back["channels"][name].view(want.dtype), want), name
    n_chunks = -(-h // xr.lines_per_chunk(compression))
    if compression != "none":       # incompressible chunks are stored raw, un-filtered; a reader sees size == n
        assert back["raw_chunks"] == sink.stored_raw == (n_chunks if set_name == "noise" else 0)
    with pytest.raises(ValueError):                # layers of another size
        sinks.EXRSink(str(tmp_path / "x.exr"), w + 1, h, 24, None, layers=L)


def _fake_layers(rrt, w, h, compression="zip"):
    """`all` with half beauty over made-up device planes 2^32 bytes apart"""
    shapes = {"hdr": (4, 0, True), "rad": (4, 0, False), "pos": (3, 0, False), "vel": (3, 0, False), "steps": (1, 1, False), "hit": (1, 1, False)}
    planes = {k: ((FAKE + ((i + 1) << 32), words, kind), up) for i, (k, (words, kind, up)) in enumerate(shapes.items())}
    return lr.api_layers(rrt, lr.LAYER_SETS["all_half"], planes, w, h, compression)


def test_refusals_without_a_device():
    """every refusal of the layers entry points, with made-up device addresses: a launch that passed the checks would fault on them"""
    from relativisticraytracer_amd import exr
    rrt, lib = _rrt(), exr.load()
    w, h = 64, 48
    out = FAKE
    launch = lib.rrt_launch_exr_layers
    n, k, y = C.c_size_t(0), C.c_int32(0), C.c_int32(0)
    g, head = (C.c_int32 * 8)(), (C.c_char * 2048)()

    def said():
        return lib.rrt_exr_last_error().decode()

    def every_function_refuses(L, part):
        assert launch(out, C.byref(L), w, h, None) == INVALID and part in said(), (part, said())
        assert lib.rrt_exr_layers_frame_bytes(C.byref(L), w, h, C.byref(n), C.byref(k)) == INVALID and part in said()
        assert lib.rrt_exr_layers_chunk(C.byref(L), w, h, 0, C.byref(y), C.byref(n), C.byref(n)) == INVALID and part in said()
        assert lib.rrt_exr_layers_launch_geometry(C.byref(L), w, h, 0, C.byref(g)) == INVALID and part in said()
        assert lib.rrt_exr_layers_header(C.byref(L), w, h, 24, 1, head, 2048, C.byref(n)) == INVALID and part in said()
        assert lib.rrt_exr_layers_host(out, C.byref(L), w, h) == INVALID and part in said()
    ok = _fake_layers(rrt, w, h)
    assert lib.rrt_exr_layers_frame_bytes(C.byref(ok), w, h, C.byref(n), C.byref(k)) == 0 and said() == "" and (n.value, k.value) == (w * h * 44, 3)
    for field, value, part in (("struct_size", 980, "struct_size"), ("compression", 1, "compression"), ("compression", 4, "compression"),
                               ("half_max", 0.0, "half_max"), ("half_max", 65520.0, "half_max"), ("half_max", float("nan"), "half_max"),
                               ("n_sources", 0, "n_sources"), ("n_sources", 9, "n_sources"), ("n_channels", 0, "n_channels"),
                               ("n_channels", 17, "n_channels")):
        L = _fake_layers(rrt, w, h)
        setattr(L, field, value)
        every_function_refuses(L, part)
    for words in (0, 2, 5, -1):
        L = _fake_layers(rrt, w, h)
        L.sources[0].words = words
        every_function_refuses(L, "words")
    for kind in (2, -1):
        L = _fake_layers(rrt, w, h)
        L.sources[1].kind = kind
        every_function_refuses(L, "kind")
    for name in (b"", b".B", b"B.", b"a b", b"a-b", b"caf\xc3\xa9", b"a,b"):
        L = _fake_layers(rrt, w, h)
        L.channels[0].name = name
        every_function_refuses(L, "name")
    L = _fake_layers(rrt, w, h)
    C.memset(C.addressof(L.channels[0]), ord("A"), 32)        # 32 bytes and no NUL
    every_function_refuses(L, "name")
    # unsorted and duplicate names: the offending pair, word for word
    L = _fake_layers(rrt, w, h)
    assert L.names[:4] == ["B", "G", "R", "direction.X"]
    L.channels[1].name = b"S"
    every_function_refuses(L, 'channel names must ascend strictly: "S" is followed by "R"')
    L.channels[1].name = b"R"
    every_function_refuses(L, 'channel names must ascend strictly: "R" is followed by "R"')
    L.channels[1].name = b"b"                                   # the order is the bytes': upper case first
    every_function_refuses(L, '"b" is followed by "R"')
    with pytest.raises(rrt.RRTError) as e:
        rrt.exr_layers_frame_bytes(rrt.ExrLayers(None, 2, 1, [("z", "uint", (FAKE, 1, 1), 0, False), ("a", "uint", (FAKE, 1, 1), 0, False)], sort=False))
    assert e.value.status == INVALID and '"z" is followed by "a"' in str(e.value)
    for field, value, part in (("type", 3, "type"), ("type", -1, "type"), ("source", 6, "source"), ("source", -1, "source"),
                               ("word", 4, "word"), ("word", -1, "word"), ("type", 0, "UINT")):      # B is a word of an F32 plane
        L = _fake_layers(rrt, w, h)
        setattr(L.channels[0], field, value)
        every_function_refuses(L, part)
    L = _fake_layers(rrt, w, h)
    steps = L.names.index("steps")
    L.channels[steps].word = 1                                  # a 1-word plane has word 0 only
    every_function_refuses(L, "word")
    # sizes
    for bw, bh in ((0, h), (w, 0), (-1, h)):
        assert launch(out, C.byref(ok), bw, bh, None) == INVALID and "width" in said()
        assert lib.rrt_exr_layers_frame_bytes(C.byref(ok), bw, bh, C.byref(n), None) == INVALID
    assert launch(out, C.byref(ok), 3050403, 16, None) == INVALID and "2^31" in said()            # 16 rows x 44 bytes x width >= 2^31
    assert lib.rrt_exr_layers_frame_bytes(C.byref(ok), 3050402, 16, C.byref(n), None) == 0
    # NULL and the buffers: before any device call
    assert launch(None, C.byref(ok), w, h, None) == INVALID and "NULL" in said()
    assert launch(out, None, w, h, None) == INVALID and "NULL" in said()
    L = _fake_layers(rrt, w, h)
    L.sources[2].d_data = None
    assert launch(out, C.byref(L), w, h, None) == INVALID and "NULL" in said()
    for off in (1, 2, 3):
        L = _fake_layers(rrt, w, h)
        L.sources[3].d_data += off
        assert launch(out, C.byref(L), w, h, None) == INVALID and "4-byte aligned" in said()
    total = rrt.exr_layers_frame_bytes(ok)
    for s in range(ok.n_sources):                               # the payload over any source: its first bytes, its last, the source inside it
        at, size = ok.sources[s].d_data, w * h * 4 * ok.sources[s].words
        for payload in (at, at + size - 1, at - total + 1):
            assert launch(payload, C.byref(ok), w, h, None) == INVALID and "overlaps" in said(), s
    assert lib.rrt_exr_layers_frame_bytes(C.byref(ok), w, h, None, None) == INVALID
    assert lib.rrt_exr_layers_chunk(C.byref(ok), w, h, 3, C.byref(y), C.byref(n), C.byref(n)) == INVALID
    assert lib.rrt_exr_layers_chunk(C.byref(ok), w, h, -1, C.byref(y), C.byref(n), C.byref(n)) == INVALID
    assert lib.rrt_exr_layers_chunk(C.byref(ok), w, h, 0, None, C.byref(n), C.byref(n)) == INVALID
    assert lib.rrt_exr_layers_launch_geometry(C.byref(ok), w, h, 0, None) == INVALID
    assert lib.rrt_exr_layers_header(C.byref(ok), w, h, 24, 1, None, 2048, C.byref(n)) == INVALID
    assert lib.rrt_exr_layers_header(C.byref(ok), w, h, 24, 1, head, 2048, None) == INVALID
    assert lib.rrt_exr_layers_header(C.byref(ok), w, h, 0, 1, head, 2048, C.byref(n)) == INVALID
    assert lib.rrt_exr_layers_default(None) == INVALID
    with pytest.raises(rrt.RRTError) as e:
        rrt.launch_exr_layers(ok.sources[0].d_data, ok)
    assert e.value.status == INVALID and "rrt_launch_exr_layers" in str(e.value) and "overlaps" in str(e.value)
    # the Python class's own
    with pytest.raises(ValueError):
        rrt.ExrLayers(None, 2, 2, [("a", "half", np.zeros(5, F), 0, False)])                  # not a multiple of 2 x 2
    with pytest.raises(ValueError):
        rrt.ExrLayers(None, 2, 2, [("a", "half", np.zeros(4, np.float64), 0, False)])
    with pytest.raises(ValueError):
        rrt.ExrLayers(None, 1, 1, [("c%02d" % i, "half", np.zeros(1, F), 0, False) for i in range(17)])


# ---- the shared source under the sanitizers

@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/exr/exr_layers_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("exr_layers")
    exe = str(d / "exr_layers_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "exr", "exr_layers_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case, text):
        path = d / (case + ".txt")
        path.write_text(text)
        r = subprocess.run([exe, case, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip().endswith(case + " ok"), (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.strip().splitlines()[:-1]
    return run


def test_shared_source_under_sanitizers_equals_the_restatement_and_the_library(exerciser):
    """odd sizes, planes and payload sized exactly, through the source the library's host entry points and kernels run: the digest
    (payload and header, in hexadecimal) equals the restatement's and the library's"""
    rrt, rng = _rrt(), np.random.default_rng(61)
    cases, text = [], []
    for set_name in SETS:
        channels = lr.ordered(lr.LAYER_SETS[set_name])
        keys = sorted({c[2] for c in channels})
        for compression in lr.COMPRESSIONS:
            for w, h, half_max in ((1, 1, 65504.0), (2, 1, 1024.0), (3, 17, 65504.0), (9, 33, 65504.0), (24, 16, 2.0)):
                planes = lr.random_planes(rng, w, h)
                L = lr.api_layers(rrt, channels, planes, w, h, compression, half_max)
                want = lr.payload(channels, planes, compression, half_max)
                assert np.array_equal(rrt.exr_layers_host(L), want)
                cases += [want.tobytes().hex(), lr.header(channels, w, h, compression).hex()]
                bits = int(np.array([half_max], F).view(np.uint32)[0])
                lines = [f"{xr.COMPRESSIONS[compression]} {bits:x} {w} {h} {len(keys)} {len(channels)}"]
                for key in keys:
                    a, up = planes[key]
                    a = np.ascontiguousarray(a)
                    lines.append(f"{a.size // (w * h)} {0 if a.dtype == np.float32 else 1} {int(up)}")
                    lines.append(" ".join(f"{v:x}" for v in a.ravel().view(np.uint32)))
                lines += [f"{n} {lr.TYPES[t]} {keys.index(k)} {word}" for n, t, k, word in channels]
                text.append("\n".join(lines) + "\n")
    assert exerciser("frames", "".join(text)) == cases


def test_shared_source_refusals_under_sanitizers(exerciser):
    assert exerciser("refusals", "") == []
