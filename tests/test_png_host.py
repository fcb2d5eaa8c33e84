"""PNG output without a GPU: librrt_png.so's host entry points against the numpy restatement (tests/png_ref.py) byte for byte and
word for word, the fixtures' own properties, the Adler fold, the header, the inverse, the refusals, the sink's files through the
restatement's reader (and PIL where it exists), the exports, and the shared source under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/png/png_exerciser.cpp, a program of its own)."""
import ctypes as C
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import png_ref as pr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID = 1
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it
DEPTHS = (8, 16)


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def frames(po):
    """one frame per depth and size, shared and left unchanged: {(depth, w, h): (frame, raw scanlines)}"""
    rng = np.random.default_rng(77)
    out = {}
    for w in pr.HOST_WIDTHS:
        for h in pr.HOST_HEIGHTS:
            f8, f16 = pr.rgba8_frame(rng, w, h), pr.hdr_frame(rng, w, h)
            out[(8, w, h)] = (f8, pr.raw_from_rgba8(f8))
            out[(16, w, h)] = (f16, pr.raw_from_hdr(po, f16))
    return out


def _host(rrt, depth, frame, filter_name):
    f = rrt.PngFormat(depth, filter_name)
    return (rrt.png_from_rgba8_host if depth == 8 else rrt.png_from_hdr_host)(frame, f)


def test_module_exports_and_the_other_libraries_are_untouched():
    from relativisticraytracer_amd import _lib, exr, png, yuv
    rrt = _rrt()
    for name in png.__all__:
        assert name in rrt.__all__ and getattr(rrt, name) is getattr(png, name), name
    others = _lib.SYMBOLS + _lib.TEST_SYMBOLS + yuv.YUV_SYMBOLS + exr.EXR_SYMBOLS
    assert not [n for n, _, _ in others if "png" in n]                  # a library of its own
    assert C.sizeof(png.rrt_png_format) == 12
    f = rrt.PngFormat()
    assert (f.struct_size, f.depth, f.filter) == (12, 8, 5)
    assert [png.FILTERS[n] for n in pr.FILTERS] == [0, 1, 2, 3, 4, 5]    # the file format's own type numbers, then the choice


def test_library_exports_exactly_what_the_header_declares():
    from relativisticraytracer_amd import build, exr, png, yuv
    from test_capi import declared_functions
    build.build_lib()

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    declared = declared_functions("rrt_png.h")
    assert exported(build.PNG_LIB) == declared
    assert declared == sorted(n for n, _, _ in png.PNG_SYMBOLS)
    assert all(re.match(r"rrt_(png|launch_png)_", n) for n in declared), declared
    # the other three libraries are what their headers say, as before: no export moved
    assert exported(build.YUV_LIB) == declared_functions("rrt_yuv.h") == sorted(n for n, _, _ in yuv.YUV_SYMBOLS)
    assert exported(build.EXR_LIB) == declared_functions("rrt_exr.h") == sorted(n for n, _, _ in exr.EXR_SYMBOLS)
    assert not [n for n in exported(build.LIB) if "png" in n]
    needed = subprocess.run(["readelf", "-d", build.PNG_LIB], capture_output=True, text=True, check=True).stdout
    assert "libz" not in needed                                # the library does not deflate: its CRCs are its own
    header = open(os.path.join(ROOT, "include", "rrt_png.h")).read()
    for name, value in (("RRT_PNG_SLICE_BYTES", png.SLICE_BYTES), ("RRT_PNG_BAND_ROWS", png.BAND_ROWS), ("RRT_PNG_SEGMENT_CHUNKS", png.SEGMENT_CHUNKS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value


def test_the_fixtures_reach_every_type_and_a_tie(frames):
    """on the restatement alone: adaptive picks each of the five types on some row of ONE frame per depth, and some row has two
    candidates with exactly the smallest score -- so the equality below is not vacuous"""
    for depth in DEPTHS:
        _, raw = frames[(depth, 64, 17)]
        cand = pr.candidates(raw, 3 * depth // 8)
        assert set(pr.choice(cand, "adaptive").tolist()) == {0, 1, 2, 3, 4}, depth
        best_two = np.sort(pr.scores(cand), axis=1)[:, :2]
        assert (best_two[:, 0] == best_two[:, 1]).any(), depth
        five_way = (pr.scores(cand) == 0).all(axis=1)                    # an all-zero row under an all-zero row
        assert five_way.any() and (pr.choice(cand, "adaptive")[five_way] == 0).all()
    lin = frames[(16, 64, 17)][0]
    assert np.isnan(lin).any() and np.isposinf(lin).any() and np.isneginf(lin).any() and (lin < 0).any() and (lin == 0).any()


@pytest.mark.parametrize("filter_name", pr.FILTERS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_host_payload_and_row_sums_equal_the_restatement(depth, filter_name, frames):
    rrt = _rrt()
    f = rrt.PngFormat(depth, filter_name)
    for w in pr.HOST_WIDTHS:
        for h in pr.HOST_HEIGHTS:
            frame, raw = frames[(depth, w, h)]
            want, types, sums = pr.payload(raw, f.bpp, filter_name)
            n, stride, table = rrt.png_frame_bytes(f, w, h, layout=True)
            assert (n, stride, table) == (want.size, want.shape[1], 8 * h) and stride == 1 + w * f.bpp
            got, got_sums = _host(rrt, depth, frame, filter_name)
            bad = np.flatnonzero(got != want.ravel())
            assert bad.size == 0, (w, h, bad[:8].tolist(), types.tolist())
            assert np.array_equal(got_sums.reshape(h, 2), sums), (w, h)
            assert rrt.png_adler32(got_sums, f, w, h) == zlib.adler32(want.tobytes()) == pr.adler32(sums, stride), (w, h)
            assert np.array_equal(rrt.png_unfilter_host(got, f, w, h), raw), (w, h)
            assert np.array_equal(pr.unfilter(want, f.bpp), raw), (w, h)         # the reader's inverse is one, too


def test_header_bytes_and_crcs():
    rrt = _rrt()
    for depth in DEPTHS:
        for w, h in ((1, 1), (640, 480), (3840, 2160), (70000, 3)):
            data = rrt.png_header(rrt.PngFormat(depth), w, h)
            assert data == pr.header(w, h, depth)                             # zlib.crc32 made those
    assert rrt.png_header(rrt.PngFormat(8, "up"), 5, 4) == rrt.png_header(rrt.PngFormat(8, "paeth"), 5, 4)     # the filter is the rows' business
    with pytest.raises(rrt.RRTError, match="cap is smaller"):
        rrt.png_header(None, 5, 4, cap=40)


def test_slices_depend_on_the_frame_alone():
    rrt = _rrt()
    for depth in DEPTHS:
        f = rrt.PngFormat(depth)
        for w, h in ((1, 1), (64, 48), (1920, 1080), (3840, 2160), (16384, 12), (400000, 2)):
            stride = 1 + w * f.bpp
            assert rrt.png_slices(f, w, h) == pr.slices(stride, h), (w, h)
    assert rrt.png_slices(rrt.PngFormat(8), 3840, 2160) == (92, 24)


def test_library_refusals_come_before_any_device_call():
    from relativisticraytracer_amd import png
    rrt = _rrt()

    def refused(fn, *args, match):
        with pytest.raises(rrt.RRTError, match=match) as e:
            fn(*args)
        assert e.value.status == INVALID

    ok8, ok16 = rrt.PngFormat(8), rrt.PngFormat(16)
    for bad, match in ((rrt.PngFormat(12), "depth"), (rrt.PngFormat(8, 6), "filter"), (rrt.PngFormat(8, -1), "filter")):
        refused(rrt.png_frame_bytes, bad, 4, 4, match=match)
        refused(rrt.launch_png_from_rgba8, FAKE, FAKE + (1 << 30), FAKE + (2 << 30), 4, 4, bad, 0, match=match)
    short = rrt.PngFormat()
    short.struct_size = 8
    refused(rrt.png_frame_bytes, short, 4, 4, match="struct_size")
    for w, h in ((0, 4), (4, 0), (-1, 4)):
        refused(rrt.png_frame_bytes, ok8, w, h, match="width and height")
    refused(rrt.png_frame_bytes, ok8, 1 << 16, 1 << 15, match="2\\^31")
    refused(rrt.png_frame_bytes, ok8, 37838, 37838, match="2\\^32")
    refused(rrt.png_frame_bytes, ok16, 26755, 26755, match="2\\^32")
    assert rrt.png_frame_bytes(ok8, 37837, 37837) == 4294953544
    # launches: NULL, the other entry point's depth, misaligned tables, overlaps -- all before a device is touched (the addresses are made up)
    a, b, c = FAKE, FAKE + (1 << 30), FAKE + (2 << 30)
    refused(rrt.launch_png_from_rgba8, 0, b, c, 4, 4, ok8, 0, match="NULL")
    refused(rrt.launch_png_from_rgba8, a, 0, c, 4, 4, ok8, 0, match="NULL")
    refused(rrt.launch_png_from_hdr, a, b, 0, 4, 4, ok16, 0, match="NULL")
    refused(rrt.launch_png_from_rgba8, a, b, c, 4, 4, ok16, 0, match="depth")
    refused(rrt.launch_png_from_hdr, a, b, c, 4, 4, ok8, 0, match="depth")
    refused(rrt.launch_png_from_rgba8, a, b + 2, c, 4, 4, ok8, 0, match="4-byte aligned")
    refused(rrt.launch_png_from_hdr, a, b, c + 2, 4, 4, ok16, 0, match="4-byte aligned")
    refused(rrt.launch_png_from_rgba8, a, b, a + 8, 4, 4, ok8, 0, match="overlaps")
    refused(rrt.launch_png_from_hdr, a + 64, b, a, 4, 4, ok16, 0, match="overlaps")
    refused(rrt.launch_png_from_rgba8, a, a + 4, c, 4, 4, ok8, 0, match="overlaps")
    refused(rrt.launch_png_from_rgba8, a, c + 4, c, 4, 4, ok8, 0, match="overlaps")
    frame = np.zeros((4, 4, 4), np.uint8)
    refused(rrt.png_from_rgba8_host, frame, ok16, match="depth")
    refused(rrt.png_unfilter_host, np.full(52, 9, np.uint8), ok8, 4, 4, match="filter type")
    assert png.load().rrt_png_frame_bytes(None, 4, 4, None, None, None) == INVALID


def test_geometry_query_follows_the_addresses():
    rrt = _rrt()
    g = rrt.png_launch_geometry(rrt.PngFormat(8), 3840, 2160)
    assert g == {"threads": 256, "rows": 4, "grid": 540, "chunks": (11521 + 30) // 16, "segments": 1, "lds_bytes": 2 * (16 * 721 + 160),
                 "wide": True, "segment_chunks": 721}
    for bits in range(1, 16):
        n = rrt.png_launch_geometry(rrt.PngFormat(8), 3840, 2160, bits)
        assert not n["wide"] and (n["threads"], n["rows"], n["grid"], n["lds_bytes"]) == (64, 64, 34, 0)
    assert rrt.png_launch_geometry(rrt.PngFormat(16), 3840, 2160, 0x7f0000000010)["wide"]


# ---- the sink's files

def _write(tmp_path, name, pay, sums, w, h, f, threads):
    from relativisticraytracer_amd import sinks
    sink = sinks.PNGSink(str(tmp_path / name), w, h, f, threads=threads)
    out = sink.write(pay, sums)
    sink.close()
    assert out == str(tmp_path / name) and not os.path.exists(out + ".tmp")
    return open(out, "rb").read(), sink


@pytest.mark.parametrize("depth", DEPTHS)
def test_sink_files_decode_to_the_raw_samples(depth, frames, po, tmp_path):
    """a frame of exactly one slice, adaptive, and a frame of several (height > R), through PNGSink and back through the reader
    written from the specification; the bytes are the restatement's, and the same with 1 and 4 threads"""
    rrt, rng = _rrt(), np.random.default_rng(5)
    one = (64, 17, "adaptive", frames[(depth, 64, 17)][0])
    wide_w = 16384
    big = pr.rgba8_frame(rng, wide_w, 40) if depth == 8 else pr.hdr_frame(rng, wide_w, 24)
    cases = [one, (wide_w, big.shape[0], "up", big)]
    for w, h, filter_name, frame in cases:
        f = rrt.PngFormat(depth, filter_name)
        raw = pr.raw_from_rgba8(frame) if depth == 8 else pr.raw_from_hdr(po, frame)
        pay, sums = _host(rrt, depth, frame, filter_name)
        rows, n = rrt.png_slices(f, w, h)
        assert (n == 1) == (w == 64) and (w == 64 or (h > rows and h % rows != 0))         # one slice | several, the last one short
        data, sink = _write(tmp_path, f"a{w}.png", pay, sums, w, h, f, 4)
        assert (sink.n_slices, sink.rows_per_slice) == (n, rows)
        assert data == _write(tmp_path, f"b{w}.png", pay, sums, w, h, f, 1)[0]
        want, _, want_sums = pr.payload(raw, f.bpp, filter_name)
        assert data == pr.write_file(want, want_sums, w, h, depth)
        back = pr.read_file(data)
        assert (back["width"], back["height"], back["depth"], back["intent"]) == (w, h, depth, 0)
        assert back["chunks"] == ["IHDR", "sRGB", "tEXt"] + ["IDAT"] * n + ["IEND"] and back["text"] == (b"Software", pr.SOFTWARE)
        samples = raw.reshape(h, w, 3) if depth == 8 else pr.q_from_hdr(po, frame)
        assert np.array_equal(back["samples"], samples), (w, h)
        if filter_name == "adaptive":
            assert len(set(back["types"].tolist())) == 5


@pytest.mark.parametrize("depth", DEPTHS)
def test_pil_reads_the_files(depth, frames, po, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rrt = _rrt()
    w, h = 65, 17
    frame = frames[(depth, w, h)][0]
    f = rrt.PngFormat(depth)
    pay, sums = _host(rrt, depth, frame, "adaptive")
    _write(tmp_path, "p.png", pay, sums, w, h, f, 1)
    with Image.open(str(tmp_path / "p.png")) as im:
        assert im.size == (w, h)
        got = np.asarray(im.convert("RGB") if depth == 16 else im)
    if depth == 8:
        assert np.array_equal(got, frame[::-1, :, :3])
    else:
        assert np.array_equal(got, (pr.q_from_hdr(po, frame) >> 8).astype(np.uint8))


def test_sink_refuses_what_the_exr_sink_refuses(tmp_path):
    from relativisticraytracer_amd import sinks
    with pytest.raises(ValueError, match="one frame field"):
        sinks.PNGSink(str(tmp_path / "f.%d.%d.png"), 4, 4)
    with pytest.raises(ValueError, match="level"):
        sinks.PNGSink(str(tmp_path / "f.%d.png"), 4, 4, level=0)
    rrt = _rrt()
    pay, sums = rrt.png_from_rgba8_host(np.zeros((4, 4, 4), np.uint8))
    sink = sinks.PNGSink(str(tmp_path / "f.png"), 4, 4)
    with pytest.raises(ValueError, match="bytes"):
        sink.write(pay[:-1], sums)
    sink.write(pay, sums)
    with pytest.raises(ValueError, match="no frame field"):
        sink.write(pay, sums)
    sink.close()
    seq = sinks.PNGSink(str(tmp_path / "g.%03d.png"), 4, 4, level=9)
    assert [os.path.basename(seq.write(pay, sums)) for _ in range(2)] == ["g.001.png", "g.002.png"]
    seq.close()


# ---- the shared source under the sanitizers

@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/png/png_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("png")
    exe = str(d / "png_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "png", "png_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case, text):
        path = d / (case + ".txt")
        path.write_text(text)
        r = subprocess.run([exe, case, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip().endswith(case + " ok"), (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.strip().splitlines()[:-1]
    return run


def test_shared_source_under_sanitizers_equals_the_restatement(exerciser, frames):
    """odd sizes, every buffer sized exactly, through the source the library's host entry points and kernels run"""
    cases, text = [], []
    for depth in DEPTHS:
        for k, filter_name in enumerate(pr.FILTERS):
            for w, h in ((1, 1), (2, 1), (1, 2), (5, 17), (9, 2), (65, 17)):
                frame, raw = frames[(depth, w, h)]
                want, _, sums = pr.payload(raw, 3 * depth // 8, filter_name)
                cases += [want.tobytes().hex(), " ".join(f"{v:x}" for v in sums.ravel()), f"{pr.adler32(sums, want.shape[1]):08x}",
                          pr.header(w, h, depth).hex()]
                words = frame.view(np.uint32).ravel()
                text.append(f"{depth} {k} {w} {h}\n" + " ".join(f"{v:x}" for v in words) + "\n")
    lines = [ln.strip() for ln in exerciser("frames", "".join(text))]
    assert lines == cases


def test_shared_source_refusals_under_sanitizers(exerciser):
    assert exerciser("refusals", "") == []
