"""Device deflate without a GPU: librrt_deflate.so's host entry points against the Python restatement (tests/deflate_ref.py) byte for
byte and word for word; every stream through zlib's inflate; the sizes against zlib's own Z_RLE streams at the same cuts; the
fixtures' own properties on the restatement; the code-length builder on chosen counts; the refusals; PNGSink.write_streams' files
through the restatement's reader (and PIL where it exists); the exports; and the shared source under AddressSanitizer and
UndefinedBehaviorSanitizer (tests/deflate/deflate_exerciser.cpp, a program of its own)."""
import ctypes as C
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

import deflate_ref as dr
import png_ref as pr

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID = 1
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def fixtures(po):
    return dr.fixtures(po)


NAMES = sorted(dr.synthetic_fixtures()) + [f"png {w}x{h} depth {d} {f}" for w, h in ((67, 9), (131, 40)) for d in (8, 16) for f in pr.FILTERS]


def test_module_exports_and_the_other_libraries_are_untouched():
    from relativisticraytracer_amd import _lib, deflate, exr, png, yuv
    rrt = _rrt()
    for name in deflate.__all__:
        assert name in rrt.__all__ and getattr(rrt, name) is getattr(deflate, name), name
    others = _lib.SYMBOLS + _lib.TEST_SYMBOLS + yuv.YUV_SYMBOLS + exr.EXR_SYMBOLS + png.PNG_SYMBOLS
    assert not [n for n, _, _ in others if "deflate" in n]              # a library of its own
    assert rrt.abi_version() == 5


def test_library_exports_exactly_what_the_header_declares():
    from relativisticraytracer_amd import build, deflate, exr, png, yuv
    from test_capi import declared_functions
    build.build_lib()

    def exported(lib):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    declared = declared_functions("rrt_deflate.h")
    assert exported(build.DEFLATE_LIB) == declared
    assert declared == sorted(n for n, _, _ in deflate.DEFLATE_SYMBOLS)
    assert all(re.match(r"rrt_(deflate_|launch_deflate)", n) for n in declared), declared
    # the other four libraries are what their headers say, as before: no export moved
    assert exported(build.YUV_LIB) == declared_functions("rrt_yuv.h") == sorted(n for n, _, _ in yuv.YUV_SYMBOLS)
    assert exported(build.EXR_LIB) == declared_functions("rrt_exr.h") == sorted(n for n, _, _ in exr.EXR_SYMBOLS)
    assert exported(build.PNG_LIB) == declared_functions("rrt_png.h") == sorted(n for n, _, _ in png.PNG_SYMBOLS)
    assert not [n for n in exported(build.LIB) if "deflate" in n]
    needed = subprocess.run(["readelf", "-d", build.DEFLATE_LIB], capture_output=True, text=True, check=True).stdout
    assert "libz" not in needed                                # the library deflates by itself
    header = open(os.path.join(ROOT, "include", "rrt_deflate.h")).read()
    for name, value in (("RRT_DEFLATE_SEGMENT_BYTES", deflate.SEGMENT_BYTES), ("RRT_DEFLATE_THREADS", deflate.THREADS),
                        ("RRT_DEFLATE_CHUNK_BYTES", deflate.CHUNK_BYTES), ("RRT_DEFLATE_LL_SYMBOLS", deflate.LL_SYMBOLS),
                        ("RRT_DEFLATE_MAX_SYMBOLS", deflate.MAX_SYMBOLS)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    assert (deflate.SEGMENT_BYTES, deflate.CHUNK_BYTES) == (dr.SEGMENT, dr.CHUNK)


def test_the_fixtures_reach_the_branches_they_are_there_for(fixtures):
    """on the restatement alone: both sides of the stored decision, a literal tree deeper than 15, every remainder of the 258 cap, a
    run over the segment boundary -- so the equalities below are not vacuous"""
    assert sorted(fixtures) == sorted(NAMES)

    def notes(name, finish=1):
        info = []
        dr.deflate(fixtures[name][0].tobytes(), fixtures[name][1], finish, info)
        return info
    assert all(n["stored"] for n in notes("noise")) and not any(n["stored"] for n in notes("zeros"))
    dyn, sto = notes("decision: dynamic")[0], notes("decision: stored")[0]
    assert not dyn["stored"] and sto["stored"] and dyn["margin"] < 0 <= sto["margin"]
    assert sto["margin"] - dyn["margin"] <= 16, (dyn, sto)                  # a few bytes on either side
    assert notes("fibonacci")[0]["ll_halvings"] >= 1
    toks = dr.tokens(fixtures["runs behind another byte"][0].tobytes())
    matches = [t - 1000 for t in toks if t >= 1000]
    # R - 1 = 2 (literals), 3, 257, 258, 258 + 1 | 2 (literals), 258 + 3, 2 * 258, 2 * 258 + 3
    assert matches == [3, 257, 258, 258, 258, 258, 3, 258, 258, 258, 258, 3], matches
    data = fixtures["run across the segment boundary"][0].tobytes()
    second = dr.tokens(data[dr.SEGMENT:])
    assert data[dr.SEGMENT - 1] == data[dr.SEGMENT] and second[0] < 256 and second[1] == 1000 + 32900 - dr.SEGMENT - 1
    zeros = dr.tokens(bytes(dr.SEGMENT))
    assert set(zeros) == {0, 1258} and (dr.SEGMENT - 1) % 258 == 1       # two used symbols plus end-of-block: the remainder is a literal
    assert len(dr.cuts(300, 1)) == 300 and dr.cuts(1001, 500)[-1] == [(1000, 1001)]
    # the code-length code: a seeded search for a segment whose 19-symbol tree is deeper than 7.  The real payloads hold several.
    found = [name for name in NAMES if any(n["cl_halvings"] for n in notes(name))]
    assert found, "no fixture halves the code-length counts; rrt_deflate_code_lengths_host covers that branch below"


@pytest.mark.parametrize("finish", (1, 0))
@pytest.mark.parametrize("name", NAMES)
def test_host_streams_equal_the_restatement_and_inflate(name, finish, fixtures):
    rrt = _rrt()
    data, stream_bytes = fixtures[name]
    raw = data.tobytes()
    want = dr.deflate(raw, stream_bytes, finish)
    got = rrt.deflate_host(data, stream_bytes, finish)
    assert [len(s) for s in got] == [len(s) for s in want]
    assert got == want
    layout = dr.cuts(len(raw), stream_bytes)
    plan = rrt.deflate_plan(len(raw), stream_bytes)
    assert (plan["streams"], plan["segments"]) == (len(layout), sum(len(s) for s in layout))
    assert plan["out_bound"] == sum(b - a + 10 if b > a else 5 for segs in layout for a, b in segs) >= sum(len(s) for s in got)
    for j, (s, segs) in enumerate(zip(got, layout)):
        z = zlib.decompressobj(-15)
        assert z.decompress(s) == raw[segs[0][0]:segs[-1][1]], j
        assert z.eof == (bool(finish) and j == len(layout) - 1) and z.unused_data == b"" and z.unconsumed_tail == b""
    if finish:
        assert zlib.decompress(b"\x78\x01" + b"".join(got) + struct.pack(">I", zlib.adler32(raw))) == raw


@pytest.mark.parametrize("name", NAMES)
def test_streams_are_no_larger_than_zlibs_rle_streams_allow(name, fixtures):
    """len <= Z + Z / 100 + 8 * segments, Z zlib's size at level 4, Z_RLE, a full flush at the same cuts.

    zlib cuts a block of its own every 16 383 tokens; the definition has one block per segment.  On stationary input that is worth
    nothing (from 28 KB upward the ratio is 0.998 ... 1.000); tests/deflate_ref.py says what it is worth on one that is not."""
    rrt = _rrt()
    data, stream_bytes = fixtures[name]
    for finish in (1, 0):
        size = sum(len(s) for s in rrt.deflate_host(data, stream_bytes, finish))
        z = dr.zlib_rle_size(data.tobytes(), stream_bytes, finish)
        segments = rrt.deflate_plan(data.size, stream_bytes)["segments"]
        print(name, finish, size, z, z + z // 100 + 8 * segments)
        assert size <= z + z // 100 + 8 * segments, (size, z, segments)


# ---- the large fixtures (tests/deflate_ref.py: large_fixtures): full-size segments by the hundred, at a frame's cut

def test_the_pool_blocks_stay_in_their_classes():
    """on the restatement alone: the stored block, the dynamic block a few dozen bytes short of it, the block of every symbol"""
    pool = dr.pool()
    assert tuple(pool) == dr.POOL and len(pool) == 8

    def note(name):
        info = []
        out = dr.fragment(pool[name].tobytes(), False, info)
        return len(out), info[0]
    size, n = note("noise")
    assert n["stored"] and n["margin"] >= 0 and size == dr.SEGMENT + 10
    size, n = note("250 values")
    assert not n["stored"] and -200 <= n["margin"] <= -1 and size == dr.SEGMENT + 10 + n["margin"], n
    size, n = note("zeros")
    assert not n["stored"] and size == 50
    for name in ("laplace 3", "laplace 1.5", "random runs", "two values", "every symbol"):
        size, n = note(name)
        assert not n["stored"] and size < dr.SEGMENT, name
    assert note("laplace 1.5")[0] < note("laplace 3")[0]
    assert set(pool["two values"].tolist()) == {3, 200} and all(t < 256 for t in dr.tokens(pool["two values"].tobytes()))
    assert any(t >= 1000 for t in dr.tokens(pool["random runs"].tobytes()))
    toks = dr.tokens(pool["every symbol"].tobytes())
    assert {t for t in toks if t < 256} == set(range(256))
    matches = sorted(dr.length_symbol(t - 1000)[0] for t in toks if t >= 1000)
    assert matches == list(range(257, 286))                          # one match per length symbol: nll = 286
    counts = [0] * dr.LL_SYMBOLS
    for t in toks:
        counts[t if t < 256 else dr.length_symbol(t - 1000)[0]] += 1
    counts[dr.EOB] = 1
    assert all(dr.lengths(counts, 15)[0])


def test_the_large_fixtures_have_the_cuts_they_are_there_for():
    large = dr.large_fixtures()
    assert tuple(large) == dr.LARGE_NAMES
    want = {"three per stream": (11803780, 181, 541), "two per stream": (9830699, 300, 599), "frame cut": (17828971, 17, 560)}
    pool = [b.tobytes() for b in dr.pool().values()]
    for name, (n, streams, segments) in want.items():
        data, stream_bytes = large[name]
        layout = dr.cuts(data.size, stream_bytes)
        assert (data.size, len(layout), sum(len(s) for s in layout)) == (n, streams, segments), name
        assert len(layout[-1]) < len(layout[0])                      # a last stream shorter than the rest
        raw = data.tobytes()
        full = [raw[a:b] for segs in layout for a, b in segs if b - a == dr.SEGMENT]
        assert set(full) == set(pool), name                          # every block of the pool is drawn
        info = []
        dr.deflate(raw, stream_bytes, 1, info)
        assert any(i["stored"] and i["m"] == dr.SEGMENT for i in info) and any(-200 <= i["margin"] <= -1 for i in info if i["m"] == dr.SEGMENT)
    assert sum(b - a == dr.SEGMENT for segs in dr.cuts(17828971, large["frame cut"][1]) for a, b in segs) == 543
    two = dr.fragments(large["two per stream"][0].tobytes(), large["two per stream"][1], 0)
    assert all(len(parts) == 2 and len(parts[1]) == 11 for parts in two[:-1]) and len(two[-1]) == 1      # a stored fragment of one byte
    for name, block in dr.LARGE_SINGLE.items():
        assert large[name][0] is dr.pool()[block] and dr.cuts(dr.SEGMENT, large[name][1]) == [[(0, dr.SEGMENT)]]


@pytest.mark.parametrize("name", dr.LARGE_NAMES)
def test_host_streams_of_the_large_fixtures_equal_the_restatement_and_inflate(name):
    rrt = _rrt()
    data, stream_bytes = dr.large_fixtures()[name]
    raw = data.tobytes()
    layout = dr.cuts(len(raw), stream_bytes)
    segments = sum(len(s) for s in layout)
    plan = rrt.deflate_plan(len(raw), stream_bytes)
    assert (plan["streams"], plan["segments"]) == (len(layout), segments)
    assert plan["out_bound"] == sum(b - a + 10 for segs in layout for a, b in segs)
    for finish in (1, 0):
        want = dr.deflate(raw, stream_bytes, finish)
        got = rrt.deflate_host(data, stream_bytes, finish)
        assert [len(s) for s in got] == [len(s) for s in want]
        assert got == want, dr.first_difference(got, raw, stream_bytes, finish)
        assert plan["out_bound"] >= sum(len(s) for s in got)
        for j, (s, segs) in enumerate(zip(got, layout)):
            z = zlib.decompressobj(-15)
            assert z.decompress(s) == raw[segs[0][0]:segs[-1][1]], j
            assert z.eof == (bool(finish) and j == len(layout) - 1) and z.unused_data == b"" and z.unconsumed_tail == b""
        # the size condition of test_streams_are_no_larger_than_zlibs_rle_streams_allow: zlib is the yardstick
        size, z = sum(len(s) for s in got), dr.zlib_rle_size(raw, stream_bytes, finish)
        print(name, finish, size, z, z + z // 100 + 8 * segments)
        assert size <= z + z // 100 + 8 * segments, (size, z, segments)


def test_host_streams_do_not_depend_on_where_the_input_lies(fixtures):
    rrt = _rrt()
    for name in ("runs across chunk boundaries", "n=32769", "stride 403"):
        data, stream_bytes = fixtures[name]
        want = dr.deflate(data.tobytes(), stream_bytes, 1)
        holder = np.zeros(data.size + 32, np.uint8)
        for shift in range(16):
            at = (-holder.ctypes.data) % 16 + shift
            holder[at:at + data.size] = data
            assert rrt.deflate_host(holder[at:at + data.size], stream_bytes, 1) == want, (name, shift)


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def test_code_lengths_on_chosen_counts():
    """step 4 alone: Fibonacci counts make the deepest trees, so both limits are exceeded and the counts halved, more than once"""
    rrt = _rrt()
    rng = np.random.default_rng(4)
    cases = [(_fib(n), 7) for n in (9, 10, 12, 19)] + [(_fib(n), 15) for n in (17, 18, 20, 30, 40)]
    cases += [([0, 0, 5, 0], 7), ([7, 0, 0, 0], 7), ([0] * 19, 7), ([3, 3], 1), ([1] * 286, 15), ([1] * 128, 7)]
    cases += [(rng.integers(0, 50, 286).tolist(), 15) for _ in range(4)] + [(rng.integers(0, 9, 19).tolist(), 7) for _ in range(8)]
    cases += [((rng.integers(0, 3, 286) * rng.integers(1, 30000, 286)).tolist(), 15) for _ in range(4)]
    halved = {1: 0, 7: 0, 15: 0}
    for counts, limit in cases:
        want, halvings = dr.lengths(counts, limit)
        got, got_halvings = rrt.deflate_code_lengths(counts, limit)
        assert got.tolist() == want and got_halvings == halvings, (counts, limit)
        halved[limit] = max(halved[limit], halvings)
        used = [l for l in want if l]
        assert max(want) <= limit and (not used or sum(2.0 ** -l for l in used) == 1.0)        # a complete prefix code
    assert halved[7] >= 2 and halved[15] >= 2, halved
    assert rrt.deflate_code_lengths([0, 0, 5, 0], 7)[0].tolist() == [1, 0, 1, 0]                # the lowest unused symbol joins a lone one
    assert rrt.deflate_code_lengths([7, 0, 0, 0], 7)[0].tolist() == [1, 1, 0, 0]


def test_library_refusals_come_before_any_device_call():
    from relativisticraytracer_amd import deflate
    rrt = _rrt()

    def refused(fn, *args, match):
        with pytest.raises(rrt.RRTError, match=match) as e:
            fn(*args)
        assert e.value.status == INVALID

    out, tab, scr, src = FAKE, FAKE + (1 << 30), FAKE + (2 << 30), FAKE + (3 << 30)
    for k in range(4):
        args = [out, tab, scr, src]
        args[k] = 0
        refused(rrt.launch_deflate, *args, 64, 64, 1, 0, match="NULL")
    refused(rrt.launch_deflate, out, tab, scr, src, 1 << 32, 64, 1, 0, match="2\\^32")
    refused(rrt.launch_deflate, out, tab, scr, src, 400000000, 1, 1, 0, match="out_bound")
    refused(rrt.launch_deflate, out, tab, scr, src, 64, 0, 1, 0, match="stream_bytes")
    refused(rrt.launch_deflate, out, tab + 2, scr, src, 64, 64, 1, 0, match="4-byte aligned")
    refused(rrt.launch_deflate, out, tab, scr + 8, src, 64, 64, 1, 0, match="16-byte aligned")
    refused(rrt.launch_deflate, src + 32, tab, scr, src, 64, 64, 1, 0, match="overlaps the input")
    refused(rrt.launch_deflate, out, src + 60, scr, src, 64, 64, 1, 0, match="overlaps the input")
    refused(rrt.launch_deflate, out, tab, src - 16, src, 64, 64, 1, 0, match="overlaps the input")
    refused(rrt.launch_deflate, out, out + 72, scr, src, 64, 64, 1, 0, match="overlap each other")
    refused(rrt.launch_deflate, out, tab, out + 64, src, 64, 64, 1, 0, match="overlap each other")
    refused(rrt.launch_deflate, out, scr + 16, scr, src, 64, 64, 1, 0, match="overlap each other")
    refused(rrt.deflate_plan, 1 << 32, 64, match="2\\^32")
    refused(rrt.deflate_plan, 64, 0, match="stream_bytes")
    refused(rrt.deflate_code_lengths, [1, 2, 3], 1, match="limit")
    refused(rrt.deflate_code_lengths, [1], 7, match="n_symbols")
    refused(rrt.deflate_code_lengths, [1 << 31, 1 << 31], 7, match="sum")
    big = (1 << 32) - 1 - 10 * 131072
    assert rrt.deflate_plan(big, 1 << 40)["segments"] == -(-big // 32768) and rrt.deflate_plan(big, 1 << 40)["out_bound"] < 1 << 32
    assert deflate.load().rrt_deflate_launch_geometry(64, 64, 0, None) == INVALID
    assert rrt.deflate_plan(0, 5) == {"streams": 1, "segments": 1, "out_bound": 5, "scratch_bytes": 16 + 48 + 64}


# ---- the sink's files

@pytest.mark.parametrize("depth", (8, 16))
def test_write_streams_files_decode_to_the_raw_samples(depth, po, tmp_path):
    """one slice and several, through PNGSink.write_streams and back through the reader written from the specification; and PIL"""
    from relativisticraytracer_amd import sinks
    rrt, rng = _rrt(), np.random.default_rng(6)
    small = pr.rgba8_frame(rng, 65, 17) if depth == 8 else pr.hdr_frame(rng, 65, 17)
    big = pr.rgba8_frame(rng, 16384, 40) if depth == 8 else pr.hdr_frame(rng, 16384, 24)
    for frame, filter_name in ((small, "adaptive"), (big, "up")):
        h, w = frame.shape[:2]
        f = rrt.PngFormat(depth, filter_name)
        pay, sums = (rrt.png_from_rgba8_host if depth == 8 else rrt.png_from_hdr_host)(frame, f)
        rows, n = rrt.png_slices(f, w, h)
        assert (n == 1) == (w == 65)
        sink = sinks.PNGSink(str(tmp_path / f"s{w}.png"), w, h, f)
        streams = rrt.deflate_host(pay, rows * sink.stride, True)
        assert len(streams) == n
        name = sink.write_streams(streams, sums)
        sink.close()
        data = open(name, "rb").read()
        back = pr.read_file(data)
        assert (back["width"], back["height"], back["depth"]) == (w, h, depth)
        assert back["chunks"] == ["IHDR", "sRGB", "tEXt"] + ["IDAT"] * n + ["IEND"]
        raw = pr.raw_from_rgba8(frame) if depth == 8 else pr.raw_from_hdr(po, frame)
        samples = raw.reshape(h, w, 3) if depth == 8 else pr.q_from_hdr(po, frame)
        assert np.array_equal(back["samples"], samples), (w, h)
        host = sinks.PNGSink(str(tmp_path / f"h{w}.png"), w, h, f)
        assert np.array_equal(pr.read_file(open(host.write(pay, sums), "rb").read())["samples"], samples)      # `write` as before
        host.close()
        if w == 65:
            Image = pytest.importorskip("PIL.Image")
            with Image.open(name) as im:
                got = np.asarray(im.convert("RGB") if depth == 16 else im)
            assert np.array_equal(got, frame[::-1, :, :3] if depth == 8 else (samples >> 8).astype(np.uint8))
    with pytest.raises(ValueError, match="streams"):
        sinks.PNGSink(str(tmp_path / "x.png"), 65, 17).write_streams([b"", b""], np.zeros(34, np.uint32))


# ---- the shared source under the sanitizers

@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/deflate/deflate_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("deflate")
    exe = str(d / "deflate_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "deflate", "deflate_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case, text):
        path = d / (case + ".txt")
        path.write_text(text)
        r = subprocess.run([exe, case, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip().endswith(case + " ok"), (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.rstrip("\n").split("\n")[:-1]
    return run


def test_shared_source_under_sanitizers_equals_the_restatement(exerciser, fixtures):
    """every fixture, every buffer sized exactly, the input at shifting alignments, through the source the library's host entry
    points and the kernel run"""
    text, want = [], []
    for k, name in enumerate(NAMES):
        data, stream_bytes = fixtures[name]
        for finish in (1, 0):
            shift = (3 * k + finish) % 16
            text.append(f"{finish} {stream_bytes} {shift} {data.size}\n{data.tobytes().hex() or '-'}\n")
            streams = dr.deflate(data.tobytes(), stream_bytes, finish)
            want += [" ".join(str(len(s)) for s in streams), b"".join(streams).hex()]
    assert exerciser("streams", "".join(text)) == want


def test_shared_source_under_sanitizers_on_full_size_segments(exerciser):
    """the eight blocks of the pool, each a full segment, and one stream of `two per stream`: a full block and one byte.  (The three
    large inputs stay out: their text would be tens of megabytes.)"""
    pool = dr.pool()
    cases = [(block, 1 << 20) for block in pool.values()]
    cases.append((np.concatenate([pool["noise"], dr.ramp(1), pool["250 values"], dr.ramp(1)]), dr.SEGMENT + 1))
    text, want = [], []
    for k, (data, stream_bytes) in enumerate(cases):
        for finish in (1, 0):
            shift = (5 * k + finish) % 16
            text.append(f"{finish} {stream_bytes} {shift} {data.size}\n{data.tobytes().hex()}\n")
            streams = dr.deflate(data.tobytes(), stream_bytes, finish)
            want += [" ".join(str(len(s)) for s in streams), b"".join(streams).hex()]
    assert exerciser("streams", "".join(text)) == want


def test_shared_source_code_lengths_and_refusals_under_sanitizers(exerciser):
    cases = [(_fib(n), 7) for n in (9, 19)] + [(_fib(n), 15) for n in (17, 40)] + [([1] * 286, 15), ([0, 0, 5, 0], 7), ([0] * 19, 7)]
    text = "".join(f"{limit} {len(c)} " + " ".join(map(str, c)) + "\n" for c, limit in cases)
    want = []
    for c, limit in cases:
        lens, halvings = dr.lengths(c, limit)
        want.append(" ".join(map(str, [halvings] + lens)))
    assert exerciser("lengths", text) == want
    assert exerciser("refusals", "") == []
