"""Y4M output without a GPU: librrt_yuv.so's host entry points (include/rrt_yuv.h) against the definition -- the coefficients against
exact rational rounding, the anchor colours, the codes' meaning against the real-valued BT.709 formula, the host conversions against
the numpy restatement (tests/yuv_ref.py) byte for byte -- the refusals, the Y4M sink, both drivers' new refusals, the exports, and
the shared source under AddressSanitizer and UndefinedBehaviorSanitizer (tests/yuv/yuv_exerciser.cpp, a program of its own)."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import exposure_ref as er
import yuv_ref as yr
from test_driver_refusals import CPP, PY, TWO_RANKS, ArgparseSays, refused  # noqa: F401

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, ABI_MISMATCH = 1, 6
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it
F = np.float32
IDS = dict(ids=lambda f: f"{f[0]}-{'full' if f[1] else 'limited'}-{f[2]}" if isinstance(f, tuple) and len(f) == 3 else None)


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


def _fmt(fmt):
    return _rrt().YuvFormat(fmt[0], "full" if fmt[1] else "limited", fmt[2])


def _samples(data, fmt):
    """a frame's bytes as integer samples"""
    return np.asarray(data, np.uint8).view(np.uint8 if fmt[2] == 8 else np.dtype("<u2")).astype(np.int64)


@pytest.fixture(scope="module")
def geometry():
    return _rrt().yuv_launch_geometry(None, 64, 48)


def test_module_exports_and_the_c_abi_is_untouched():
    from relativisticraytracer_amd import _lib, yuv
    rrt = _rrt()
    names = ["YuvFormat", "yuv_coefficients", "yuv_frame_bytes", "y4m_header", "launch_yuv_from_rgba8", "launch_yuv_from_hdr",
             "yuv_from_rgba8_host", "yuv_from_hdr_host", "yuv_launch_geometry"]
    for name in names:
        assert name in rrt.__all__ and getattr(rrt, name) is getattr(yuv, name), name
    assert not [n for n, _, _ in _lib.SYMBOLS + _lib.TEST_SYMBOLS if "yuv" in n or "y4m" in n]      # a library of its own
    assert C.sizeof(yuv.rrt_yuv_format) == 16
    f = rrt.YuvFormat()
    assert (f.struct_size, f.chroma, f.range, f.bits) == (16, 420, 0, 8)


def test_library_exports_exactly_what_the_header_declares():
    from relativisticraytracer_amd import build, yuv
    from test_capi import declared_functions
    build.build_lib()
    out = subprocess.run(["nm", "-D", "--defined-only", build.YUV_LIB], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)
    declared = declared_functions("rrt_yuv.h")
    assert exported == declared
    assert declared == sorted(n for n, _, _ in yuv.YUV_SYMBOLS)
    assert all(re.match(r"rrt_(yuv|y4m|launch_yuv)_", n) for n in declared), declared


@pytest.mark.parametrize("full,bits", [(False, 8), (True, 8), (False, 10), (True, 10)])
def test_coefficients_are_the_exactly_rounded_rationals(full, bits):
    Kr, Kb = Fraction(2126, 10000), Fraction(722, 10000)
    Kg = 1 - Kr - Kb
    K = [[Kr, Kg, Kb], [-Kr / (2 * (1 - Kb)), -Kg / (2 * (1 - Kb)), Fraction(1, 2)], [Fraction(1, 2), -Kg / (2 * (1 - Kr)), -Kb / (2 * (1 - Kr))]]
    A, off = yr.scales(full, bits)
    exact = [[(k * A[r] * 2 ** 30 / 65535 + Fraction(1, 2)).__floor__() for k in K[r]] for r in range(3)]
    for chroma in (420, 444):
        coef, offs = _rrt().yuv_coefficients(_fmt((chroma, full, bits)))
        assert coef.tolist() == exact
        assert offs.tolist() == off
    assert yr.coefficients(full, bits)[0].tolist() == exact                # the restatement's double formula agrees too
    if (full, bits) == (False, 8):
        assert exact == [[762841, 2566245, 259064], [-420488, -1414548, 1835036], [1835036, -1666774, -168262]]
        assert off == [16, 128, 128]
    k = 1 << (bits - 8)
    assert off == ([0, 128 * k, 128 * k] if full else [16 * k, 128 * k, 128 * k])


BLACK, WHITE, RED, GREEN, BLUE, GREY = (0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (128, 128, 128)
ANCHORS = {
    (False, 8): {BLACK: (16, 128, 128), WHITE: (235, 128, 128), RED: (63, 102, 240), GREEN: (173, 42, 26), BLUE: (32, 240, 118),
                 GREY: (126, 128, 128)},
    (True, 8): {BLACK: (0, 128, 128), WHITE: (255, 128, 128), RED: (54, 99, 255), BLUE: (18, 255, 116)},
    (False, 10): {BLACK: (64, 512, 512), WHITE: (940, 512, 512), RED: (250, 409, 960), BLUE: (127, 960, 471)},
    (True, 10): {WHITE: (1023, 512, 512), RED: (217, 395, 1023), BLUE: (74, 1023, 465)},
}


@pytest.mark.parametrize("full,bits", list(ANCHORS))
def test_anchor_colours_per_pixel_and_as_a_block(full, bits):
    rrt = _rrt()
    for rgb, want in ANCHORS[(full, bits)].items():
        for chroma in (420, 444):
            fmt = (chroma, full, bits)
            one = np.array([[list(rgb) + [7]]], np.uint8)                   # alpha is ignored
            assert tuple(_samples(rrt.yuv_from_rgba8_host(one, _fmt(fmt)), fmt)) == want, (rgb, fmt)
            block = _samples(rrt.yuv_from_rgba8_host(np.tile(one, (2, 2, 1)), _fmt(fmt)), fmt)
            n = 1 if chroma == 420 else 4
            assert block.tolist() == [want[0]] * 4 + [want[1]] * n + [want[2]] * n, (rgb, fmt)


@pytest.mark.parametrize("fmt", yr.FORMATS, **IDS)
def test_hdr_anchors(fmt):
    """H = 0 is black, +inf white; NaN and negative values (and -inf) are black"""
    rrt = _rrt()
    A, off = yr.scales(fmt[1], fmt[2])
    black, white = (off[0], off[1], off[2]), (off[0] + A[0], off[1], off[2])
    for v, want in ((0.0, black), (np.inf, white), (np.nan, black), (-3.0, black), (-np.inf, black), (-0.0, black)):
        one = np.full((1, 1, 4), v, F)
        assert tuple(_samples(rrt.yuv_from_hdr_host(one, _fmt(fmt)), fmt)) == want, (v, fmt)


def _real_codes(q, full, bits):
    """the real-valued BT.709 codes of (n, 3) sixteen-bit components, in float64, unrounded and unclamped"""
    A, off = yr.scales(full, bits)
    e = np.asarray(q, np.float64) / 65535.0
    return np.stack([np.asarray(yr.matrix()[r]) @ e.T * A[r] + off[r] for r in range(3)], axis=-1)


@pytest.mark.parametrize("full,bits", [(False, 8), (True, 8), (False, 10), (True, 10)])
def test_codes_mean_bt709_within_half_a_code(full, bits, po):
    """20 000 random colours through each input: every code within 0.501 of the float64 BT.709 value of the q it was computed
    from (0.5 from the final rounding, <= 3 * 0.5 * 65535 / 2^30 = 9.2e-5 from the rounded coefficients, the rest margin).  The
    ideal value lies inside the code range for every q, so the clamp does not enter."""
    rrt, rng, fmt = _rrt(), np.random.default_rng(709 + bits + full), (444, full, bits)
    n = 20000
    rgba = rng.integers(0, 256, (1, n, 4), dtype=np.uint8)
    got = _samples(rrt.yuv_from_rgba8_host(rgba, _fmt(fmt)), fmt).reshape(3, n).T
    err8 = np.abs(got - _real_codes(yr.q_from_rgba8(rgba)[0], full, bits)).max()
    hdr = np.zeros((1, n, 4), F)
    hdr[..., :3] = -np.log1p(-rng.uniform(0.0, 1.0, (1, n, 3))) / 0.8      # t roughly uniform over [0, 1)
    q = yr.q_from_hdr(po, hdr)[0]
    assert q.min() < 700 and q.max() > 64800 and len(np.unique(q)) > 20000      # sixteen-bit values, not bytes
    got = _samples(rrt.yuv_from_hdr_host(hdr, _fmt(fmt)), fmt).reshape(3, n).T
    err16 = np.abs(got - _real_codes(q, full, bits)).max()
    print(f"largest error, codes: from bytes {err8:.5f}, from HDR {err16:.5f}")
    assert err8 <= 0.501 and err16 <= 0.501


def test_restatement_tone_map_is_the_exposure_restatements(po):
    """yuv_ref.tone is exposure_ref.tone_map up to the cast: the same bytes from it"""
    rng = np.random.default_rng(3)
    rgb = np.exp2(rng.uniform(-12.0, 5.0, (500, 3))).astype(F)
    t = yr.tone(po, rgb)
    assert np.array_equal(np.trunc(t * F(255.0)).astype(np.int64) & 255, er.tone_map(po, rgb)[..., :3].astype(np.int64))


@pytest.mark.parametrize("fmt", yr.FORMATS, **IDS)
def test_host_conversions_equal_the_restatement(fmt, geometry, po):
    rrt, rng = _rrt(), np.random.default_rng(fmt[0] + fmt[2] + fmt[1])
    seen = set()
    for w, h in yr.sizes(geometry):
        seen.add(rrt.yuv_launch_geometry(_fmt(fmt), w, h)["wide"])
        rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        got = rrt.yuv_from_rgba8_host(rgba, _fmt(fmt))
        assert got.size == yr.frame_bytes(fmt, w, h)[0] == rrt.yuv_frame_bytes(_fmt(fmt), w, h)
        assert np.array_equal(got, yr.frame_from_rgba8(rgba, fmt)), (w, h)
        hdr = yr.hdr_frame(rng, w, h)
        assert np.array_equal(rrt.yuv_from_hdr_host(hdr, _fmt(fmt)), yr.frame_from_hdr(po, hdr, fmt)), (w, h)
    assert seen == {True, False}            # the list holds sizes of both launch paths (the GPU tests share it)


def test_geometry_names_the_strip_and_the_path():
    rrt = _rrt()
    g = rrt.yuv_launch_geometry(None, 64, 48)
    assert g["threads"] % 64 == 0 and g["strip_h"] == 2 and g["strip_w"] % 4 == 0 and g["wide"]
    assert not rrt.yuv_launch_geometry(None, 1023, 3)["wide"]          # the Cb plane starts at an odd address
    assert not rrt.yuv_launch_geometry(None, g["strip_w"] + 1, 4)["wide"]


@pytest.mark.parametrize("fmt", [(420, False, 8), (444, False, 8), (420, True, 10)], **IDS)
def test_flip_and_plane_order(fmt):
    """a frame whose bytes encode their own buffer (row, column) comes out top-down, Y then Cb then Cr, at plane_offset: with
    G = B = 0 luma grows with R, with R = B the chroma codes tell rows and columns apart"""
    rrt = _rrt()
    w, h = 6, 4
    n, offs = rrt.yuv_frame_bytes(_fmt(fmt), w, h, planes=True)
    assert (n, offs) == yr.frame_bytes(fmt, w, h)
    frame = np.zeros((h, w, 4), np.uint8)
    frame[..., 0] = (np.arange(h)[:, None] * 40 + np.arange(w)[None, :] * 5)      # R encodes (buffer row, column)
    frame[..., 2] = 255 - frame[..., 0]
    got = rrt.yuv_from_rgba8_host(frame, _fmt(fmt))
    bps = 1 if fmt[2] == 8 else 2
    Y = _samples(got[offs[0]:offs[1]], fmt).reshape(h, w)
    want = yr.planes(yr.q_from_rgba8(frame), fmt)
    assert np.array_equal(Y, want[0])
    # luma is monotonic in R - B here: the top display row is the LAST buffer row, and columns run left to right
    lum = yr.planes(yr.q_from_rgba8(frame[::-1]), fmt)[0]
    assert np.array_equal(Y[::-1], lum) and Y[0, 0] > Y[h - 1, 0] and Y[0, w - 1] > Y[0, 0]
    ch, cw = want[1].shape
    assert offs[2] - offs[1] == ch * cw * bps and n - offs[2] == ch * cw * bps
    assert np.array_equal(_samples(got[offs[1]:offs[2]], fmt).reshape(ch, cw), want[1])
    assert np.array_equal(_samples(got[offs[2]:], fmt).reshape(ch, cw), want[2])
    assert want[1][0, 0] < want[1][ch - 1, 0] and want[2][0, 0] > want[2][ch - 1, 0]      # Cb falls with R, Cr rises: rows are flipped


def test_y4m_header_and_frame_bytes():
    rrt = _rrt()
    expect = {
        (420, False, 8): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n",
        (444, False, 8): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C444 XCOLORRANGE=LIMITED\n",
        (420, True, 8): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n",
        (444, True, 8): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C444 XCOLORRANGE=FULL\n",
        (420, False, 10): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C420p10 XCOLORRANGE=LIMITED\n",
        (444, False, 10): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C444p10 XCOLORRANGE=LIMITED\n",
        (420, True, 10): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C420p10 XCOLORRANGE=FULL\n",
        (444, True, 10): b"YUV4MPEG2 W65 H47 F24:1 Ip A1:1 C444p10 XCOLORRANGE=FULL\n",
    }
    assert set(expect) == set(yr.FORMATS)
    for fmt, line in expect.items():
        assert rrt.y4m_header(_fmt(fmt), 65, 47) == line == yr.header(fmt, 65, 47)
        assert rrt.y4m_header(_fmt(fmt), 65, 47, cap=len(line)) == line            # an exact fit is enough: no NUL is written
        with pytest.raises(rrt.RRTError) as e:
            rrt.y4m_header(_fmt(fmt), 65, 47, cap=len(line) - 1)
        assert e.value.status == INVALID
    assert rrt.y4m_header(None, 1920, 1080, 30000, 1001) == b"YUV4MPEG2 W1920 H1080 F30000:1001 Ip A1:1 C420jpeg XCOLORRANGE=LIMITED\n"
    for num, den in ((0, 1), (24, 0), (-24, 1)):
        with pytest.raises(rrt.RRTError):
            rrt.y4m_header(None, 65, 47, num, den)
    assert rrt.yuv_frame_bytes(None, 3, 5, planes=True) == (15 + 6 + 6, (0, 15, 21))
    assert rrt.yuv_frame_bytes(_fmt((420, False, 10)), 3, 5, planes=True) == (54, (0, 30, 42))
    assert rrt.yuv_frame_bytes(_fmt((444, True, 8)), 3, 5, planes=True) == (45, (0, 15, 30))
    assert rrt.yuv_frame_bytes(_fmt((420, False, 8)), 1, 1) == 3
    assert rrt.yuv_frame_bytes(_fmt((420, False, 8)), 3840, 2160) == 3840 * 2160 * 3 // 2


def _bad_formats():
    rrt = _rrt()
    out = []
    for field, value in (("chroma", 422), ("chroma", 0), ("range", 2), ("range", -1), ("bits", 12), ("bits", 0)):
        f = rrt.YuvFormat()
        setattr(f, field, value)
        out.append((f, INVALID))
    f = rrt.YuvFormat()
    f.struct_size = 12
    out.append((f, ABI_MISMATCH))
    return out


def test_refusals_without_a_device():
    """every refusal of include/rrt_yuv.h, with made-up device addresses: a launch that passed the checks would fault on them"""
    from relativisticraytracer_amd import yuv
    rrt, lib = _rrt(), yuv.load()
    ok = rrt.YuvFormat()
    w, h = 64, 48
    n = rrt.yuv_frame_bytes(ok, w, h)
    out, src = FAKE, FAKE + (1 << 32)
    launches = (lib.rrt_launch_yuv_from_rgba8, lib.rrt_launch_yuv_from_hdr)
    for launch, src_bytes, src_align in zip(launches, (w * h * 4, w * h * 16), (4, 16)):
        assert launch(None, src, w, h, C.byref(ok), None) == INVALID
        assert launch(out, None, w, h, C.byref(ok), None) == INVALID
        assert launch(out, src, w, h, None, None) == INVALID
        for bw, bh in ((0, h), (w, 0), (-1, h), (w, -5), (1 << 16, 1 << 15), (46341, 46341)):
            assert launch(out, src, bw, bh, C.byref(ok), None) == INVALID, (bw, bh)
        for f, status in _bad_formats():
            assert launch(out, src, w, h, C.byref(f), None) == status
        for off in (1, 2, 4, 8):
            assert launch(out + off, src, w, h, C.byref(ok), None) == INVALID          # d_yuv: 16-byte aligned
        for off in (1, 2, 3, 4, 8):
            if off % src_align:
                assert launch(out, src + off, w, h, C.byref(ok), None) == INVALID
        # an output that overlaps the input: its first byte, its last, and the input inside the output
        assert launch(src, src, w, h, C.byref(ok), None) == INVALID
        assert launch(src + ((src_bytes - 16) & ~15), src, w, h, C.byref(ok), None) == INVALID
        assert launch(src - ((n - 1) & ~15), src, w, h, C.byref(ok), None) == INVALID
    # the host-only queries and conversions refuse the same sizes and formats
    bytes_out, hdr = C.c_size_t(0), (C.c_char * 160)()
    g, coef, off3 = (C.c_int32 * 4)(), (C.c_int64 * 9)(), (C.c_int32 * 3)()
    for f, status in _bad_formats():
        assert lib.rrt_yuv_coefficients(C.byref(f), C.byref(coef), C.byref(off3)) == status
        assert lib.rrt_yuv_frame_bytes(C.byref(f), w, h, C.byref(bytes_out), None) == status
        assert lib.rrt_y4m_header(C.byref(f), w, h, 24, 1, hdr, 160, C.byref(bytes_out)) == status
        assert lib.rrt_yuv_launch_geometry(C.byref(f), w, h, C.byref(g)) == status
    for bw, bh in ((0, h), (w, 0), (1 << 16, 1 << 15)):
        assert lib.rrt_yuv_frame_bytes(C.byref(ok), bw, bh, C.byref(bytes_out), None) == INVALID
        assert lib.rrt_yuv_launch_geometry(C.byref(ok), bw, bh, C.byref(g)) == INVALID
        assert lib.rrt_y4m_header(C.byref(ok), bw, bh, 24, 1, hdr, 160, C.byref(bytes_out)) == INVALID
    assert lib.rrt_yuv_frame_bytes(C.byref(ok), w, h, None, None) == INVALID
    assert lib.rrt_yuv_coefficients(C.byref(ok), None, C.byref(off3)) == INVALID
    assert lib.rrt_yuv_coefficients(C.byref(ok), C.byref(coef), None) == INVALID
    assert lib.rrt_yuv_coefficients(None, C.byref(coef), C.byref(off3)) == INVALID
    assert lib.rrt_yuv_launch_geometry(C.byref(ok), w, h, None) == INVALID
    assert lib.rrt_y4m_header(C.byref(ok), w, h, 24, 1, None, 160, C.byref(bytes_out)) == INVALID
    assert lib.rrt_y4m_header(C.byref(ok), w, h, 24, 1, hdr, 160, None) == INVALID
    assert lib.rrt_yuv_format_default(None) == INVALID
    buf = np.zeros(4 * 4 * 16 + 64, np.uint8)
    p = buf.ctypes.data
    for host in (lib.rrt_yuv_from_rgba8_host, lib.rrt_yuv_from_hdr_host):
        assert host(None, p, 4, 4, C.byref(ok)) == INVALID and host(p, None, 4, 4, C.byref(ok)) == INVALID
        assert host(p, p, 4, 4, C.byref(ok)) == INVALID and host(p + 8, p, 4, 4, C.byref(ok)) == INVALID
        assert host(p, p + 1024, 0, 4, C.byref(ok)) == INVALID
    assert not buf.any()                              # nothing was written
    assert lib.rrt_yuv_last_error() == b""            # and no HIP call was made
    with pytest.raises(rrt.RRTError) as e:
        rrt.launch_yuv_from_rgba8(out + 4, src, w, h)
    assert e.value.status == INVALID and "rrt_launch_yuv_from_rgba8" in str(e.value)


def test_y4m_sink_round_trip(tmp_path):
    from relativisticraytracer_amd import sinks
    rrt, rng = _rrt(), np.random.default_rng(5)
    for fmt in ((420, False, 8), (444, True, 10)):
        w, h = 7, 5
        path = tmp_path / f"s{fmt[0]}_{fmt[2]}.y4m"
        frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2)]
        sink = sinks.Y4MSink(str(path), w, h, 24, _fmt(fmt))
        for f in frames:
            sink.write(rrt.yuv_from_rgba8_host(f, _fmt(fmt)))
        with pytest.raises(ValueError):
            sink.write(np.zeros(sink.frame_bytes - 1, np.uint8))
        with pytest.raises(ValueError):
            sink.write(np.zeros(sink.frame_bytes + 1, np.uint8))
        sink.close()
        assert sink.frames == 2
        head, got = yr.parse_y4m(path.read_bytes(), fmt, w, h)
        assert head == yr.header(fmt, w, h) and len(got) == 2
        for f, g in zip(frames, got):
            assert np.array_equal(g, yr.frame_from_rgba8(f, fmt))
    assert isinstance(sinks.open_sink(str(tmp_path / "x.y4m"), 4, 4), sinks.PPMSink)       # --out keeps its meaning


# ---- the shared source under the sanitizers

@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/yuv/yuv_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("yuv")
    exe = str(d / "yuv_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "yuv", "yuv_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case, text):
        path = d / (case + ".txt")
        path.write_text(text)
        r = subprocess.run([exe, case, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip().endswith(case + " ok"), (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.strip().splitlines()[:-1]
    return run


def test_shared_source_under_sanitizers_equals_the_restatement(exerciser, po):
    """the odd sizes, input and output buffers sized exactly, through the source the library's host entry points and kernels run"""
    rng = np.random.default_rng(11)
    cases, text = [], []
    for fmt in yr.FORMATS:
        for w, h in ((1, 1), (1, 2), (2, 1), (3, 5), (7, 5), (9, 3), (65, 47)):
            rgba = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            hdr = yr.hdr_frame(rng, w, h)
            cases += [yr.frame_from_rgba8(rgba, fmt), yr.frame_from_hdr(po, hdr, fmt)]
            text.append(f"rgba {fmt[0]} {int(fmt[1])} {fmt[2]} {w} {h}\n" + " ".join(f"{v:x}" for v in rgba.ravel()) + "\n")
            text.append(f"hdr {fmt[0]} {int(fmt[1])} {fmt[2]} {w} {h}\n" + " ".join(f"{v:x}" for v in hdr.ravel().view(np.uint32)) + "\n")
    lines = exerciser("frames", "".join(text))
    assert len(lines) == len(cases)
    for line, want in zip(lines, cases):
        assert line == want.tobytes().hex()


# ---- the drivers' refusals: a table of its own (tests/test_driver_refusals.py's is closed), same conventions

NEEDED = "--y4m-chroma / --y4m-range / --y4m-depth need --y4m PATH"
NO_GLOW = "--y4m-depth 10 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow"
SAME_FILE = "--y4m and --out name the same file"
Y4M_ROWS = [
    (["--y4m-chroma", "444"], None, NEEDED),
    (["--y4m-range", "full"], None, NEEDED),
    (["--y4m-depth", "10"], None, NEEDED),
    (["--y4m", "a.y4m", "--y4m-chroma", "422"], None, "--y4m-chroma 420 | 444"),
    (["--y4m", "a.y4m", "--y4m-range", "tv"], None, "--y4m-range limited | full"),
    (["--y4m", "a.y4m", "--y4m-depth", "12"], None, "--y4m-depth 8 | 10"),
    (["--y4m", "a.y4m", "--y4m-depth", "10", "--glow", "0.25"], None, NO_GLOW),
    (["--y4m", "a.y4m", "--out", "a.y4m"], None, SAME_FILE),
    (["--y4m", "a.y4m", "--out", "./sub/../a.y4m"], None, SAME_FILE),
]
PY_ONLY = [(["--y4m", "a.y4m", "--y4m-depth", "10"], TWO_RANKS, "--y4m-depth 10: one GPU only (WORLD_SIZE > 1)")]
CPP_ONLY = [(["--y4m", "a.y4m", "--y4m-depth", "10", "--gpus", "2"], None, "--y4m-depth 10: one GPU only (--gpus 1)"),
            (["--y4m", "a.y4m", "--y4m-depth", "10", "--force-collective"], None, "--y4m-depth 10: one GPU only (--gpus 1)"),
            (["--y4m", "a.y4m", "--y4m-depth"], None, "--y4m-depth 8 | 10")]
ROW_IDS = dict(ids=lambda a: " ".join(a) if isinstance(a, list) else "")


@pytest.mark.parametrize("args,env,msg", Y4M_ROWS + PY_ONLY, **ROW_IDS)
def test_python_driver_refuses(args, env, msg):
    refused(PY, args, msg, env)


@pytest.mark.parametrize("args,env,msg", Y4M_ROWS + CPP_ONLY, **ROW_IDS)
def test_cpp_driver_refuses(args, env, msg):
    refused(CPP, args, "usage: " + msg, env)
