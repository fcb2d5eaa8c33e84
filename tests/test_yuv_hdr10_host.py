"""HDR10 output without a GPU: librrt_yuv.so's host entry points (include/rrt_yuv.h, "HDR10 output") against the numpy restatement
(tests/hdr10_ref.py) byte for byte and, for the light-level state, word for word; the coefficients against exact rational rounding;
steps B-E against the same steps in float64; the PQ anchors, the shoulder, the light levels, the refusals, the sidecar, both drivers'
new refusals, and the shared source under AddressSanitizer and UndefinedBehaviorSanitizer (tests/yuv/hdr10_exerciser.cpp, a program
of its own)."""
import ctypes as C
import json
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import hdr10_ref as hr
import yuv_ref as yr
from test_driver_refusals import CPP, PY, TWO_RANKS, refused

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, ABI_MISMATCH = 1, 6
FAKE = 0x7777000000000000
F = np.float32
SETTINGS = [(203.0, peak, knee) for peak in (1000.0, 10000.0) for knee in (0.0, 0.5, 1.0)]
IDS = dict(ids=lambda s: f"peak{int(s[1])}-knee{s[2]}" if isinstance(s, tuple) else None)


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


def _fmt(fmt):
    return _rrt().YuvFormat(fmt[0], "full" if fmt[1] else "limited", fmt[2])


def _set(settings):
    return _rrt().Hdr10Settings(*settings)


def _state():
    from relativisticraytracer_amd import yuv
    return np.zeros(1, yuv.LIGHT_DTYPE)


def _samples(data):
    return np.asarray(data, np.uint8).view(np.dtype("<u2")).astype(np.int64)


@pytest.fixture(scope="module")
def geometry():
    return _rrt().yuv_launch_geometry(None, 64, 48)


def test_module_exports_and_the_structs():
    from relativisticraytracer_amd import yuv
    rrt = _rrt()
    for name in ("Hdr10Settings", "yuv_hdr10_coefficients", "yuv_hdr10_light_bytes", "launch_yuv_hdr10_from_hdr",
                 "launch_yuv_hdr10_light_reset", "yuv_hdr10_from_hdr_host", "yuv_hdr10_light_levels", "y4m_hdr10_sidecar"):
        assert name in rrt.__all__ and getattr(rrt, name) is getattr(yuv, name), name
    assert C.sizeof(yuv.rrt_yuv_hdr10) == 16 and C.sizeof(yuv.rrt_yuv_format) == 16
    assert C.sizeof(yuv.rrt_yuv_hdr10_light) == yuv.LIGHT_DTYPE.itemsize == rrt.yuv_hdr10_light_bytes() == 32
    s = rrt.Hdr10Settings()
    assert (s.struct_size, s.white_nits, s.peak_nits, s.knee) == (16, 203.0, 1000.0, 0.5)
    bound = {n for n, _, _ in yuv.YUV_SYMBOLS}
    assert {"rrt_yuv_hdr10_default", "rrt_yuv_hdr10_coefficients", "rrt_yuv_hdr10_light_bytes", "rrt_launch_yuv_hdr10_from_hdr",
            "rrt_launch_yuv_hdr10_light_reset", "rrt_yuv_hdr10_from_hdr_host", "rrt_yuv_hdr10_light_levels",
            "rrt_y4m_hdr10_sidecar"} <= bound


@pytest.mark.parametrize("settings", SETTINGS, **IDS)
def test_host_conversion_equals_the_restatement_bytes_and_state(settings, geometry, po):
    """the four 10-bit formats over the shared sizes; A-D and the metering are computed once per size and shared by the formats"""
    rrt, rng = _rrt(), np.random.default_rng(int(settings[1] + 10 * settings[2]))
    seen = set()
    for w, h in yr.sizes(geometry):
        hdr = yr.hdr_frame(rng, w, h)
        c = hr.nits(po, hdr, settings)
        q = hr.pq(po, c)
        want_state = hr.state_words(hr.meter(c, hr.new_state()))
        for fmt in hr.FORMATS:
            seen.add(rrt.yuv_launch_geometry(_fmt(fmt), w, h)["wide"])
            state = _state()
            got = rrt.yuv_hdr10_from_hdr_host(hdr, _fmt(fmt), _set(settings), state)
            assert got.size == yr.frame_bytes(fmt, w, h)[0]
            assert np.array_equal(got, yr.pack(hr.planes(q, fmt), 10)), (fmt, w, h)
            assert state.tobytes() == want_state, (fmt, w, h)
            assert np.array_equal(rrt.yuv_hdr10_from_hdr_host(hdr, _fmt(fmt), _set(settings)), got)      # light NULL: the same planes
    assert seen == {True, False}


def test_coefficients_are_the_exactly_rounded_rationals():
    Kr, Kb = Fraction(2627, 10000), Fraction(593, 10000)
    Kg = 1 - Kr - Kb
    K = [[Kr, Kg, Kb], [-Kr / (2 * (1 - Kb)), -Kg / (2 * (1 - Kb)), Fraction(1, 2)], [Fraction(1, 2), -Kg / (2 * (1 - Kr)), -Kb / (2 * (1 - Kr))]]
    for full in (False, True):
        A, off = yr.scales(full, 10)
        exact = [[(k * A[r] * 2 ** 30 / 65535 + Fraction(1, 2)).__floor__() for k in K[r]] for r in range(3)]
        for chroma in (420, 444):
            coef, offs = _rrt().yuv_hdr10_coefficients(_fmt((chroma, full, 10)))
            assert coef.tolist() == exact and offs.tolist() == off
        assert hr.coefficients(full)[0].tolist() == exact
        assert exact != _rrt().yuv_coefficients(_fmt((420, full, 10)))[0].tolist()          # not BT.709's
    assert _rrt().yuv_hdr10_coefficients()[1].tolist() == [64, 512, 512]


def _pq64(c):
    y = np.asarray(c, np.float64) * 1.0e-4
    p = y ** 0.1593017578125
    return ((0.8359375 + 18.8515625 * p) / (1.0 + 18.6875 * p)) ** 78.84375


# the largest errors measured by the test below (2^20 colours, seed 2084), see its docstring
MEASURED_Q, MEASURED_CODE = 0.8854, 0.5096


def test_steps_b_to_e_against_float64(po):
    """2^20 colours (3 * 2^20 channels), each channel's light log-uniform over 2^-24 ... 10^4 nits (white_nits = 1: H is nits),
    at the default peak and knee: steps B-D in binary32 with rrt_expf / rrt_powf against the same steps in float64 with numpy's exp and
    pow, on q (|q - 65535 PQ64|, unrounded) and on the 10-bit 4:4:4 codes of both ranges (|code - real-valued code|).  The bound
    was not fixed in advance: it is the largest error measured here plus 10 % -- a change of rrt_powf shows, the last-place noise of
    numpy's pow does not.  Measured: q 0.8854 (0.5 of it is the final rounding; the rest is under 1/100 of a 10-bit code), codes 0.5096 (0.5 the rounding)."""
    n, rng = 1 << 20, np.random.default_rng(2084)
    settings = (1.0, 1000.0, 0.5)
    a = np.exp(rng.uniform(np.log(2.0 ** -24), np.log(1.0e4), (n, 3))).astype(F)
    b = hr.gamut(hr.light(a, settings))
    q = hr.pq(po, hr.shoulder(po, b, settings))
    G = np.array([[float(g) for g in row] for row in hr.GAMUT])          # the binary32 literals, as the definition writes them
    b64 = a.astype(np.float64) @ G.T
    K, span = 500.0, 500.0
    c64 = np.minimum(np.where(b64 <= K, b64, K + span * (1.0 - np.exp(-(np.maximum(b64, K) - K) / span))), 1000.0)
    e64 = _pq64(c64)
    err_q = float(np.abs(q - 65535.0 * e64).max())
    err_code = 0.0
    for full in (False, True):
        A, off = yr.scales(full, 10)
        for r in range(3):
            real = (e64 @ np.asarray(hr.matrix()[r])) * A[r] + off[r]
            err_code = max(err_code, float(np.abs(hr.code(q, r, 0, full) - real).max()))
    print(f"largest error over {n} colours: q {err_q:.4f}, 10-bit codes {err_code:.4f}")
    assert q.min() < 10 and q.max() > 49000
    assert err_q <= MEASURED_Q * 1.1 and err_code <= MEASURED_CODE * 1.1


def test_pq_anchors(po):
    """step D alone"""
    nits = np.array([0.0, 100.0, 203.0, 1000.0, 10000.0], F)
    assert hr.pq(po, nits).tolist() == [0, 33297, 38056, 49271, 65535]
    # through the library: black, and +inf at peak 10000 (q 65535: white), in both ranges
    rrt = _rrt()
    for full in (False, True):
        A, off = yr.scales(full, 10)
        for v, y in ((0.0, off[0]), (np.inf, off[0] + A[0]), (np.nan, off[0]), (-2.0, off[0]), (-np.inf, off[0])):
            got = rrt.yuv_hdr10_from_hdr_host(np.full((1, 1, 4), v, F), _fmt((444, full, 10)), _set((203.0, 10000.0, 0.5)))
            assert _samples(got).tolist() == [y, 512, 512], (v, full)


@pytest.mark.parametrize("settings", [(203.0, 1000.0, 0.5), (203.0, 1000.0, 0.25), (100.0, 4000.0, 0.75), (203.0, 10000.0, 0.0)], **IDS)
def test_shoulder_is_continuous_and_monotone_across_the_knee(settings, po):
    _, peak, _, K, span, _ = hr.derived(settings)
    ulp = np.spacing(max(K, F(1.0e-30)))
    b = (K + np.arange(-3000, 3001, dtype=np.float64) * float(ulp)).astype(F)           # adjacent floats around K
    b = np.unique(np.maximum(b, F(0.0)))
    c = hr.shoulder(po, b, settings)
    assert (np.diff(c.astype(np.float64)) >= 0.0).all()
    assert np.array_equal(c[b <= K], b[b <= K])                                       # the identity up to K
    # slope 1 at K, so no step: within 3000 floats of K the curve leaves the identity by the rounding of 1.0f - rrt_expf(-x) alone,
    # an absolute 2^-24 of the subtraction and as much of the exp near 1, times span (at knee 0 that is all there is: K = 0)
    assert float(np.abs(c.astype(np.float64) - b.astype(np.float64)).max()) <= 4.0 * float(ulp) + float(span) * 2.0 ** -22
    wide = np.concatenate([np.exp2(np.linspace(-24.0, 40.0, 20001)), [np.inf]]).astype(F)
    cw = hr.shoulder(po, wide, settings)
    assert (np.diff(cw.astype(np.float64)) >= 0.0).all() and cw.max() == peak and cw[-1] == peak


def test_knee_one_is_the_hard_clip(po):
    settings = (203.0, 1000.0, 1.0)
    b = np.array([0.0, 1.0, 999.99994, 1000.0, 1000.0001, 5000.0, np.inf], F)
    assert np.array_equal(hr.shoulder(po, b, settings), np.minimum(b, F(1000.0)))


def test_light_levels():
    rrt = _rrt()
    from relativisticraytracer_amd import yuv
    # ceilings in integers
    for cll, s, w, h, want in ((0, 0, 4, 4, (0, 0)), (64 * 5, 64 * 16 * 7, 4, 4, (5, 7)), (64 * 5 + 1, 64 * 16 * 7 + 1, 4, 4, (6, 8)),
                               (640000, 8192 * 640000, 128, 64, (10000, 10000)), (1, 1, 7680, 4320, (1, 1))):
        st = np.zeros(1, yuv.LIGHT_DTYPE)
        st["max_cll"], st["max_frame_sum"], st["frames"] = cll, s, 3
        assert rrt.yuv_hdr10_light_levels(st, w, h) == {"max_cll": want[0], "max_fall": want[1], "frames": 3}
        assert hr.levels({"max_cll": cll, "max_frame_sum": s, "frames": 3}, w, h) == {"max_cll": want[0], "max_fall": want[1], "frames": 3}
    # 128 x 64 of +inf at peak 10000: the frame's sum passes 2^32
    state = _state()
    rrt.yuv_hdr10_from_hdr_host(np.full((64, 128, 4), np.inf, F), None, _set((203.0, 10000.0, 0.5)), state)
    assert int(state["max_frame_sum"][0]) == 8192 * 640000 > 1 << 32 and int(state["max_cll"][0]) == 640000
    assert (int(state["frame_sum"][0]), int(state["frame_max"][0]), int(state["frames"][0]), int(state["reserved"][0])) == (0, 0, 1, 0)
    assert rrt.yuv_hdr10_light_levels(state, 128, 64) == {"max_cll": 10000, "max_fall": 10000, "frames": 1}


def test_the_clamped_420_edge_is_metered_once():
    """3 x 5, 4:2:0: the last column and the last row are read twice for the chroma sums and counted once"""
    rrt = _rrt()
    hdr = np.zeros((5, 3, 4), F)
    hdr[..., :3] = 1.0                    # 203 nits, under the knee: gray stays gray up to the gamut's rounding
    hdr[0, 2, :3] = 2.0                   # the display's bottom-right pixel: on the doubled column and the doubled row
    for fmt in ((420, False, 10), (444, False, 10)):
        state = _state()
        rrt.yuv_hdr10_from_hdr_host(hdr, _fmt(fmt), None, state)
        one = _state()
        rrt.yuv_hdr10_from_hdr_host(hdr[1:2, :1], _fmt(fmt), None, one)
        two = _state()
        rrt.yuv_hdr10_from_hdr_host(hdr[:1, 2:], _fmt(fmt), None, two)
        assert int(state["max_frame_sum"][0]) == 14 * int(one["max_frame_sum"][0]) + int(two["max_frame_sum"][0])
        assert int(state["max_cll"][0]) == int(two["max_cll"][0]) > int(one["max_cll"][0]) > 0


def test_max_fall_is_the_largest_frame_mean_not_the_mean(po):
    rrt, rng = _rrt(), np.random.default_rng(8613)
    w, h = 7, 5
    frames = [yr.hdr_frame(rng, w, h) * F(s) for s in (1.0e-3, 1.0, 1.0e-5)]
    frames[1][..., :3] = np.minimum(np.nan_to_num(frames[1][..., :3], nan=0.0, posinf=1.0, neginf=0.0), F(1.5))
    state, want, sums = _state(), hr.new_state(), []
    for f in frames:
        rrt.yuv_hdr10_from_hdr_host(f, None, None, state)
        before = want["max_frame_sum"]
        hr.meter(hr.nits(po, f, hr.DEFAULT), want)
        single = hr.meter(hr.nits(po, f, hr.DEFAULT), hr.new_state())
        sums.append(single["max_frame_sum"])
        assert want["max_frame_sum"] == max(before, sums[-1])
    assert state.tobytes() == hr.state_words(want) and want["frames"] == 3
    assert want["max_frame_sum"] == max(sums) and len(set(sums)) == 3 and max(sums) * 3 > sum(sums)
    assert rrt.yuv_hdr10_light_levels(state, w, h) == hr.levels(want, w, h)
    assert hr.levels(want, w, h)["max_fall"] == -(-max(sums) // (64 * w * h))


def _bad_settings():
    rrt = _rrt()
    out = []
    for field, value in (("white_nits", np.nan), ("white_nits", np.inf), ("white_nits", 0.0), ("white_nits", -203.0),
                         ("white_nits", 10000.5), ("peak_nits", np.nan), ("peak_nits", np.inf), ("peak_nits", -np.inf),
                         ("peak_nits", 0.0), ("peak_nits", -1.0), ("peak_nits", 10001.0), ("knee", -0.001), ("knee", 1.001), ("knee", np.nan)):
        s = rrt.Hdr10Settings()
        setattr(s, field, value)
        out.append((s, INVALID))
    s = rrt.Hdr10Settings()
    s.struct_size = 12
    out.append((s, ABI_MISMATCH))
    return out


def _bad_formats():
    rrt = _rrt()
    out = []
    for field, value in (("bits", 8), ("bits", 12), ("chroma", 422), ("range", 2)):
        f = rrt.YuvFormat(bits=10)
        setattr(f, field, value)
        out.append((f, INVALID))
    f = rrt.YuvFormat(bits=10)
    f.struct_size = 12
    out.append((f, ABI_MISMATCH))
    return out


def test_refusals_without_a_device():
    """every refusal of the settings and of the format, with made-up device addresses: a launch that passed the checks would use them"""
    from relativisticraytracer_amd import yuv
    rrt, lib = _rrt(), yuv.load()
    ok, st = rrt.YuvFormat(bits=10), rrt.Hdr10Settings()
    w, h = 64, 48
    n = rrt.yuv_frame_bytes(ok, w, h)
    out, src, light = FAKE, FAKE + (1 << 32), FAKE + (1 << 33)
    launch = lib.rrt_launch_yuv_hdr10_from_hdr
    assert launch(None, src, w, h, C.byref(ok), C.byref(st), light, None) == INVALID
    assert launch(out, None, w, h, C.byref(ok), C.byref(st), light, None) == INVALID
    assert launch(out, src, w, h, None, C.byref(st), light, None) == INVALID
    assert launch(out, src, w, h, C.byref(ok), None, light, None) == INVALID
    for bw, bh in ((0, h), (w, 0), (-1, h), (1 << 16, 1 << 15)):
        assert launch(out, src, bw, bh, C.byref(ok), C.byref(st), light, None) == INVALID
    for s, status in _bad_settings():
        assert launch(out, src, w, h, C.byref(ok), C.byref(s), light, None) == status
        assert launch(out, src, w, h, C.byref(ok), C.byref(s), None, None) == status
    for f, status in _bad_formats():
        assert launch(out, src, w, h, C.byref(f), C.byref(st), light, None) == status
    for off in (1, 2, 4, 8):
        assert launch(out + off, src, w, h, C.byref(ok), C.byref(st), light, None) == INVALID
        assert launch(out, src + off, w, h, C.byref(ok), C.byref(st), light, None) == INVALID
        assert launch(out, src, w, h, C.byref(ok), C.byref(st), light + off, None) == INVALID      # d_light: 16-byte aligned
        assert lib.rrt_launch_yuv_hdr10_light_reset(light + off, None) == INVALID
    assert lib.rrt_launch_yuv_hdr10_light_reset(None, None) == INVALID
    assert launch(src, src, w, h, C.byref(ok), C.byref(st), light, None) == INVALID              # the output overlaps the input
    # a state that overlaps the input or the output: their first and last 32 bytes
    for base, size in ((src, w * h * 16), (out, n)):
        assert launch(out, src, w, h, C.byref(ok), C.byref(st), base, None) == INVALID
        assert launch(out, src, w, h, C.byref(ok), C.byref(st), base + ((size - 1) & ~15), None) == INVALID
        assert launch(out, src, w, h, C.byref(ok), C.byref(st), base - 16, None) == INVALID
    # the host-only entry points
    coef, off3, lv, nb = (C.c_int64 * 9)(), (C.c_int32 * 3)(), (C.c_uint32 * 3)(), C.c_size_t(0)
    for f, status in _bad_formats():
        assert lib.rrt_yuv_hdr10_coefficients(C.byref(f), C.byref(coef), C.byref(off3)) == status
    assert lib.rrt_yuv_hdr10_coefficients(None, C.byref(coef), C.byref(off3)) == INVALID
    assert lib.rrt_yuv_hdr10_coefficients(C.byref(ok), None, C.byref(off3)) == INVALID
    assert lib.rrt_yuv_hdr10_default(None) == INVALID and lib.rrt_yuv_hdr10_light_bytes(None) == INVALID
    state = _state()
    sp = state.ctypes.data
    assert lib.rrt_yuv_hdr10_light_levels(None, w, h, C.byref(lv)) == INVALID
    assert lib.rrt_yuv_hdr10_light_levels(sp, w, h, None) == INVALID
    assert lib.rrt_yuv_hdr10_light_levels(sp, 0, h, C.byref(lv)) == INVALID
    assert lib.rrt_yuv_hdr10_light_levels(sp, 1 << 16, 1 << 15, C.byref(lv)) == INVALID
    buf = np.zeros(4 * 4 * 16 + 256, np.uint8)
    p = buf.ctypes.data
    host = lib.rrt_yuv_hdr10_from_hdr_host
    assert host(None, p, 4, 4, C.byref(ok), C.byref(st), None) == INVALID and host(p, None, 4, 4, C.byref(ok), C.byref(st), None) == INVALID
    assert host(p, p, 4, 4, C.byref(ok), C.byref(st), None) == INVALID
    assert host(p + 256, p, 4, 4, C.byref(ok), C.byref(st), p + 64) == INVALID                    # the state inside the input
    for s, status in _bad_settings():
        assert host(p + 256, p, 4, 4, C.byref(ok), C.byref(s), sp) == status
    for f, status in _bad_formats():
        assert host(p + 256, p, 4, 4, C.byref(f), C.byref(st), sp) == status
    text = C.create_string_buffer(1024)
    assert lib.rrt_y4m_hdr10_sidecar(None, C.byref(lv), text, 1024, C.byref(nb)) == INVALID
    assert lib.rrt_y4m_hdr10_sidecar(C.byref(st), None, text, 1024, C.byref(nb)) == INVALID
    assert lib.rrt_y4m_hdr10_sidecar(C.byref(st), C.byref(lv), None, 1024, C.byref(nb)) == INVALID
    assert lib.rrt_y4m_hdr10_sidecar(C.byref(st), C.byref(lv), text, 1024, None) == INVALID
    assert lib.rrt_y4m_hdr10_sidecar(C.byref(st), C.byref(lv), text, 16, C.byref(nb)) == INVALID
    for s, status in _bad_settings():
        assert lib.rrt_y4m_hdr10_sidecar(C.byref(s), C.byref(lv), text, 1024, C.byref(nb)) == status
    assert not buf.any() and not state.tobytes().strip(b"\0") and not text.raw.strip(b"\0")      # nothing was written
    assert lib.rrt_yuv_last_error() == b""                                                       # and no HIP call was made
    with pytest.raises(rrt.RRTError) as e:
        rrt.launch_yuv_hdr10_from_hdr(out, src, w, h, rrt.YuvFormat(bits=8))
    assert e.value.status == INVALID and "rrt_launch_yuv_hdr10_from_hdr" in str(e.value)


def test_sidecar_bytes_and_the_sink(tmp_path):
    from relativisticraytracer_amd import sinks
    rrt = _rrt()
    lv = {"max_cll": 987, "max_fall": 123, "frames": 2}
    want = (b'{\n'
            b'  "white_nits": 203,\n'
            b'  "peak_nits": 1000,\n'
            b'  "knee": 0.5,\n'
            b'  "max_cll": 987,\n'
            b'  "max_fall": 123,\n'
            b'  "frames": 2,\n'
            b'  "master_display": "G(8500,39850)B(6550,2300)R(35400,14600)WP(15635,16450)L(10000000,1)",\n'
            b'  "x265": "--colorprim bt2020 --transfer smpte2084 --colormatrix bt2020nc --master-display '
            b'\\"G(8500,39850)B(6550,2300)R(35400,14600)WP(15635,16450)L(10000000,1)\\" --max-cll \\"987,123\\"",\n'
            b'  "ffmpeg": "-color_primaries bt2020 -color_trc smpte2084 -colorspace bt2020nc"\n'
            b'}\n')
    assert rrt.y4m_hdr10_sidecar(None, lv) == want == hr.sidecar(hr.DEFAULT, lv)
    odd = (180.5, 4000.0, 0.3)
    assert rrt.y4m_hdr10_sidecar(_set(odd), lv) == hr.sidecar(odd, lv)
    doc = json.loads(rrt.y4m_hdr10_sidecar(_set(odd), lv))
    assert doc["peak_nits"] == 4000 and doc["white_nits"] == 180.5 and abs(doc["knee"] - 0.3) < 1e-7 and doc["max_fall"] == 123
    assert doc["master_display"].endswith("L(40000000,1)") and '--max-cll "987,123"' in doc["x265"]
    # the sink: an HDR10 film closes with its levels and leaves the sidecar; an SDR film leaves none
    w, h, fmt = 7, 5, (420, False, 10)
    rng = np.random.default_rng(6)
    path = tmp_path / "f.y4m"
    sink = sinks.Y4MSink(str(path), w, h, 24, _fmt(fmt), rrt.Hdr10Settings())
    state, frames = _state(), [yr.hdr_frame(rng, w, h) for _ in range(2)]
    packed = [rrt.yuv_hdr10_from_hdr_host(f, _fmt(fmt), None, state) for f in frames]
    for b in packed:
        sink.write(b)
    with pytest.raises(ValueError):
        sink.close()
    levels = rrt.yuv_hdr10_light_levels(state, w, h)
    sink.close(levels)
    head, got = yr.parse_y4m(path.read_bytes(), fmt, w, h)
    assert head == yr.header(fmt, w, h) and all(np.array_equal(g, b) for g, b in zip(got, packed)) and len(got) == 2
    assert (tmp_path / "f.y4m.hdr10.json").read_bytes() == hr.sidecar(hr.DEFAULT, levels) and levels["frames"] == 2
    plain = sinks.Y4MSink(str(tmp_path / "s.y4m"), w, h, 24, _fmt(fmt))
    plain.close()
    assert sorted(os.listdir(tmp_path)) == ["f.y4m", "f.y4m.hdr10.json", "s.y4m"]


# ---- the shared source under the sanitizers

@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/yuv/hdr10_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("hdr10")
    exe = str(d / "hdr10_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "yuv", "hdr10_exerciser.cpp"), "-o", exe], check=True)
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
    """the odd sizes, the input sized exactly, guard bytes around every plane and around the state; each frame is packed and folded
    twice, so the state shows the maxima kept and two frames counted"""
    rng = np.random.default_rng(12)
    want, text = [], []
    for fmt in hr.FORMATS:
        for (w, h), settings in zip(((1, 1), (1, 2), (2, 1), (3, 5), (7, 5), (9, 3), (65, 47)), SETTINGS + [(100.0, 600.0, 0.25)]):
            hdr = yr.hdr_frame(rng, w, h)
            state = hr.new_state()
            hr.meter(hr.nits(po, hdr, settings), state)
            want += [hr.frame(po, hdr, fmt, settings, state).tobytes().hex(), hr.state_words(state).hex()]
            assert state["frames"] == 2
            bits = " ".join(f"{v:x}" for v in np.array(settings, F).view(np.uint32))
            text.append(f"{fmt[0]} {int(fmt[1])} {w} {h} {bits}\n" + " ".join(f"{v:x}" for v in hdr.ravel().view(np.uint32)) + "\n")
    lines = exerciser("frames", "".join(text))
    assert lines == want


# ---- the drivers' refusals

PQ_NEEDS = "--y4m-transfer pq needs --y4m PATH and --y4m-depth 10"
HDR_NEEDS = "--hdr-white / --hdr-peak / --hdr-knee need --y4m-transfer pq"
NITS = "--hdr-white / --hdr-peak NITS: in (0, 10000]"
KNEE = "--hdr-knee F: in [0, 1]"
NO_GLOW = "--y4m-depth 10 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow"
PQ = ["--y4m", "a.y4m", "--y4m-depth", "10", "--y4m-transfer", "pq"]
ROWS = [
    (["--y4m", "a.y4m", "--y4m-transfer", "hlg"], None, "--y4m-transfer sdr | pq"),
    (["--y4m-transfer", "pq"], None, PQ_NEEDS),
    (["--y4m-depth", "10", "--y4m-transfer", "pq"], None, PQ_NEEDS),
    (["--y4m", "a.y4m", "--y4m-transfer", "pq"], None, PQ_NEEDS),
    (["--y4m", "a.y4m", "--y4m-depth", "8", "--y4m-transfer", "pq"], None, PQ_NEEDS),
    (["--y4m-transfer", "sdr"], None, "--y4m-transfer needs --y4m PATH"),
    (["--hdr-white", "100"], None, HDR_NEEDS),
    (["--y4m", "a.y4m", "--y4m-depth", "10", "--hdr-peak", "600"], None, HDR_NEEDS),
    (["--y4m", "a.y4m", "--y4m-depth", "10", "--y4m-transfer", "sdr", "--hdr-knee", "0.5"], None, HDR_NEEDS),
    (PQ + ["--hdr-white", "0"], None, NITS),
    (PQ + ["--hdr-white", "nan"], None, NITS),
    (PQ + ["--hdr-peak", "10001"], None, NITS),
    (PQ + ["--hdr-peak", "inf"], None, NITS),
    (PQ + ["--hdr-peak", "-5"], None, NITS),
    (PQ + ["--hdr-knee", "1.5"], None, KNEE),
    (PQ + ["--hdr-knee", "-0.1"], None, KNEE),
    (PQ + ["--hdr-knee", "nan"], None, KNEE),
    (PQ + ["--glow", "0.25"], None, NO_GLOW),
]
PY_ONLY = [(PQ, TWO_RANKS, "--y4m-depth 10: one GPU only (WORLD_SIZE > 1)")]
CPP_ONLY = [(PQ + ["--gpus", "2"], None, "--y4m-depth 10: one GPU only (--gpus 1)"),
            (["--y4m", "a.y4m", "--y4m-transfer"], None, "--y4m-transfer sdr | pq"),
            (PQ + ["--hdr-peak", "bright"], None, NITS)]
ROW_IDS = dict(ids=lambda a: " ".join(a) if isinstance(a, list) else "")


@pytest.mark.parametrize("args,env,msg", ROWS + PY_ONLY, **ROW_IDS)
def test_python_driver_refuses(args, env, msg):
    refused(PY, args, msg, env)


@pytest.mark.parametrize("args,env,msg", ROWS + CPP_ONLY, **ROW_IDS)
def test_cpp_driver_refuses(args, env, msg):
    refused(CPP, args, "usage: " + msg, env)
