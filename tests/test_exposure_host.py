"""Exposure control (rrt_exposure_*, rrt_launch_exposure*, include/rrt.h) on a host without a GPU: the entry points are exported and
bound, the struct and its defaults are the documented ones, every refusal happens before the library touches a device, the bin
centres are log2 to 1e-12, the bin rule lands every edge case where the contract says, the host meter equals the numpy restatement
(tests/exposure_ref.py) on random frames, the resolve walk -- the source the resolve kernel runs, compiled for the host under ASan
and UBSan (tests/exposure/exposure_exerciser.cpp, a program of its own) -- equals the restatement bit for bit, the built kernels
use no scratch, and both headless drivers refuse what they must.  The frames themselves: tests/test_gpu_exposure.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import exposure_ref as er
from test_driver_refusals import CPP, IDS, PY, TWO_RANKS, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, ABI_MISMATCH = 1, 6
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it
F = np.float32


def _lib():
    from relativisticraytracer_amd import _lib
    return _lib.load()


def _exp(**kw):
    import relativisticraytracer_amd as rrt
    return rrt.ExposureSettings(**kw)


def test_symbols_are_exported_and_bound():
    from relativisticraytracer_amd import _lib
    import relativisticraytracer_amd as rrt
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in ("rrt_exposure_default", "rrt_exposure_bin_ev", "rrt_exposure_adapt", "rrt_exposure_scratch_bytes",
                 "rrt_exposure_meter_host", "rrt_launch_exposure_reset", "rrt_launch_exposure"):
        assert name in bound and hasattr(lib, name), name
    assert {"ExposureSettings", "exposure_scratch_bytes", "exposure_bin_ev", "exposure_adapt", "exposure_meter_host",
            "launch_exposure_reset", "launch_exposure"} <= set(rrt.__all__)
    assert lib.rrt_abi_version() == 5                      # no existing struct changed


def test_struct_layout_defaults_and_scratch_layout():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    e = _exp()
    assert e.struct_size == C.sizeof(e) == 40
    offs = [getattr(_lib.rrt_exposure, f[0]).offset for f in _lib.rrt_exposure._fields_]
    assert offs == list(range(0, 40, 4))
    assert (e.mode, e.ev, e.key, e.low_permille, e.high_permille, e.min_ev, e.max_ev, e.adapt_up, e.adapt_down) == \
        (rrt.EXPOSURE_MANUAL, 0.0, 0.5, 400, 20, -8.0, 8.0, 1.0, 1.0)
    assert _exp(mode="auto").mode == rrt.EXPOSURE_AUTO == 1
    with pytest.raises(AttributeError):
        _exp(nonexistent=1)
    assert _lib.load().rrt_exposure_default(None) == INVALID
    # the histogram, the 64-byte state, the table of doubles: 16-byte aligned sections
    assert (rrt.EXPOSURE_HIST_OFFSET, rrt.EXPOSURE_STATE_OFFSET, rrt.EXPOSURE_TABLE_OFFSET) == (0, 1024, 1088)
    assert rrt.exposure_scratch_bytes() == 1088 + 256 * 8 and rrt.exposure_scratch_bytes() % 16 == 0
    assert _lib.load().rrt_exposure_scratch_bytes(None) == INVALID
    hdr = open(os.path.join(ROOT, "include", "rrt.h")).read()
    for name, v in (("HIST", 0), ("STATE", 1024), ("TABLE", 1088)):
        assert f"#define RRT_EXPOSURE_{name}_OFFSET {v}\n" in hdr


def _launch(e, w=64, h=36, out=FAKE, hdr_out=0, hdr_in=FAKE + 0x100000, scratch=FAKE + 0x200000, nbytes=None):
    import relativisticraytracer_amd as rrt
    if nbytes is None:
        nbytes = rrt.exposure_scratch_bytes()
    p = lambda a: C.c_void_p(a) if a else None
    return _lib().rrt_launch_exposure(p(out), p(hdr_out), p(hdr_in), w, h, C.byref(e) if e is not None else None, p(scratch), nbytes,
                                      None)


BAD_SETTINGS = [dict(mode=2), dict(mode=-1), dict(ev=math.nan), dict(ev=math.inf), dict(key=0.0), dict(key=-0.5), dict(key=math.nan),
                dict(key=math.inf), dict(low_permille=-1), dict(high_permille=-1), dict(low_permille=600, high_permille=400),
                dict(low_permille=1000, high_permille=0), dict(low_permille=2 ** 31 - 1, high_permille=2 ** 31 - 1),
                dict(min_ev=1.0, max_ev=0.5), dict(min_ev=math.nan), dict(max_ev=math.nan), dict(min_ev=-math.inf), dict(max_ev=math.inf),
                dict(adapt_up=0.0), dict(adapt_up=-0.1), dict(adapt_up=1.5), dict(adapt_up=math.nan), dict(adapt_down=0.0),
                dict(adapt_down=1.0001), dict(adapt_down=math.nan)]


@pytest.mark.parametrize("mode", ["manual", "auto"])
def test_settings_refusals(mode):
    for kw in BAD_SETTINGS:
        e = _exp(**dict(dict(mode=mode), **kw))
        assert _launch(e) == INVALID, kw
    e = _exp(mode=mode)
    e.struct_size = 36
    assert _launch(e) == ABI_MISMATCH
    assert _launch(None) == INVALID
    ok = _exp(mode=mode, low_permille=999, high_permille=0, min_ev=2.0, max_ev=2.0, adapt_up=1e-30, adapt_down=1.0)
    assert _launch(ok, out=0, hdr_out=0) == INVALID               # the settings pass; both outputs NULL is the one refusal left


@pytest.mark.parametrize("mode", ["manual", "auto"])
def test_launch_refusals(mode):
    import relativisticraytracer_amd as rrt
    e = _exp(mode=mode)
    n = rrt.exposure_scratch_bytes()
    assert _launch(e, out=0, hdr_out=0) == INVALID                                    # both outputs NULL
    assert _launch(e, hdr_in=0) == INVALID
    for off in (1, 4, 8, 12):
        assert _launch(e, hdr_in=FAKE + 0x100000 + off) == INVALID, off               # misaligned HDR in / out
        assert _launch(e, hdr_out=FAKE + 0x300000 + off) == INVALID, off
    for off in (1, 2, 3):
        assert _launch(e, out=FAKE + off) == INVALID, off                             # the RGBA8 frame is stored as 4-byte pixels
    for ww, hh in ((0, 36), (64, 0), (-1, 36), (65536, 32768), (1 << 16, 1 << 15)):
        assert _launch(e, w=ww, h=hh) == INVALID, (ww, hh)                            # w * h >= 2^31: as the glow
    # an output that overlaps the input without being the input
    assert _launch(e, hdr_out=FAKE + 0x100000 + 16) == INVALID
    assert _launch(e, hdr_out=FAKE + 0x100000 + 64 * 36 * 16 - 16) == INVALID
    if mode == "auto":
        assert _launch(e, scratch=0) == INVALID
        assert _launch(e, nbytes=n - 1) == INVALID                                    # scratch one byte short
        for off in (1, 4, 8):
            assert _launch(e, scratch=FAKE + 0x200000 + off, nbytes=n + 64) == INVALID, off


def test_reset_and_host_query_refusals():
    import relativisticraytracer_amd as rrt
    lib, n = _lib(), rrt.exposure_scratch_bytes()
    assert lib.rrt_launch_exposure_reset(None, n, None) == INVALID
    assert lib.rrt_launch_exposure_reset(C.c_void_p(FAKE), n - 1, None) == INVALID
    assert lib.rrt_launch_exposure_reset(C.c_void_p(FAKE + 8), n + 64, None) == INVALID
    v = C.c_double(0.0)
    assert lib.rrt_exposure_bin_ev(-1, C.byref(v)) == INVALID and lib.rrt_exposure_bin_ev(256, C.byref(v)) == INVALID
    assert lib.rrt_exposure_bin_ev(0, None) == INVALID
    hist = np.zeros(256, np.uint32)
    px = np.zeros(4, np.float32)
    assert lib.rrt_exposure_meter_host(None, 1, 1, hist.ctypes.data) == INVALID
    assert lib.rrt_exposure_meter_host(px.ctypes.data, 1, 1, None) == INVALID
    assert lib.rrt_exposure_meter_host(px.ctypes.data, 0, 1, hist.ctypes.data) == INVALID
    assert lib.rrt_exposure_meter_host(px.ctypes.data, 1 << 16, 1 << 15, hist.ctypes.data) == INVALID


def test_adapt_is_the_documented_exponential():
    import relativisticraytracer_amd as rrt
    for dt, tau in ((1 / 24, 0.2), (1 / 24, 1.0), (1 / 60, 0.05), (0.5, 1e-3), (1 / 24, 1e9), (0.0, 1.0)):
        assert rrt.exposure_adapt(dt, tau) == F(1.0 - math.exp(-dt / tau)), (dt, tau)
    assert rrt.exposure_adapt(1 / 24, 0.0) == 1.0 and rrt.exposure_adapt(0.0, 0.0) == 1.0
    a = C.c_float(7.0)
    for dt, tau in ((-1.0, 1.0), (1.0, -1.0), (math.nan, 1.0), (1.0, math.nan), (math.inf, 1.0), (1.0, math.inf)):
        assert _lib().rrt_exposure_adapt(dt, tau, C.byref(a)) == INVALID and a.value == 7.0, (dt, tau)
    assert _lib().rrt_exposure_adapt(1.0, 1.0, None) == INVALID


def test_bin_centres_agree_with_numpy_log2():
    table = er.library_table(__import__("relativisticraytracer_amd"))
    want = er.bin_centres()
    assert np.max(np.abs(table - want)) <= 1e-12
    assert table[0] == -16.0 + math.log2(1.0 + 0.5 / 8.0) and abs(table[255] - (16.0 + math.log2(15.5 / 16.0))) <= 1e-12
    assert np.all(np.diff(table) > 0)
    # a bin's centre lies inside the bin: between the log2 of its two edges
    edges = (np.arange(257, dtype=np.uint32) + np.uint32(888)) << np.uint32(20)
    lo, hi = np.log2(edges[:-1].view(F).astype(np.float64)), np.log2(edges[1:].view(F).astype(np.float64))
    assert np.all((lo < table) & (table < hi))


def _bits(u):
    return np.array([u], np.uint32).view(F)[0]


EDGES = [  # (luma bits, metered, bin)
    (0x37800000, True, 0),                      # 2^-16: the first value of bin 0
    (0x377FFFFF, True, 0),                      # just below: clamped into bin 0
    (0x37800001, True, 0),
    (0x378FFFFF, True, 0), (0x37900000, True, 1),
    (0x47800000, True, 255),                    # 2^16: past the last octave, clamped into bin 255
    (0x477FFFFF, True, 255),                    # just below 2^16: the last value of bin 255
    (0x476FFFFF, True, 254), (0x47700000, True, 255),
    (0x3F800000, True, 128), (0x3F7FFFFF, True, 127),      # 1.0 opens bin 128
    (0x007FFFFF, True, 0),                      # the largest subnormal
    (0x00000001, True, 0),                      # the smallest
    (0x7F7FFFFF, True, 255),                    # FLT_MAX
    (0x00000000, False, 0), (0x80000000, False, 0),        # +-0
    (0xBF800000, False, 0), (0x80000001, False, 0),        # negative
    (0x7F800000, False, 0), (0xFF800000, False, 0),        # +-inf
    (0x7FC00000, False, 0), (0x7F800001, False, 0), (0xFFC00000, False, 0),   # NaN
]


def test_bin_edges_in_the_restatement_and_the_host_meter():
    import relativisticraytracer_amd as rrt
    for u, metered, b in EDGES:
        y = _bits(u)
        m, bb = er.bin_of(np.array([y], F))
        assert bool(m[0]) == metered and (not metered or int(bb[0]) == b), hex(u)
    # through the library: a pixel (0, g, 0) has luma g * 0.7152f; search the g whose product has the wanted bits where one exists,
    # otherwise (zero, negative, non-finite) feed the value itself
    for u, metered, b in EDGES:
        y = _bits(u)
        px = np.zeros((1, 1, 4), F)
        if metered:
            with np.errstate(over="ignore"):
                g = F(y / F(0.7152))
            cands = np.array([g, np.nextafter(g, F(np.inf)), np.nextafter(g, F(-np.inf))], F)
            hit = [c for c in cands if (F(F(0.0) + c * F(0.7152)) + F(0.0)).view(np.uint32) == np.uint32(u)]
            if not hit:
                continue                        # no float g gives exactly this luma: the exerciser feeds the bits directly
            px[0, 0, 1] = hit[0]
        else:
            px[0, 0, 1] = y
        hist = rrt.exposure_meter_host(px)
        assert int(hist.sum()) == (1 if metered else 0), hex(u)
        if metered:
            assert int(np.argmax(hist)) == b, hex(u)


def _random_frame(rng, w, h):
    """lumas spread log-uniformly over 2^-20 ... 2^20, with zeros, negatives and non-finite values mixed in"""
    hdr = (2.0 ** rng.uniform(-20.0, 20.0, (h, w, 1)) * rng.uniform(0.2, 1.8, (h, w, 3))).astype(F)
    hdr = np.concatenate([hdr, np.ones((h, w, 1), F)], axis=-1)
    r = rng.random((h, w))
    hdr[r < 0.05, :3] = 0.0
    hdr[(r >= 0.05) & (r < 0.08), :3] *= F(-1.0)
    hdr[(r >= 0.08) & (r < 0.10), 0] = np.nan
    hdr[(r >= 0.10) & (r < 0.12), 1] = np.inf
    hdr[(r >= 0.12) & (r < 0.13), 2] = -np.inf
    hdr[(r >= 0.13) & (r < 0.14), :3] = F(1e-42)              # subnormal lumas
    hdr[(r >= 0.14) & (r < 0.15), :3] = F(3e38)               # overflows to +inf in the sum: not metered
    return hdr


@pytest.mark.parametrize("w,h", [(1, 1), (7, 5), (257, 9), (300, 200)])
def test_host_meter_equals_the_restatement(w, h):
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(w * 1000 + h)
    hdr = _random_frame(rng, w, h)
    got, want = rrt.exposure_meter_host(hdr), er.histogram(hdr)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    if w * h > 1000:
        assert 0 < int(want.sum()) < w * h and want[0] > 0 and want[255] > 0 and (want > 0).sum() > 200


@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/exposure/exposure_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    d = tmp_path_factory.mktemp("exposure")
    exe = str(d / "exposure_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "exposure", "exposure_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case, text):
        path = d / (case + ".txt")
        path.write_text(text)
        r = subprocess.run([exe, case, str(path)], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip().endswith(case + " ok"), (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.strip().splitlines()[:-1]
    return run


def test_bin_rule_source_on_the_edge_bits(exerciser):
    """every edge value's bits through exposure_bin itself (the source the meter kernel and the host meter run)"""
    lines = exerciser("bins", "".join(f"{u:08x}\n" for u, _, _ in EDGES))
    assert len(lines) == len(EDGES)
    for ln, (u, metered, b) in zip(lines, EDGES):
        bits, got = ln.split()
        assert int(bits, 16) == u and int(got) == (b if metered else -1), ln


def _hex(x):
    return f"{int(np.array([x], F).view(np.uint32)[0]):08x}"


def _sparse(hist):
    nz = np.flatnonzero(hist)
    return f"frame {nz.size} " + " ".join(f"{b} {int(hist[b])}" for b in nz) + "\n"


def _hist(pairs):
    h = np.zeros(256, np.uint32)
    for b, c in pairs.items():
        h[b] = c
    return h


def _walk_cases():
    rng = np.random.default_rng(2026)
    smooth = dict(adapt_up=0.25, adapt_down=0.0625)
    cases = {
        # lo = 37 cuts bins 3 and 10 whole and bin 40 partially; hi = 18 cuts bin 250 whole and bin 200 partially
        "partial_cuts": (dict(low_permille=370, high_permille=180), [_hist({3: 10, 10: 20, 40: 30, 200: 35, 250: 5})]),
        "empty": (dict(ev=1.25), [_hist({}), _hist({}), _hist({100: 7}), _hist({})]),
        "empty_clamped": (dict(ev=5.0, min_ev=-2.0, max_ev=2.0), [_hist({}), _hist({90: 3})]),
        "one_pixel": (dict(low_permille=999, high_permille=0), [_hist({77: 1}), _hist({201: 1})]),
        # N = 1000, lo + hi = 999 = N - 1: one pixel is retained
        "all_but_one": (dict(low_permille=600, high_permille=399), [_hist({5: 300, 120: 300, 121: 1, 122: 399}),
                                                                      _hist({60: 1000})]),
        "all_in_bin_0": (dict(), [_hist({0: 123456})]),
        "all_in_bin_255": (dict(), [_hist({255: 2 ** 31 - 1})]),
        "both_ends": (dict(key=0.18, low_permille=0, high_permille=0), [_hist({0: 2 ** 31 - 1, 255: 2 ** 31 - 1})]),
        "asymmetric": (dict(key=0.18, ev=-0.5, **smooth),
                       [_hist({b: 50 + 3 * k}) for k, b in enumerate((60, 200, 210, 90, 30, 140, 140, 250))]),
        "range": (dict(min_ev=-1.0, max_ev=1.5, **smooth), [_hist({10: 9}), _hist({240: 9}), _hist({128: 9}), _hist({20: 9})]),
        "random": (dict(key=0.35, ev=0.3, low_permille=123, high_permille=77, adapt_up=0.7, adapt_down=0.2),
                   [rng.integers(0, 5000, 256).astype(np.uint32) * (rng.random(256) < 0.6) for _ in range(6)]),
    }
    return cases


def test_resolve_walk_under_sanitizers_equals_the_restatement(exerciser, po):
    """the resolve kernel's source, compiled for the host, against the restatement: N, m, target, ev and scale bit for bit over
    sequences on one state -- partial-bin cuts, empty frames, one pixel, lo + hi = N - 1, everything in bin 0 or 255, asymmetric
    adapt factors"""
    import relativisticraytracer_amd as rrt
    cases = _walk_cases()
    text = ""
    for name, (kw, frames) in cases.items():
        s = _exp(mode="auto", **kw)
        text += (f"case {name} {_hex(s.key)} {_hex(s.ev)} {s.low_permille} {s.high_permille} {_hex(s.min_ev)} {_hex(s.max_ev)} "
                 f"{_hex(s.adapt_up)} {_hex(s.adapt_down)} {len(frames)}\n")
        text += "".join(_sparse(h) for h in frames)
    lines = exerciser("walk", text)
    table = er.library_table(rrt)
    it = iter(lines)
    seen_partial = False
    for name, (kw, frames) in cases.items():
        s = _exp(mode="auto", **kw)
        st = er.State()
        for f, hist in enumerate(frames):
            n, m, target = st.step(hist, table, s)
            got = next(it).split()
            want_m = np.array([m if m is not None else 0.0], np.float64).view(np.uint64)[0]
            want = [name, str(f), str(n), f"{int(want_m):016x}", _hex(target if target is not None else 0.0), _hex(st.ev),
                    _hex(er.scale_of(po, st.ev)), str(st.frames)]
            assert got == want, (name, f)
        if name == "partial_cuts":
            # by hand: 37 off the bottom leaves 23 of bin 40; 18 off the top leaves 22 of bin 200
            kept = {40: 23, 200: 22}
            m_hand = sum(c * table[b] for b, c in sorted(kept.items())) / 45.0
            assert abs(m_hand - m) < 1e-12
            seen_partial = True
        if name == "empty":
            assert st.ev != F(1.25) and st.frames == 4          # frame 0 took the setting, frame 2 the metered target, frame 3 kept it
        if name == "one_pixel":
            assert (n, target) == (1, er.clamp(F(math.log2(0.5) - table[201]), -8, 8))
    assert seen_partial and next(it, None) is None


def test_restatement_resolve_properties():
    """the restatement against closed forms: a frame of one luminance is brought to the key; the cuts are percentiles"""
    import relativisticraytracer_amd as rrt
    table = er.library_table(rrt)
    s = _exp(mode="auto", key=0.5, low_permille=0, high_permille=0)
    for b in (0, 100, 128, 255):
        n, m, target = er.resolve(_hist({b: 1000}), table, s)
        assert (n, m) == (1000, table[b]) and target == er.clamp(F(-1.0 - table[b]), -8, 8)
    # 2^target * (the bin's centre luminance) == key, to the bin's width
    n, m, target = er.resolve(_hist({140: 10}), table, s)
    assert abs(2.0 ** float(target) * 2.0 ** table[140] - 0.5) < 1e-6
    # cutting 40 % off the bottom of a 50/50 frame leaves 10 dark + 50 bright of every 100
    cut = _exp(mode="auto", low_permille=400, high_permille=0)
    n, m, _ = er.resolve(_hist({50: 500, 150: 500}), table, cut)
    assert abs(m - (100 * table[50] + 500 * table[150]) / 600.0) < 1e-12
    # a per-mille pair that floors to nothing on a small frame
    n, m, _ = er.resolve(_hist({50: 1, 150: 1}), table, cut)
    assert abs(m - (table[50] + table[150]) / 2.0) < 1e-12


def test_exposure_kernels_in_the_built_library_use_no_scratch():
    """the four kernels are in librrt_hip.so's gfx950 code object, with no private segment, the meter's four wave histograms as its
    only LDS, and few enough registers for eight waves per SIMD (the code object's own metadata)"""
    import re
    import tempfile
    from relativisticraytracer_amd import build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_bytes as kb
    build.build_lib()
    with tempfile.TemporaryDirectory() as tmp:
        co = kb.code_object(build.LIB, tmp, "lib")
        notes = subprocess.run([kb.llvm_tool("llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    got = {}
    for blk in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        k = next((k for k in ("exposure_reset", "exposure_meter", "exposure_resolve", "exposure_apply") if k in name), None)
        if k:
            got[k] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, blk).group(1))
                      for f in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    assert set(got) == {"exposure_reset", "exposure_meter", "exposure_resolve", "exposure_apply"}, got
    for k, v in got.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= 64, (k, v)
        assert v["group_segment_fixed_size"] == (4 * 256 * 4 if k == "exposure_meter" else 0), (k, v)


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("args,msg", rows("exposure", PY), **IDS)
def test_python_driver_refuses(args, msg):
    refused(PY, args, msg)


SEVERAL_RANKS = {tuple(args): msg for args, msg in rows("exposure", PY, TWO_RANKS)}


@pytest.mark.parametrize("args", [list(args) for args in SEVERAL_RANKS], ids=lambda a: " ".join(a))
def test_python_driver_refuses_several_ranks(args):
    refused(PY, args, SEVERAL_RANKS[tuple(args)], TWO_RANKS)


@pytest.mark.parametrize("args,msg", rows("exposure", CPP), **IDS)
def test_cpp_driver_refuses(args, msg):
    refused(CPP, args, msg)
