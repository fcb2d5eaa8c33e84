"""HDR glow (rrt_glow_*, rrt_launch_glow, include/rrt.h) on a host without a GPU: the entry points are exported and bound, every
refusal happens before the library touches a device, the taps are the documented double-precision Gaussians, the numpy
restatement (tests/glow_ref.py) is itself right, the kernels compile for gfx950 without scratch, and both headless drivers refuse
a bad or multi-GPU --glow.  The frames themselves: tests/test_gpu_glow.py."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import glow_ref
from test_driver_refusals import CPP, PY, TWO_RANKS, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, ABI_MISMATCH = 1, 6
FAKE = 0x7777000000000000             # a made-up, 16-byte aligned device address: a launch that passes every check would use it


def _lib():
    from relativisticraytracer_amd import _lib
    return _lib.load()


def _glow(**kw):
    import relativisticraytracer_amd as rrt
    return rrt.GlowSettings(**kw)


def test_symbols_are_exported_and_bound():
    from relativisticraytracer_amd import _lib
    import relativisticraytracer_amd as rrt
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in ("rrt_glow_default", "rrt_glow_weights", "rrt_glow_scratch_bytes", "rrt_launch_glow"):
        assert name in bound and hasattr(lib, name), name
    assert {"GlowSettings", "glow_weights", "glow_scratch_bytes", "launch_glow"} <= set(rrt.__all__)


def test_defaults():
    g = _glow()
    assert g.struct_size == C.sizeof(g) == 20
    assert (g.radius, g.lobes, g.threshold, g.intensity) == (np.float32(0.004), 4, 1.0, 0.25)


def _bytes(w, h, g):
    n = C.c_size_t(0)
    rc = _lib().rrt_glow_scratch_bytes(w, h, C.byref(g) if g is not None else None, C.byref(n))
    return rc, n.value


def _launch(w, h, g, out=FAKE, hdr=FAKE + 0x100000, scratch=FAKE + 0x200000, nbytes=None):
    if nbytes is None:
        nbytes = _bytes(w, h, g)[1]
    return _lib().rrt_launch_glow(C.c_void_p(out) if out else None, C.c_void_p(hdr) if hdr else None, w, h,
                                  C.byref(g) if g is not None else None, C.c_void_p(scratch) if scratch else None, nbytes, None)


def _bad_settings():
    bad = [dict(lobes=0), dict(lobes=5), dict(lobes=-1), dict(radius=0.0), dict(radius=-0.001), dict(radius=math.nan),
           dict(radius=math.inf), dict(threshold=-0.5), dict(threshold=math.nan), dict(threshold=math.inf),
           dict(intensity=-0.01), dict(intensity=math.nan), dict(intensity=math.inf)]
    return [_glow(**kw) for kw in bad]


def test_scratch_query_is_the_planes_and_the_taps():
    for w, h, kw in ((3840, 2160, {}), (97, 61, dict(lobes=2, radius=0.05)), (1, 1, dict(lobes=1))):
        g = _glow(**kw)
        rc, n = _bytes(w, h, g)
        assert rc == 0
        taps = sum(2 * math.ceil(3 * g.radius * h * 2 ** l) + 1 for l in range(g.lobes))
        assert n == g.lobes * w * h * 16 + (taps * 4 + 15) // 16 * 16, (w, h, kw)


def test_settings_refusals():
    for g in _bad_settings():
        assert _bytes(64, 36, g)[0] == INVALID, g.info()
        assert _launch(64, 36, g, nbytes=1 << 40) == INVALID, g.info()
        assert _lib().rrt_glow_weights(C.byref(g), 36, 0, None, 0, None) == INVALID, g.info()
    g = _glow()
    g.struct_size = 16
    assert _bytes(64, 36, g)[0] == ABI_MISMATCH and _launch(64, 36, g, nbytes=1 << 40) == ABI_MISMATCH
    assert _lib().rrt_glow_weights(C.byref(g), 36, 0, None, 0, None) == ABI_MISMATCH
    assert _bytes(64, 36, None)[0] == INVALID and _launch(64, 36, None, nbytes=1 << 40) == INVALID


def test_widest_lobe_limit():
    """R_{L-1} = ceil(3 sigma_{L-1}) <= 1024, sigma_l = radius * height * 2^l"""
    h = 1000
    ok = _glow(lobes=4, radius=1024 / 3 / 8 / h * (1 - 1e-6))         # R_3 = 1024
    r = C.c_int(0)
    assert _lib().rrt_glow_weights(C.byref(ok), h, 3, None, 0, C.byref(r)) == 0 and r.value == 1024
    assert _bytes(4, h, ok)[0] == 0
    over = _glow(lobes=4, radius=1024 / 3 / 8 / h * (1 + 1e-5))       # R_3 = 1025
    assert _bytes(4, h, over)[0] == INVALID and _launch(4, h, over, nbytes=1 << 40) == INVALID
    one = _glow(lobes=1, radius=over.radius)                           # the same radius with one lobe is narrow enough
    assert _bytes(4, h, one)[0] == 0


def test_launch_refusals():
    g = _glow(lobes=2, radius=0.01)
    w, h = 64, 36
    n = _bytes(w, h, g)[1]
    assert _launch(w, h, g, nbytes=n - 1) == INVALID                                  # scratch one byte short
    assert _launch(w, h, g, out=0) == INVALID
    assert _launch(w, h, g, hdr=0) == INVALID
    assert _launch(w, h, g, scratch=0) == INVALID
    for off in (4, 8, 12, 1):
        assert _launch(w, h, g, hdr=FAKE + 0x100000 + off) == INVALID, off            # misaligned HDR
        assert _launch(w, h, g, scratch=FAKE + 0x200000 + off, nbytes=n + 64) == INVALID, off
    for ww, hh in ((0, 36), (64, 0), (-1, 36), (65536, 32768), (1 << 16, 1 << 15)):
        assert _launch(ww, hh, g, nbytes=1 << 60) == INVALID, (ww, hh)                # w * h >= 2^31
        assert _bytes(ww, hh, g)[0] == INVALID, (ww, hh)
    assert _bytes(65535, 32768, _glow(lobes=1, radius=1e-5))[0] == 0                   # just under 2^31 pixels


def test_weights_query_refusals():
    g = _glow(lobes=2, radius=0.01)
    r = C.c_int(0)
    buf = (C.c_float * 64)()
    lib = _lib()
    assert lib.rrt_glow_weights(C.byref(g), 100, 0, None, 0, C.byref(r)) == 0 and r.value == 3
    assert lib.rrt_glow_weights(C.byref(g), 100, 0, buf, 6, C.byref(r)) == INVALID            # cap < 2R + 1
    assert lib.rrt_glow_weights(C.byref(g), 100, 0, buf, 7, None) == 0
    assert lib.rrt_glow_weights(C.byref(g), 100, 2, buf, 64, None) == INVALID                 # lobe >= L
    assert lib.rrt_glow_weights(C.byref(g), 100, -1, buf, 64, None) == INVALID
    assert lib.rrt_glow_weights(C.byref(g), 0, 0, buf, 64, None) == INVALID


@pytest.mark.parametrize("h", [1, 37, 540, 1080, 2160])
def test_weights_are_the_documented_gaussians(h):
    import relativisticraytracer_amd as rrt
    for radius in (0.004, 0.0123, 0.05):
        sig = [(float(np.float32(radius)) * h) * 2.0 ** l for l in range(4)]
        lobes = sum(math.ceil(3 * s) <= 1024 for s in sig)         # the widest lobe the settings may have
        if lobes == 0:
            continue
        g = _glow(radius=radius, lobes=lobes)
        for l, sigma in enumerate(sig[:lobes]):
            w = rrt.glow_weights(g, h, l)
            r = (w.size - 1) // 2
            assert r == math.ceil(3 * sigma) and w.dtype == np.float32, (h, radius, l)
            assert np.array_equal(w, w[::-1])
            k = np.arange(-r, r + 1, dtype=np.float64)
            e = np.exp(-(k * k) / (2.0 * sigma * sigma))
            want = e / math.fsum(e)
            assert np.all(np.abs(w.astype(np.float64) - want) <= np.spacing(want.astype(np.float32))), (h, radius, l)
            assert abs(float(np.sum(w.astype(np.float64))) - 1.0) <= 4 * 2 ** -24 * math.sqrt(w.size), (h, radius, l)


def test_restatement_impulse_is_the_outer_product():
    """one bright pixel far from the edges, threshold 0 (B = H), intensity L (s = 1): G is w_l w_l^T summed over the lobes"""
    taps = [np.array([0.25, 0.5, 0.25], np.float32), np.array([0.0625, 0.25, 0.375, 0.25, 0.0625], np.float32)]
    H = np.zeros((11, 13, 4), np.float32)
    H[5, 6, :3] = (2.0, 1.0, 4.0)
    out = glow_ref.glow_hdr(H, taps, 0.0, float(len(taps)))
    G = out - H[..., :3]
    want = np.zeros((11, 13), np.float64)
    for t in taps:
        r = (t.size - 1) // 2
        want[5 - r:5 + r + 1, 6 - r:6 + r + 1] += np.outer(t, t)
    for c, v in enumerate((2.0, 1.0, 4.0)):
        assert np.allclose(G[..., c], want * v, rtol=1e-6, atol=1e-7), c
    for c in range(3):
        assert G[..., c][want == 0].max() == 0


def test_restatement_conserves_energy_and_matches_a_float64_convolution():
    """away from the edges the glow moves light, it does not make it; everywhere it is the 2-D convolution with clamped edges"""
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(5)
    h, w = 48, 71
    g = _glow(lobes=3, radius=0.02)
    taps = glow_ref.lobe_taps(rrt, g, h)
    H = np.zeros((h, w, 4), np.float32)
    H[12:36, 18:52, :3] = rng.uniform(0.0, 6.0, (24, 34, 3)).astype(np.float32)
    out = glow_ref.glow_hdr(H, taps, 1.0, 0.6)
    B = np.stack(glow_ref.bright_pass(H, 1.0), -1).astype(np.float64)
    s = float(np.float32(0.6) / np.float32(3))
    G = (out - H[..., :3]).astype(np.float64)
    assert abs(G.sum() / s - B.sum() * 3) <= 1e-4 * B.sum() * 3
    want = np.zeros_like(B)
    for t in taps:
        r = (t.size - 1) // 2
        t64 = t.astype(np.float64)
        hx = sum(t64[k + r] * B[:, np.clip(np.arange(w) + k, 0, w - 1)] for k in range(-r, r + 1))
        want += sum(t64[k + r] * hx[np.clip(np.arange(h) + k, 0, h - 1)] for k in range(-r, r + 1))
    assert np.allclose(G / s, want, rtol=1e-5, atol=1e-6 * want.max())


def test_restatement_bright_pass_is_a_soft_knee():
    H = np.array([[[0.5, 0.5, 0.5, 1], [1.0, 1.0, 1.0, 1], [2.0, 2.0, 2.0, 1], [8.0, 0.0, 0.0, 1]]], np.float32)
    r, g, b = glow_ref.bright_pass(H, 1.0)
    assert r[0, 0] == 0 and r[0, 1] == 0                                  # at or below T: nothing
    assert abs(r[0, 2] - 1.0) < 1e-6                                      # (2 - 1) / 2 * 2
    luma = np.float32(8.0) * np.float32(0.2126)
    assert r[0, 3] == np.float32(8.0) * ((luma - np.float32(1)) / luma) and g[0, 3] == 0


def _resource_usage(kernels):
    from relativisticraytracer_amd import build
    d = tempfile.mkdtemp(prefix="rrt_glow_isa_")
    cmd = [build.hipcc_path()] + [f for f in build.HIPCC_FLAGS if f != "-shared"] + \
        ["-Rpass-analysis=kernel-resource-usage", "-c"] + build.SOURCES + ["-o", os.path.join(d, "x.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=d, timeout=1500)
    assert r.returncode == 0, r.stderr[-2000:]
    got, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = next((k for k in kernels if k in m.group(1)), None)
            if name:
                got[name] = {}
            continue
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", ln)
        if m and name:
            got[name][m.group(1).split()[0]] = int(m.group(2))
    return got


def test_glow_kernels_compile_for_gfx950_without_scratch():
    got = _resource_usage(("glow_hpass", "glow_vpass", "glow_load_weights"))
    assert set(got) == {"glow_hpass", "glow_vpass", "glow_load_weights"}, got
    for k, v in got.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["Occupancy"] >= 2, (k, v)


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("bad", rows("glow", PY))
def test_python_driver_refuses_bad_glow_arguments(bad):
    refused(PY, *bad)


def test_python_driver_refuses_glow_on_several_ranks():
    for args, msg in rows("glow", PY, TWO_RANKS):
        refused(PY, args, msg, TWO_RANKS)


def test_cpp_driver_refuses_bad_or_multi_gpu_glow():
    for args, msg in rows("glow", CPP):
        refused(CPP, args, msg)
