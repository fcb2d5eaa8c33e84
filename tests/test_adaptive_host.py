"""Adaptive supersampling (rrt_launch_raymarch_adaptive, rrt_adaptive_mask; include/rrt.h) on a host without a GPU: the host mask
query against its numpy restatement (tests/adaptive_ref.py), every refusal before the library touches a device, the refine kernel's
vacuum step and register budget, and both headless drivers' refusals.  The frames themselves: tests/test_gpu_adaptive.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref
from test_driver_refusals import CPP, IDS, PY, TWO_RANKS, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, BAD_HANDLE, ABI_MISMATCH = 1, 4, 6
NO_SKY = 0x7777000000000001          # never a registered sky: a launch that passes every check stops at the handle lookup
THRESHOLDS = (0, 8, 255)


def test_symbols_are_exported_and_bound():
    from relativisticraytracer_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in ("rrt_adaptive_default", "rrt_adaptive_scratch_bytes", "rrt_adaptive_mask", "rrt_launch_raymarch_adaptive"):
        assert name in bound and hasattr(lib, name), name


def test_default_is_threshold_8():
    import relativisticraytracer_amd as rrt
    ad = rrt.AdaptiveSettings()
    assert ad.threshold == 8 and ad.struct_size == C.sizeof(rrt.rrt_adaptive) == 8
    assert rrt.AdaptiveSettings(17).info() == {"threshold": 17}
    assert rrt._lib.load().rrt_adaptive_default(None) == INVALID


# ---------------------------------------------------------------- the mask
def _check_mask(frame, T):
    import relativisticraytracer_amd as rrt
    got, count = rrt.adaptive_mask(frame, rrt.AdaptiveSettings(T))
    want = adaptive_ref.mask(frame, T)
    assert got.dtype == np.uint8 and got.shape == want.shape and set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want), (frame.shape, T, int((got.astype(bool) != want).sum()))
    assert count == int(want.sum()) == int(got.sum())
    if T == 255:
        assert count == 0 and not got.any()
    return count


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (7, 5), (33, 17), (64, 96)])
def test_mask_equals_the_restatement_on_random_frames(shape):
    """white noise (every pixel refined at T = 0 and 8), smooth noise whose neighbours differ by a few steps (the threshold
    decides), and a flat frame with a differing alpha channel (nothing refined at any T)"""
    h, w = shape
    rng = np.random.default_rng(1000 * h + w)
    noise = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    walk = (128 + np.cumsum(np.cumsum(rng.integers(-6, 7, (h, w, 4)), axis=0), axis=1) // 3).clip(0, 255).astype(np.uint8)
    near = (rng.integers(0, 2, (h, w, 4)) * 9 + 100).astype(np.uint8)                # differences of exactly 0 or 9: T = 8 < 9
    flat = np.full((h, w, 4), 77, np.uint8)
    flat[..., 3] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for T in THRESHOLDS:
        for frame in (noise, walk, near):
            _check_mask(frame, T)
        assert _check_mask(flat, T) == 0
    # the comparison is strict: a step of exactly T is not refined, T + 1 is
    step = np.zeros((h, w, 4), np.uint8)
    step[:, w // 2:, 1] = 9
    assert _check_mask(step, 9) == 0
    assert _check_mask(step, 8) == (2 * h if w > 1 else 0)


def test_mask_equals_the_restatement_on_the_golden_frames(frames_gold):
    n, refined = 0, 0
    for key, frame in frames_gold.items():
        if not key.endswith("_rgba8"):
            continue
        for T in THRESHOLDS:
            c = _check_mask(frame, T)
            refined += c if T == 8 else 0
        n += 1
    assert n >= 8 and refined > 0


def test_mask_ignores_alpha_and_does_not_wrap():
    import relativisticraytracer_amd as rrt
    f = np.zeros((4, 6, 4), np.uint8)
    f[:, 0, 0] = 200                     # the left column differs from the right one: a wrap would refine column 5
    m, n = rrt.adaptive_mask(f, rrt.AdaptiveSettings(8))
    assert n == 8 and m[:, :2].all() and not m[:, 2:].any()
    f[..., 3] = np.arange(24, dtype=np.uint8).reshape(4, 6) * 10
    assert np.array_equal(rrt.adaptive_mask(f, rrt.AdaptiveSettings(8))[0], m)


def test_mask_refusals():
    import relativisticraytracer_amd as rrt
    lib = rrt._lib.load()
    f, m, ad = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4), np.uint8), rrt.AdaptiveSettings()
    fp, mp = f.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p)
    assert lib.rrt_adaptive_mask(fp, 4, 4, C.byref(ad), mp, None) == 0
    assert lib.rrt_adaptive_mask(None, 4, 4, C.byref(ad), mp, None) == INVALID
    assert lib.rrt_adaptive_mask(fp, 4, 4, C.byref(ad), None, None) == INVALID
    assert lib.rrt_adaptive_mask(fp, 4, 4, None, mp, None) == INVALID
    assert lib.rrt_adaptive_mask(fp, 0, 4, C.byref(ad), mp, None) == INVALID
    assert lib.rrt_adaptive_mask(fp, 4, -1, C.byref(ad), mp, None) == INVALID
    for T in (-1, 256):
        assert lib.rrt_adaptive_mask(fp, 4, 4, C.byref(rrt.AdaptiveSettings(T)), mp, None) == INVALID
    bad = rrt.AdaptiveSettings()
    bad.struct_size = 12
    assert lib.rrt_adaptive_mask(fp, 4, 4, C.byref(bad), mp, None) == ABI_MISMATCH


# ---------------------------------------------------------------- the launch's refusals
def test_scratch_bytes_and_its_refusals():
    import relativisticraytracer_amd as rrt
    lib = rrt._lib.load()
    assert rrt.adaptive_scratch_bytes(96, 64) == 16 + 4 * 96 * 64
    assert rrt.adaptive_scratch_bytes(1, 1) == 32 and rrt.adaptive_scratch_bytes(67, 45) % 16 == 0
    assert rrt.adaptive_scratch_bytes(67, 45) >= 16 + 4 * 67 * 45
    n = C.c_size_t(0)
    assert lib.rrt_adaptive_scratch_bytes(96, 64, None) == INVALID
    for w, h in ((0, 64), (96, 0), (-1, 64), (65536, 32768)):
        assert lib.rrt_adaptive_scratch_bytes(w, h, C.byref(n)) == INVALID, (w, h)


def _launch(w=64, h=36, s=2, out=1, ad="default", scratch=4096, scratch_bytes=None, proj=None, cam=True, fx=True, prm=None):
    import relativisticraytracer_amd as rrt
    c, f, p = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams()
    a = rrt.AdaptiveSettings() if isinstance(ad, str) else ad
    if scratch_bytes is None:
        scratch_bytes = 16 + 4 * max(w, 1) * max(h, 1) + 16
    return rrt._lib.load().rrt_launch_raymarch_adaptive(
        C.c_void_p(out) if out else None, None, w, h, s, C.byref(proj) if proj is not None else None,
        C.byref(a) if a is not None else None, 1.0, C.byref(c) if cam else None, NO_SKY, C.byref(f) if fx else None,
        C.byref(prm if prm is not None else p), C.c_void_p(scratch) if scratch else None, scratch_bytes, None)


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_good_arguments_pass_the_checks(s):
    """... and reach the sky lookup, which refuses the made-up handle: no check said no"""
    import relativisticraytracer_amd as rrt
    assert _launch(37, 21, s) == BAD_HANDLE
    assert _launch(37, 21, s, scratch_bytes=rrt.adaptive_scratch_bytes(37, 21)) == BAD_HANDLE
    for T in (0, 255):
        assert _launch(37, 21, s, ad=rrt.AdaptiveSettings(T)) == BAD_HANDLE
    for kind in ("pinhole", "equirect", "fisheye"):
        assert _launch(32, 32, s, proj=rrt.Projection(kind)) == BAD_HANDLE
    # the ignored params are ignored, as in rrt_launch_raymarch_ss
    assert _launch(37, 21, s, prm=rrt.RenderParams(workspace=12345, tile_order=54321, path_policy=2)) == BAD_HANDLE


def test_adaptive_refusals():
    import relativisticraytracer_amd as rrt
    assert _launch(out=0) == INVALID                              # NULL pointers
    assert _launch(ad=None) == INVALID
    assert _launch(scratch=0) == INVALID
    assert _launch(cam=False) == INVALID and _launch(fx=False) == INVALID
    for T in (-1, 256, 1 << 20):                                  # the threshold's range
        assert _launch(ad=rrt.AdaptiveSettings(T)) == INVALID, T
    for s in (0, -1, 3, 5, 6, 7, 16):                             # the factor
        assert _launch(s=s) == INVALID, s
    need = rrt.adaptive_scratch_bytes(64, 36)                     # a short or misaligned scratch
    assert _launch(scratch_bytes=need - 1) == INVALID and _launch(scratch_bytes=0) == INVALID
    assert _launch(scratch_bytes=need) == BAD_HANDLE
    for off in (1, 4, 8):
        assert _launch(scratch=4096 + off) == INVALID, off
    for size in (0, 4, 12, 16):                                   # another struct_size
        bad = rrt.AdaptiveSettings()
        bad.struct_size = size
        assert _launch(ad=bad) == ABI_MISMATCH, size


def test_everything_the_supersampled_launch_refuses_is_refused():
    import relativisticraytracer_amd as rrt
    assert _launch(0, 36) == INVALID and _launch(64, 0) == INVALID and _launch(-3, 36) == INVALID
    assert _launch(65536, 32768, scratch_bytes=1 << 40) == INVALID                   # w h >= 2^31
    assert _launch(8192, 8192, 8, scratch_bytes=1 << 40) == INVALID                  # the virtual frame's limits
    assert _launch(8192, 8192, 4, scratch_bytes=1 << 40) == BAD_HANDLE
    assert _launch(1, 65536, 8, scratch_bytes=1 << 40) == INVALID and _launch(1, 65535, 8, scratch_bytes=1 << 40) == BAD_HANDLE
    assert _launch(prm=rrt.RenderParams(max_steps=-1)) == INVALID
    assert _launch(prm=rrt.RenderParams(arith_mode=7)) == INVALID
    p40 = rrt.RenderParams()
    p40.struct_size = 40
    assert _launch(prm=p40) == ABI_MISMATCH
    # the projection's refusals (rrt_launch_raymarch_pano)
    assert _launch(proj=rrt.Projection("equirect", fov_deg=400.0)) == INVALID
    assert _launch(proj=rrt.Projection("fisheye", fov_deg=0.0)) == INVALID
    bad = rrt.Projection("equirect")
    bad.kind = 9
    assert _launch(proj=bad) == INVALID
    bad = rrt.Projection("equirect")
    bad.struct_size = 8
    assert _launch(proj=bad) == ABI_MISMATCH


# ---------------------------------------------------------------- the refine kernel's code
def _isa(*kernels):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_histogram.py")] + list(kernels),
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-1500:]
    got, name = {}, None
    for ln in r.stdout.splitlines():
        if ln.startswith("== "):
            name = ln[3:].strip()
            got[name] = {}
        m = re.search(r"registers: (\d+) VGPR, (\d+) SGPR, occupancy (\d+) waves/SIMD, scratch (\d+) B", ln)
        if m and name:
            got[name].update(vgpr=int(m.group(1)), occupancy=int(m.group(3)), scratch=int(m.group(4)))
        m = re.search(r"VACUUM LOOP \(nested, body written out (\d+)x\).*?(\d+) VALU \((\d+) v_mov\) = ([0-9.]+) VALU per RK4 step", ln)
        if m and name:
            got[name].update(unroll=int(m.group(1)), mov=int(m.group(3)), per_step=float(m.group(4)))
    return got, r.stdout


def test_refine_kernel_keeps_the_vacuum_step_and_the_register_budget():
    """refine_pixels runs the sampled kernels' march unchanged: per arithmetic mode and ray kind its nested vacuum loop costs what
    supersample_pixels' / panorama_pixels' does per RK4 step in the same build (the counting is tools/isa_histogram.py's), with no
    scratch, no more VGPRs than theirs and raymarch_pixels' 5-wave budget."""
    pairs = {}
    for arith in (0, 2):
        pairs[f"refine_pixels<true, 2, {arith}, (SampledRay)0>"] = f"supersample_pixels<true, 2, {arith}>"
        pairs[f"refine_pixels<true, 2, {arith}, (SampledRay)1>"] = f"panorama_pixels<true, 2, {arith}>"
    got, out = _isa("refine_pixels<true, 2, 0,", "refine_pixels<true, 2, 2,", *sorted(set(pairs.values())))
    names = {k: [n for n in got if n.replace("(anonymous namespace)::", "").startswith(k)] for k in list(pairs) + list(pairs.values())}
    for k, v in names.items():
        assert len(v) == 1, (k, sorted(got), out[-1500:])
    for new, old in pairs.items():
        g, ref = got[names[new][0]], got[names[old][0]]
        assert g.get("unroll") == 2 and g["mov"] == 0, (new, g)
        assert g["per_step"] == ref["per_step"], (new, g, ref)
        assert g["scratch"] == 0, (new, g)
        assert g["vgpr"] <= ref["vgpr"], (new, g, ref)
        assert g["occupancy"] >= 5, (new, g)


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("args,msg", rows("adaptive", PY), **IDS)
def test_python_driver_refuses(args, msg):
    refused(PY, args, msg)


def test_python_driver_refuses_several_gpus():
    for args, msg in rows("adaptive", PY, TWO_RANKS):
        refused(PY, args, msg, TWO_RANKS)


@pytest.mark.parametrize("args,msg", rows("adaptive", CPP), **IDS)
def test_cpp_driver_refuses(args, msg):
    refused(CPP, args, msg)
