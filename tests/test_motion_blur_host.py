"""Motion-blurred frames (rrt_launch_raymarch_mb*, rrt_motion_clock, include/rrt.h) on a host without a GPU: the entry points are
exported and bound, every refusal happens before the library touches a device, the shutter clock is the documented binary32
arithmetic, the kernel keeps the march's vacuum step and register budget, and both headless drivers refuse a bad --motion-blur or
--shutter.  The frames themselves: tests/test_gpu_motion_blur.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_supersample_host import _isa
from test_driver_refusals import CPP, PY, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, BAD_HANDLE, ABI_MISMATCH = 1, 4, 6
NO_SKY = 0x7777000000000001          # never a registered sky: a launch that passes every check stops at the handle lookup


def test_symbols_are_exported_and_bound():
    from relativisticraytracer_amd import _lib
    import relativisticraytracer_amd as rrt
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in ("rrt_launch_raymarch_mb", "rrt_launch_raymarch_mb_tiles", "rrt_motion_clock"):
        assert name in bound and hasattr(lib, name), name
    assert {"launch_raymarch_mb", "launch_raymarch_mb_tiles"} <= set(rrt.__all__)


def _subs(n, times=None):
    import relativisticraytracer_amd as rrt
    t = times if times is not None else [1.0 + 0.01 * k for k in range(n)]
    return (C.c_float * len(t))(*t), (rrt_camera_array(len(t)))(*[rrt.CameraState.default() for _ in t])


def rrt_camera_array(n):
    from relativisticraytracer_amd import _lib
    return _lib.rrt_camera * n


def _mb(w, h, s, n, out=1, times=True, cams=True, fx=True, prm=None, tv=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    t, c = _subs(max(n, 1), tv)
    return _lib.load().rrt_launch_raymarch_mb(C.c_void_p(out) if out else None, None, w, h, s, n, t if times else None,
                                              c if cams else None, NO_SKY, C.byref(rrt.CameraEffects()) if fx else None,
                                              C.byref(prm if prm is not None else rrt.RenderParams()), None)


def _mb_tiles(w, h, s, n, tile_rows=16, shard=0, n_shards=1, prm=None, tv=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    t, c = _subs(max(n, 1), tv)
    return _lib.load().rrt_launch_raymarch_mb_tiles(C.c_void_p(1), w, h, s, tile_rows, shard, n_shards, n, t, c, NO_SKY,
                                                    C.byref(rrt.CameraEffects()),
                                                    C.byref(prm if prm is not None else rrt.RenderParams()), None)


@pytest.mark.parametrize("n", [0, -1, 3, 5, 6, 7, 12, 32])
def test_sub_frame_count_outside_the_set_is_refused(n):
    assert _mb(64, 36, 1, n) == INVALID
    assert _mb_tiles(64, 36, 2, n) == INVALID


@pytest.mark.parametrize("s", [0, 3, 16])
def test_factor_outside_the_set_is_refused(s):
    assert _mb(64, 36, s, 4) == INVALID and _mb_tiles(64, 36, s, 4) == INVALID


def test_null_arrays_and_non_finite_times_are_refused():
    assert _mb(64, 36, 1, 4, times=False) == INVALID
    assert _mb(64, 36, 1, 4, cams=False) == INVALID
    for bad in (math.nan, math.inf, -math.inf):
        for k in (0, 3):
            tv = [1.0, 1.1, 1.2, 1.3]
            tv[k] = bad
            assert _mb(64, 36, 2, 4, tv=tv) == INVALID, (bad, k)
            assert _mb_tiles(64, 36, 2, 4, tv=tv) == INVALID, (bad, k)


def test_checks_of_the_supersampled_launch_are_refused():
    import relativisticraytracer_amd as rrt
    for n in (1, 4):
        assert _mb(64, 36, 2, n, out=0) == INVALID
        assert _mb(64, 36, 2, n, fx=False) == INVALID
        assert _mb(0, 36, 2, n) == INVALID and _mb(64, 0, 2, n) == INVALID
        assert _mb(8192, 8192, 8, n) == INVALID and _mb(8192, 8192, 4, n) == BAD_HANDLE      # the virtual frame's size
        assert _mb(1, 65536, 8, n) == INVALID and _mb_tiles(1, 65536, 8, n) == INVALID
        assert _mb(64, 36, 2, n, prm=rrt.RenderParams(max_steps=-1)) == INVALID
        assert _mb(64, 36, 2, n, prm=rrt.RenderParams(arith_mode=7)) == INVALID
        p40 = rrt.RenderParams()
        p40.struct_size = 40
        assert _mb(64, 36, 2, n, prm=p40) == ABI_MISMATCH and _mb_tiles(64, 36, 2, n, prm=p40) == ABI_MISMATCH
        for tr, sh, ns in ((0, 0, 1), (16, 1, 1), (16, -1, 2), (16, 0, 0)):
            assert _mb_tiles(64, 36, 2, n, tile_rows=tr, shard=sh, n_shards=ns) == INVALID, (tr, sh, ns)


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16])
def test_good_arguments_pass_the_checks(n):
    """... and reach the sky lookup, which refuses the made-up handle: no check said no"""
    import relativisticraytracer_amd as rrt
    for s in (1, 2, 8):
        assert _mb(37, 21, s, n) == BAD_HANDLE
        assert _mb_tiles(37, 21, s, n, tile_rows=5, shard=2, n_shards=3) == BAD_HANDLE
    assert _mb(37, 21, 2, n, prm=rrt.RenderParams(workspace=12345, tile_order=54321, path_policy=2, pool_rounds=3,
                                                 pass_chains=2)) == BAD_HANDLE


def _clock(k, fps, shutter, n):
    from relativisticraytracer_amd import _lib
    s, p = (C.c_float * 16)(), (C.c_float * 16)()
    return _lib.load().rrt_motion_clock(k, fps, shutter, n, s, p), np.array(s[:max(n, 0)], np.float32), np.array(p[:max(n, 0)], np.float32)


def test_motion_clock_refuses_bad_arguments():
    for k, fps, shutter, n in ((1, 24, -0.01, 4), (1, 24, 1.01, 4), (1, 24, math.nan, 4), (1, 24, 0.5, 3), (1, 24, 0.5, 0),
                               (1, 24, 0.5, 32), (-1, 24, 0.5, 4), (1, 0, 0.5, 4)):
        assert _clock(k, fps, shutter, n)[0] == INVALID, (k, fps, shutter, n)


def test_motion_clock_is_the_documented_binary32_arithmetic():
    from relativisticraytracer_amd import camera_paths as cp
    f32 = np.float32
    for k in (1, 2, 7, 24, 300, 1000):
        for fps in (24, 30, 60):
            S, P = cp.recording_clock(k, fps)
            for shutter in (0.0, 0.25, 0.5, 1.0, 0.3):
                for n in (1, 2, 4, 8, 16):
                    sim, path = cp.motion_clock(k, fps, shutter, n)
                    d = f32(shutter) * (f32(1.0) / f32(fps))
                    u = ((np.arange(n, 0, -1).astype(f32)) - f32(0.5)) / f32(n)
                    assert u.dtype == np.float32
                    want_s, want_p = f32(S) - d * u, f32(P) - d * u
                    assert np.array_equal(sim.view(np.uint32), want_s.view(np.uint32)), (k, fps, shutter, n)
                    assert np.array_equal(path.view(np.uint32), want_p.view(np.uint32)), (k, fps, shutter, n)
                    if shutter == 0.0:
                        assert np.all(sim == f32(S)) and np.all(path == f32(P))
                    elif n > 1 and k <= 300:
                        assert np.all(np.diff(sim) > 0) and np.all(np.diff(path) > 0), (k, fps, shutter, n)
                    assert np.all(sim <= f32(S)) and np.all(path <= f32(P))


def test_motion_kernel_keeps_the_vacuum_step_and_the_register_budget():
    """The blurred kernel runs the single kernel's march unchanged inside its loop over the sub-frames: its nested vacuum loop costs
    what raymarch_pixels' does per RK4 step, no v_mov, no scratch, and no registers beyond raymarch_pixels' 5-wave budget."""
    mb_strict, mb_fmad, ref = "motion_pixels<true, 2, 0>", "motion_pixels<true, 2, 2>", "raymarch_pixels<true, 2, false, 0>"
    ref_fmad = "raymarch_pixels<true, 2, false, 2>"
    got, out = _isa(mb_strict, mb_fmad, ref, ref_fmad)
    assert {mb_strict, mb_fmad, ref, ref_fmad} <= set(got), out[-2000:]
    for k, r in ((mb_strict, ref), (mb_fmad, ref_fmad)):
        assert got[k].get("unroll") == 2 and got[k]["mov"] == 0, (k, got[k])
        assert got[k]["scratch"] == 0, (k, got[k])
        assert got[k]["vgpr"] <= got[ref]["vgpr"], (k, got[k], got[ref])
        assert got[k]["occupancy"] >= 5, (k, got[k])
        assert got[k]["per_step"] == got[r]["per_step"], (k, got[k], got[r])


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("bad", rows("motion-blur", PY))
def test_python_driver_refuses_bad_blur_arguments(bad):
    refused(PY, *bad)


def test_cpp_driver_refuses_bad_blur_arguments():
    for args, msg in rows("motion-blur", CPP):
        refused(CPP, args, msg)
