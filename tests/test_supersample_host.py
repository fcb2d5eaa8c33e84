"""Supersampled frames (rrt_launch_raymarch_ss*, include/rrt.h) on a host without a GPU: the entry points are exported and bound,
every refusal happens before the library touches a device, the kernel keeps the march's vacuum step and register budget, and
both headless drivers refuse a factor outside {1, 2, 4, 8}.  The frames themselves: tests/test_gpu_supersample.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from test_driver_refusals import CPP, PY, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, BAD_HANDLE, ABI_MISMATCH = 1, 4, 6
NO_SKY = 0x7777000000000001          # never a registered sky: a launch that passes every check stops at the handle lookup


def test_symbols_are_exported_and_bound():
    from relativisticraytracer_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in ("rrt_launch_raymarch_ss", "rrt_launch_raymarch_ss_tiles"):
        assert name in bound and hasattr(lib, name), name


def _args():
    import relativisticraytracer_amd as rrt
    return rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams()


def _ss(w, h, s, out=1, cam=True, fx=True, prm=None):
    from relativisticraytracer_amd import _lib
    c, f, p = _args()
    return _lib.load().rrt_launch_raymarch_ss(C.c_void_p(out) if out else None, None, w, h, s, 1.0, C.byref(c) if cam else None,
                                              NO_SKY, C.byref(f) if fx else None, C.byref(prm if prm is not None else p), None)


def _ss_tiles(w, h, s, tile_rows=16, shard=0, n_shards=1, prm=None):
    from relativisticraytracer_amd import _lib
    c, f, p = _args()
    return _lib.load().rrt_launch_raymarch_ss_tiles(C.c_void_p(1), w, h, s, tile_rows, shard, n_shards, 1.0, C.byref(c), NO_SKY,
                                                    C.byref(f), C.byref(prm if prm is not None else p), None)


@pytest.mark.parametrize("s", [0, -1, 3, 5, 6, 7, 16])
def test_factor_outside_the_set_is_refused(s):
    assert _ss(64, 36, s) == INVALID
    assert _ss_tiles(64, 36, s) == INVALID


def test_virtual_frame_limits_are_refused():
    # (s w)(s h) >= 2^31 while w h itself is fine
    assert _ss(8192, 8192, 8) == INVALID and _ss(8192, 8192, 4) == BAD_HANDLE
    assert _ss(32768, 16384, 2) == INVALID and _ss(32768, 16383, 2) == BAD_HANDLE      # 2^31 exactly / just under
    # s h > 524 280 virtual rows
    assert _ss(1, 65536, 8) == INVALID and _ss(1, 65535, 8) == BAD_HANDLE
    assert _ss(1, 262141, 2) == INVALID and _ss(1, 262140, 2) == BAD_HANDLE
    assert _ss_tiles(1, 65536, 8) == INVALID and _ss_tiles(1, 65535, 8) == BAD_HANDLE


def test_common_checks_are_refused():
    import relativisticraytracer_amd as rrt
    for s in (1, 2):
        assert _ss(64, 36, s, out=0) == INVALID
        assert _ss(64, 36, s, cam=False) == INVALID
        assert _ss(64, 36, s, fx=False) == INVALID
        assert _ss(0, 36, s) == INVALID and _ss(64, 0, s) == INVALID and _ss(-3, 36, s) == INVALID
        assert _ss(65536, 32768, s) == INVALID                   # w h >= 2^31
        assert _ss(1, 524281, s) == INVALID                      # h > 524 280
        assert _ss(64, 36, s, prm=rrt.RenderParams(max_steps=-1)) == INVALID
        assert _ss(64, 36, s, prm=rrt.RenderParams(arith_mode=7)) == INVALID
        assert _ss(64, 36, s, prm=rrt.RenderParams(nudge_ulps=-1)) == INVALID
        p40 = rrt.RenderParams()
        p40.struct_size = 40                                      # built against another header
        assert _ss(64, 36, s, prm=p40) == ABI_MISMATCH
        assert _ss_tiles(64, 36, s, prm=p40) == ABI_MISMATCH
        for tr, sh, n in ((0, 0, 1), (16, 1, 1), (16, -1, 2), (16, 0, 0)):
            assert _ss_tiles(64, 36, s, tile_rows=tr, shard=sh, n_shards=n) == INVALID, (tr, sh, n)


@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_good_arguments_pass_the_checks(s):
    """... and reach the sky lookup, which refuses the made-up handle: no check said no."""
    import relativisticraytracer_amd as rrt
    assert _ss(37, 21, s) == BAD_HANDLE
    assert _ss_tiles(37, 21, s, tile_rows=5, shard=2, n_shards=3) == BAD_HANDLE
    # the ignored params are ignored, not validated as objects: made-up workspace / tile-order ids pass the checks too
    assert _ss(37, 21, s, prm=rrt.RenderParams(workspace=12345, tile_order=54321, path_policy=2, pool_rounds=3, pass_chains=2)) == BAD_HANDLE


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


def test_supersample_kernel_keeps_the_vacuum_step_and_the_register_budget():
    """The supersampled kernel runs the single kernel's march unchanged: its nested vacuum loop costs what raymarch_pixels' does per
    RK4 step (tests/test_tools.py's marks: <= 225 VALU FMAD, <= 283 strict, no v_mov on the straight path), and the reduction after
    the march costs no registers beyond raymarch_pixels' 5-wave budget and no scratch."""
    ss_strict, ss_fmad, ref = "supersample_pixels<true, 2, 0>", "supersample_pixels<true, 2, 2>", "raymarch_pixels<true, 2, false, 0>"
    got, out = _isa(ss_strict, ss_fmad, ref)
    assert {ss_strict, ss_fmad, ref} <= set(got), out[-2000:]
    for k in (ss_strict, ss_fmad):
        assert got[k].get("unroll") == 2 and got[k]["mov"] == 0, (k, got[k])
        assert got[k]["scratch"] == 0, (k, got[k])
        assert got[k]["vgpr"] <= got[ref]["vgpr"], (k, got[k], got[ref])
        assert got[k]["occupancy"] >= 5, (k, got[k])
    assert got[ss_strict]["per_step"] <= 283.0 and got[ss_fmad]["per_step"] <= 225.0, got
    assert got[ss_strict]["per_step"] == got[ref]["per_step"], got


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
def test_python_driver_refuses_other_factors():
    for args, msg in rows("supersample", PY):
        refused(PY, args, msg)


def test_cpp_driver_refuses_other_factors():
    for args, msg in rows("supersample", CPP):
        refused(CPP, args, msg)
