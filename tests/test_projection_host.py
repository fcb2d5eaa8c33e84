"""Panoramas (rrt_projection, rrt_launch_raymarch_pano*, include/rrt.h) on a host without a GPU: the entry points are exported and
bound, the defaults and the struct are as documented, every refusal happens before the library touches a device, the host query
rrt_projection_ray equals the numpy restatement (tests/projection_ref.py) bit for bit on every pixel, the kernel keeps the march's
vacuum step and register budget, and both headless drivers refuse bad spans and the combinations the kernels lack.  The frames
themselves: tests/test_gpu_projection.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import projection_ref as pr
from test_driver_refusals import CPP, IDS, PY, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, BAD_HANDLE, ABI_MISMATCH = 1, 4, 6
NO_SKY = 0x7777000000000001          # never a registered sky: a launch that passes every check stops at the handle lookup
PUBLIC = ("rrt_projection_default", "rrt_projection_ray", "rrt_launch_projection_map", "rrt_launch_raymarch_pano",
          "rrt_launch_raymarch_pano_tiles")

# (kind, fov, vfov, W, H): the frames every direction test covers
FRAMES = [(pr.EQUIRECT, 360.0, 180.0, 64, 32), (pr.EQUIRECT, 180.0, 90.0, 64, 32), (pr.EQUIRECT, 360.0, 180.0, 37, 19),
          (pr.FISHEYE, 180.0, 0.0, 48, 48), (pr.FISHEYE, 220.0, 0.0, 48, 48), (pr.FISHEYE, 180.0, 0.0, 33, 27),
          (pr.PINHOLE, 0.0, 0.0, 40, 23)]


def cameras():
    """the reference's start-up camera, a yawed and pitched one, and path 0 part-way through"""
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import camera_paths as cp
    return [rrt.CameraState.default(), rrt.CameraState.from_angles((12.0, -3.0, 40.0), 137.0, 21.5),
            cp.CameraPath(0).camera_at(3.7)]


def test_symbols_are_exported_and_bound():
    from relativisticraytracer_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in PUBLIC:
        assert name in bound and hasattr(lib, name), name


def test_struct_layout_and_defaults():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    P = _lib.rrt_projection
    assert C.sizeof(P) == 16 and [P.kind.offset, P.fov_deg.offset, P.vfov_deg.offset] == [4, 8, 12]
    lib = _lib.load()
    want = {0: (0.0, 0.0), 1: (360.0, 180.0), 2: (180.0, 0.0)}
    for kind, (fov, vfov) in want.items():
        p = P()
        assert lib.rrt_projection_default(kind, C.byref(p)) == 0
        assert (p.struct_size, p.kind, p.fov_deg, p.vfov_deg) == (16, kind, fov, vfov), kind
    assert rrt.PROJ_PINHOLE == 0 and rrt.PROJ_EQUIRECT == 1 and rrt.PROJ_FISHEYE == 2
    assert rrt.projection_default("fisheye").info() == {"kind": "fisheye", "fov_deg": 180.0, "vfov_deg": 0.0}
    assert rrt.Projection("equirect", 180, 90).info() == {"kind": "equirect", "fov_deg": 180.0, "vfov_deg": 90.0}
    for bad in (-1, 3, 99):
        assert lib.rrt_projection_default(bad, C.byref(P())) == INVALID
    assert lib.rrt_projection_default(1, None) == INVALID
    with pytest.raises(ValueError):
        rrt.Projection("cubemap")


def _proj(kind=1, fov=None, vfov=None, size=None):
    from relativisticraytracer_amd import _lib
    p = _lib.rrt_projection()
    assert _lib.load().rrt_projection_default(kind, C.byref(p)) == 0
    if fov is not None:
        p.fov_deg = fov
    if vfov is not None:
        p.vfov_deg = vfov
    if size is not None:
        p.struct_size = size
    return p


def _pano(w, h, s, proj, out=1, cam=True, fx=True, prm=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    c, f, p = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams()
    return _lib.load().rrt_launch_raymarch_pano(C.c_void_p(out) if out else None, None, w, h, s,
                                                C.byref(proj) if proj is not None else None, 1.0, C.byref(c) if cam else None,
                                                NO_SKY, C.byref(f) if fx else None, C.byref(prm if prm is not None else p), None)


def _pano_tiles(w, h, s, proj, tile_rows=16, shard=0, n_shards=1, prm=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    c, f, p = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams()
    return _lib.load().rrt_launch_raymarch_pano_tiles(C.c_void_p(1), w, h, s, tile_rows, shard, n_shards,
                                                      C.byref(proj) if proj is not None else None, 1.0, C.byref(c), NO_SKY,
                                                      C.byref(f), C.byref(prm if prm is not None else p), None)


def _ray(proj, w=8, h=4, x=0, y=0):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    d, inside = (C.c_float * 3)(), C.c_int(0)
    return _lib.load().rrt_projection_ray(C.byref(proj) if proj is not None else None, w, h, x, y,
                                          C.byref(rrt.CameraState.default()), C.byref(d), C.byref(inside))


BAD_SPANS = [(1, 0.0, 180.0), (1, -10.0, 180.0), (1, 360.5, 180.0), (1, float("nan"), 180.0), (1, float("inf"), 180.0),
             (1, 360.0, 0.0), (1, 360.0, 180.01), (1, 360.0, -90.0), (1, 360.0, float("nan")), (1, 360.0, float("-inf")),
             (2, 0.0, None), (2, 361.0, None), (2, float("nan"), None), (2, -180.0, None)]


@pytest.mark.parametrize("kind,fov,vfov", BAD_SPANS)
def test_bad_spans_are_refused(kind, fov, vfov):
    p = _proj(kind, fov, vfov)
    assert _pano(64, 32, 1, p) == INVALID
    assert _pano_tiles(64, 32, 2, p) == INVALID
    assert _ray(p) == INVALID


def _map(proj, w=8, h=4, out=16, cam=True):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    return _lib.load().rrt_launch_projection_map(C.c_void_p(out) if out else None, w, h, C.byref(proj) if proj is not None else None,
                                                 C.byref(rrt.CameraState.default()) if cam else None, None)


def test_projection_map_refusals():
    """rrt_launch_projection_map refuses before any device call (a GPU-free host has none to make: every accepted call would fail
    in the launch, so only refusals are checked here)"""
    assert _map(None) == INVALID and _map(_proj(1, size=12)) == ABI_MISMATCH and _map(_proj(1, 400.0)) == INVALID
    assert _map(_proj(2, float("nan"))) == INVALID
    assert _map(_proj(1), out=0) == INVALID and _map(_proj(1), out=8) == INVALID and _map(_proj(1), cam=False) == INVALID
    assert _map(_proj(1), w=0) == INVALID and _map(_proj(1), h=-1) == INVALID and _map(_proj(1), 65536, 32768) == INVALID


def test_projection_refusals():
    p = _proj(1)
    assert _pano(64, 32, 1, None) == INVALID and _pano_tiles(64, 32, 1, None) == INVALID and _ray(None) == INVALID
    for kind in (-1, 3, 7):
        q = _proj(1)
        q.kind = kind
        assert _pano(64, 32, 1, q) == INVALID and _pano_tiles(64, 32, 1, q) == INVALID and _ray(q) == INVALID
    for size in (0, 12, 20):
        q = _proj(1, size=size)
        assert _pano(64, 32, 1, q) == ABI_MISMATCH and _pano_tiles(64, 32, 1, q) == ABI_MISMATCH and _ray(q) == ABI_MISMATCH
    # the host query's own: the frame and the pixel
    for w, h, x, y in ((0, 4, 0, 0), (8, 0, 0, 0), (8, 4, 8, 0), (8, 4, 0, 4), (8, 4, -1, 0), (8, 4, 0, -1)):
        assert _ray(p, w, h, x, y) == INVALID, (w, h, x, y)
    from relativisticraytracer_amd import _lib
    d = (C.c_float * 3)()
    assert _lib.load().rrt_projection_ray(C.byref(p), 8, 4, 0, 0, None, C.byref(d), None) == INVALID
    import relativisticraytracer_amd as rrt
    assert _lib.load().rrt_projection_ray(C.byref(p), 8, 4, 0, 0, C.byref(rrt.CameraState.default()), None, None) == INVALID
    assert _lib.load().rrt_projection_ray(C.byref(p), 8, 4, 0, 0, C.byref(rrt.CameraState.default()), C.byref(d), None) == 0


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_everything_ss_refuses_is_refused(kind):
    import relativisticraytracer_amd as rrt
    p = _proj(kind)
    for s in (0, 3, 16):
        assert _pano(64, 32, s, p) == INVALID and _pano_tiles(64, 32, s, p) == INVALID
    assert _pano(64, 32, 1, p, out=0) == INVALID
    assert _pano(64, 32, 1, p, cam=False) == INVALID
    assert _pano(64, 32, 1, p, fx=False) == INVALID
    assert _pano(0, 32, 1, p) == INVALID and _pano(64, 0, 1, p) == INVALID
    assert _pano(65536, 32768, 1, p) == INVALID                           # w h >= 2^31
    assert _pano(8192, 8192, 8, p) == INVALID and _pano(1, 65536, 8, p) == INVALID      # the virtual frame's limits
    assert _pano(64, 32, 1, p, prm=rrt.RenderParams(arith_mode=7)) == INVALID
    assert _pano(64, 32, 1, p, prm=rrt.RenderParams(nudge_ulps=-1)) == INVALID
    p40 = rrt.RenderParams()
    p40.struct_size = 40
    assert _pano(64, 32, 1, p, prm=p40) == ABI_MISMATCH
    for tr, sh, n in ((0, 0, 1), (16, 1, 1), (16, -1, 2), (16, 0, 0)):
        assert _pano_tiles(64, 32, 2, p, tile_rows=tr, shard=sh, n_shards=n) == INVALID, (tr, sh, n)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_good_arguments_pass_the_checks(kind, s):
    """... and reach the sky lookup, which refuses the made-up handle: no check said no"""
    import relativisticraytracer_amd as rrt
    for p in (_proj(kind), _proj(kind, 90.0, 45.0) if kind == 1 else _proj(kind, 360.0)):
        assert _pano(37, 21, s, p) == BAD_HANDLE
        assert _pano_tiles(37, 21, s, p, tile_rows=5, shard=2, n_shards=3) == BAD_HANDLE
        assert _pano(37, 21, s, p, prm=rrt.RenderParams(workspace=12345, tile_order=54321, path_policy=2, pool_rounds=3,
                                                        pass_chains=2)) == BAD_HANDLE
    if kind == 2:
        assert _pano(37, 21, s, _proj(2, 180.0, float("nan"))) == BAD_HANDLE       # a fisheye's vfov is not looked at
    if kind == 0:
        assert _pano(37, 21, s, _proj(0, float("nan"), -1.0)) == BAD_HANDLE        # nor a pinhole's spans


def host_directions(kind, fov, vfov, W, H, cam):
    import relativisticraytracer_amd as rrt
    p = _proj(kind, fov, vfov)
    d = np.zeros((H, W, 3), np.float32)
    inside = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            d[y, x], inside[y, x] = rrt.projection_ray(p, W, H, x, y, cam)
    return d, inside


@pytest.mark.parametrize("frame", FRAMES, ids=lambda f: "%s_%gx%g_%dx%d" % ((("pinhole", "equirect", "fisheye")[f[0]],) + tuple(f[1:])))
def test_host_query_equals_the_restatement_bit_for_bit(po, frame):
    kind, fov, vfov, W, H = frame
    for cam in cameras():
        got, inside = host_directions(kind, fov, vfov, W, H, cam)
        want, want_in = pr.directions(po, kind, fov, vfov, W, H, cam.as_array())
        assert np.array_equal(inside, want_in), frame
        bad = got.view(np.uint32) != want.view(np.uint32)
        assert not bad.any(), (frame, int(bad.any(-1).sum()), np.argwhere(bad.any(-1))[:5].tolist())
        n = np.linalg.norm(got[inside].astype(np.float64), axis=-1)
        assert np.all(np.abs(n - 1.0) < 1e-6), frame                      # unit directions


def test_fisheye_disc_split_and_geometry(po):
    """outside <=> r2 > 1 (a zero direction); the disc's centre looks along forward, its rim at half the aperture"""
    import relativisticraytracer_amd as rrt
    cam = rrt.CameraState.default()
    fw = cam.as_array()[1]
    for W, H in ((48, 48), (33, 27), (64, 32)):
        got, inside = host_directions(pr.FISHEYE, 180.0, 0.0, W, H, cam)
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        u = (np.float32(2) * (x.astype(np.float32) + np.float32(0.5)) - np.float32(W)) / np.float32(H)
        v = (np.float32(2) * (y.astype(np.float32) + np.float32(0.5)) - np.float32(H)) / np.float32(H)
        assert np.array_equal(~inside, u * u + v * v > np.float32(1.0)), (W, H)
        assert not got[~inside].any() and 0 < (~inside).sum() < W * H
        angle = np.degrees(np.arccos(np.clip(got[inside] @ fw, -1, 1)))
        r = np.sqrt((u * u + v * v)[inside].astype(np.float64))
        assert np.allclose(angle, 90.0 * r, atol=1e-3), (W, H)            # equidistant: angle = r * aperture / 2
    got, _ = host_directions(pr.EQUIRECT, 360.0, 180.0, 64, 32, cam)
    # the centre column looks along forward at the horizon row, +x turns toward right, +y toward up
    a = cam.as_array()
    mid = (got[15, 31] + got[16, 32]) / 2
    assert mid @ a[1] > 0.99 and got[16, 48] @ a[2] > 0.99 and got[31, 32] @ a[3] > 0.99


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


def test_panorama_kernel_keeps_the_vacuum_step_and_the_register_budget():
    """The panorama kernel runs the single kernel's march unchanged: its nested vacuum loop costs what raymarch_pixels' does per RK4
    step (<= 283 VALU strict, <= 225 FMAD, no v_mov on the straight path), and the projection before the march and the branch around
    it for outside lanes cost no registers beyond raymarch_pixels' 5-wave budget and no scratch."""
    strict, fmad = "panorama_pixels<true, 2, 0>", "panorama_pixels<true, 2, 2>"
    ref_strict, ref_fmad = "raymarch_pixels<true, 2, false, 0>", "raymarch_pixels<true, 2, false, 2>"
    got, out = _isa(strict, fmad, ref_strict, ref_fmad)
    assert {strict, fmad, ref_strict, ref_fmad} <= set(got), out[-2000:]
    for k in (strict, fmad):
        assert got[k].get("unroll") == 2 and got[k]["mov"] == 0, (k, got[k])
        assert got[k]["scratch"] == 0, (k, got[k])
        assert got[k]["vgpr"] <= got[ref_strict]["vgpr"], (k, got[k], got[ref_strict])
        assert got[k]["occupancy"] >= 5, (k, got[k])
    assert got[strict]["per_step"] <= 283.0 and got[fmad]["per_step"] <= 225.0, got
    assert got[strict]["per_step"] == got[ref_strict]["per_step"], got
    assert got[fmad]["per_step"] == got[ref_fmad]["per_step"], got


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("args,msg", rows("projection", PY), **IDS)
def test_python_driver_refuses(args, msg):
    refused(PY, args, msg)


def test_python_driver_refuses_other_projections():
    for args, msg in rows("projection-kind", PY):
        refused(PY, args, msg)


@pytest.mark.parametrize("args,msg", rows("projection", CPP), **IDS)
def test_cpp_driver_refuses(args, msg):
    refused(CPP, args, msg)
