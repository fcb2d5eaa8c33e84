"""Depth of field (rrt_launch_raymarch_dof*, rrt_lens_ray, rrt_lens_points, include/rrt.h) on a host without a GPU: the entry
points are exported, declared and bound, the host query rrt_lens_ray equals the numpy restatement (tests/lens_ref.py) bit for bit,
with ly = 0 it is rrt_stereo_ray's eye, in flat space all lens points' rays through a pixel meet on the plane in focus,
rrt_lens_points is the documented spiral, every refusal happens before the library touches a device, lens_ray and lens_points are
clean under ASan and UBSan (tests/lens/lens_exerciser.cpp, a program of its own), and both headless drivers refuse what the
kernel lacks.  The frames themselves: tests/test_gpu_dof.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lens_ref as lr
import projection_ref as pr
from test_projection_host import cameras
from test_driver_refusals import CPP, IDS, PY, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, BAD_HANDLE, ABI_MISMATCH = 1, 4, 6
NO_SKY = 0x7777000000000001          # never a registered sky: a launch that passes every check stops at the handle lookup
PUBLIC = ("rrt_launch_raymarch_dof", "rrt_launch_raymarch_dof_tiles", "rrt_lens_ray", "rrt_lens_points")
F = np.float32
NAN, INF = float("nan"), float("inf")


def test_symbols_are_exported_declared_and_bound():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "rrt.h")).read()
    for name in PUBLIC:
        assert name in bound and hasattr(lib, name), name
        assert re.search(r"^int %s\(" % name, header, re.M), name
    for name in ("launch_raymarch_dof", "launch_raymarch_dof_tiles", "lens_ray", "lens_points"):
        assert name in rrt.__all__ and hasattr(rrt, name), name
    assert re.search(r"#define RRT_ABI_VERSION 5\b", header) and rrt.abi_version() == 5      # additive exports
    compat = open(os.path.join(ROOT, "include", "raymarcher.h")).read()
    assert "inline int launch_raymarch_dof(" in compat and "inline int launch_raymarch_dof_tiles(" in compat


def host_rays(W, H, cam, lx, ly, focus):
    import relativisticraytracer_amd as rrt
    o, d = np.zeros((H, W, 3), F), np.zeros((H, W, 3), F)
    for y in range(H):
        for x in range(W):
            o[y, x], d[y, x] = rrt.lens_ray(W, H, x, y, cam, lx, ly, focus)
    return o, d


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def signed_zero_camera():
    import relativisticraytracer_amd as rrt
    return rrt.CameraState((-0.0, 0.0, -0.0), *rrt.CameraState.default().as_array()[1:])


def test_host_query_equals_the_restatement_bit_for_bit():
    """whole frames at fixed lens points that cover the zero rules (a zero of either sign on either axis, a quotient that
    underflows to zero) and a signed-zero position, then random cameras, sizes, pixels, lens points and focus"""
    import relativisticraytracer_amd as rrt
    fixed = [(0.0, 0.0, 12.0), (-0.0, -0.0, 3.0), (0.5, 0.0, 12.0), (-0.5, -0.0, 12.0), (0.0, 0.3, 7.0), (-0.0, -0.3, 7.0),
             (0.37, -0.21, 9.5), (1e-42, -1e-42, 1e6), (2.5, 1.75, 0.4)]
    for cam in cameras() + [signed_zero_camera()]:
        for W, H in ((13, 7), (8, 11)):
            for lx, ly, z in fixed:
                got_o, got_d = host_rays(W, H, cam, lx, ly, z)
                want_o, want_d = lr.rays(W, H, cam.as_array(), lx, ly, z)
                assert np.array_equal(_bits(got_d), _bits(want_d)), (W, H, lx, ly, z)
                assert np.array_equal(_bits(got_o), _bits(np.broadcast_to(want_o, got_o.shape))), (W, H, lx, ly, z)
                if lx == 0 and ly == 0:                     # the zero rule: pos untouched, a signed zero included
                    assert np.array_equal(_bits(got_o[0, 0]), _bits(cam.as_array()[0]))
    assert F(1e-42) / F(1e6) == 0 and F(1e-42) != 0        # that case's shift is zero although its lens point is not
    rng = np.random.default_rng(20261018)
    for _ in range(400):
        cam = rrt.CameraState.from_angles(rng.uniform(-50, 50, 3), rng.uniform(-180, 180), rng.uniform(-80, 80))
        W, H = int(rng.integers(1, 200)), int(rng.integers(1, 200))
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        lx, ly = (F(v) for v in rng.normal(0, 0.5, 2) * rng.choice([0.0, 1.0, 1.0, 1.0], 2))
        z = F(10 ** rng.uniform(-1, 2))
        o, d = rrt.lens_ray(W, H, x, y, cam, lx, ly, z)
        want_o, want_D = lr.ray(W, H, cam.as_array(), lx, ly, z, x, y)
        assert np.array_equal(_bits(o), _bits(want_o)) and np.array_equal(_bits(d), _bits(pr.normalize(want_D))), (W, H, x, y, lx, ly, z)


def test_a_horizontal_lens_point_is_the_stereo_eye():
    """ly = 0: rrt_lens_ray(lx, 0, Z) == rrt_stereo_ray of the right (lx > 0) or left (lx < 0) eye of the pinhole pair with base
    2 |lx| (exact) and convergence Z, bit for bit, every pixel"""
    import relativisticraytracer_amd as rrt
    p = rrt.Projection("pinhole")
    for cam in cameras() + [signed_zero_camera()]:
        for lx, z, W, H in ((0.5, 12.0, 17, 9), (0.325, 14.0, 9, 13), (1.5, 0.3, 12, 12), (0.0, 5.0, 6, 5)):
            st = rrt.Stereo("side-by-side", 2.0 * lx, z)
            assert F(0.5 * float(F(2.0 * lx))) == F(lx)
            for eye, e in ((0, -1.0), (1, 1.0)):
                got_o, got_d = host_rays(W, H, cam, e * lx, 0.0 if eye else -0.0, z)
                for y in range(H):
                    for x in range(W):
                        o, d, _ = rrt.stereo_ray(p, st, W, H, eye, x, y, cam)
                        assert np.array_equal(_bits(o), _bits(got_o[y, x])) and np.array_equal(_bits(d), _bits(got_d[y, x])), (lx, z, eye, x, y)


def test_all_lens_points_meet_on_the_plane_in_focus():
    """flat-space geometry in double: the ray of every lens point through pixel (x, y) crosses the plane `focus` along forward
    where the pixel's centre ray (lens point (0, 0)) does.  Bound: the point is org + D t with t = focus / (D . fw) and D's
    coordinates rounded to float: the binary32 roundings of u - cx, of the products and sums in D and in org (a handful, each half
    an ulp of a term no larger than the coordinates involved: |pos| + aperture at the lens, focus (1 + |u| + |v|) on the plane)
    -- 16 ulps of that magnitude covers them with room to spare and is still 1e-6 of the scene."""
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(7)
    eps = float(np.finfo(F).eps)
    for cam in cameras():
        pos, fw, rt, up = (v.astype(np.float64) for v in cam.as_array())
        for W, H, z in ((40, 23, 12.0), (64, 36, 55.0), (31, 31, 2.5)):
            pts = lr.points(0.8, 16, 0.4)
            for _ in range(12):
                x, y = int(rng.integers(0, W)), int(rng.integers(0, H))

                def hit(lx, ly):
                    o, d = rrt.lens_ray(W, H, x, y, cam, lx, ly, z)
                    o, d = o.astype(np.float64), d.astype(np.float64)
                    return o + d * ((z - (o - pos) @ fw) / (d @ fw))
                centre = hit(0.0, 0.0)
                scale = np.abs(pos).max() + 0.8 + np.abs(centre - pos).max()
                for lx, ly in pts:
                    err = np.abs(hit(lx, ly) - centre).max()
                    assert err <= 16 * eps * scale, (W, H, z, x, y, lx, ly, err, scale)
    # and the spread a quarter of the way to the plane is three quarters of the lens: the blur is real
    cam = cameras()[0]
    pos, fw = (v.astype(np.float64) for v in cam.as_array()[:2])
    at = []
    for lx, ly in ((0.8, 0.0), (-0.8, 0.0)):
        o, d = (v.astype(np.float64) for v in rrt.lens_ray(40, 23, 20, 11, cam, lx, ly, 12.0))
        at.append(o + d * ((3.0 - (o - pos) @ fw) / (d @ fw)))
    assert abs(np.linalg.norm(at[0] - at[1]) - 1.6 * 0.75) < 1e-3


def test_lens_points_are_the_documented_spiral():
    import relativisticraytracer_amd as rrt
    for n in (1, 2, 4, 8, 16):
        for aperture, rot in ((0.3, 0.0), (1.0, 0.4), (0.0, 2.0), (12.5, -3.0)):
            got = rrt.lens_points(aperture, n, rot)
            want = lr.points(aperture, n, rot)
            assert got.shape == (n, 2) and got.dtype == np.float32
            # to 1 ulp of float: libm and numpy may round the double sine and cosine differently
            assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))), (n, aperture, rot)
            assert np.all(np.hypot(*got.astype(np.float64).T) <= float(F(aperture))), (n, aperture, rot)
            if n == 1:
                assert np.array_equal(_bits(got), np.zeros((1, 2), np.uint32))
            elif aperture > 0:
                r = np.hypot(*got.astype(np.float64).T)
                assert np.all(np.diff(r) > 0)                                       # equal-area rings, the last one at the rim
                assert np.allclose(r, aperture * np.sqrt((np.arange(n) + 0.5) / n), rtol=1e-6)
    assert np.array_equal(rrt.lens_points(0.3, 8), rrt.lens_points(0.3, 8, 0.0))


def test_lens_points_refusals():
    from relativisticraytracer_amd import _lib
    lib, xy = _lib.load(), (C.c_float * 32)()
    for n in (0, -1, 3, 5, 6, 12, 32):
        assert lib.rrt_lens_points(0.3, n, 0.0, xy) == INVALID, n
    for a, rot in ((-0.1, 0.0), (NAN, 0.0), (INF, 0.0), (-INF, 0.0), (0.3, NAN), (0.3, INF)):
        assert lib.rrt_lens_points(a, 4, rot, xy) == INVALID, (a, rot)
    assert lib.rrt_lens_points(0.3, 4, 0.0, None) == INVALID
    assert lib.rrt_lens_points(0.3, 4, 0.0, xy) == 0 and lib.rrt_lens_points(0.0, 16, 0.0, xy) == 0


def test_lens_ray_refusals():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    lib, cam, v = _lib.load(), rrt.CameraState.default(), (C.c_float * 3)()

    def q(w=8, h=4, x=0, y=0, lx=0.1, ly=0.1, z=5.0, c=True, o=True, d=True):
        return lib.rrt_lens_ray(w, h, x, y, C.byref(cam) if c else None, lx, ly, z, C.byref(v) if o else None, C.byref(v) if d else None)
    assert q() == 0 and q(x=7, y=3) == 0 and q(lx=0.0, ly=-0.0) == 0
    for bad in (dict(w=0), dict(h=0), dict(x=8), dict(y=4), dict(x=-1), dict(y=-1), dict(c=False), dict(o=False), dict(d=False),
                dict(lx=NAN), dict(lx=INF), dict(ly=NAN), dict(ly=-INF), dict(z=0.0), dict(z=-0.0), dict(z=-3.0), dict(z=NAN),
                dict(z=INF)):
        assert q(**bad) == INVALID, bad


def _samples(n, tv=None, lens=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    t = tv if tv is not None else [1.0 + 0.01 * k for k in range(n)]
    xy = lens if lens is not None else [0.05 * k for k in range(2 * n)]
    return ((C.c_float * len(t))(*t), (_lib.rrt_camera * len(t))(*[rrt.CameraState.default() for _ in t]), (C.c_float * len(xy))(*xy))


def _dof(w, h, s, n, out=1, times=True, cams=True, lens=True, focus=12.0, fx=True, prm=None, tv=None, xy=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    t, c, l = _samples(max(n, 1), tv, xy)
    return _lib.load().rrt_launch_raymarch_dof(C.c_void_p(out) if out else None, None, w, h, s, n, t if times else None,
                                               c if cams else None, l if lens else None, focus, NO_SKY,
                                               C.byref(rrt.CameraEffects()) if fx else None,
                                               C.byref(prm if prm is not None else rrt.RenderParams()), None)


def _dof_tiles(w, h, s, n, tile_rows=16, shard=0, n_shards=1, lens=True, focus=12.0, prm=None, tv=None, xy=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    t, c, l = _samples(max(n, 1), tv, xy)
    return _lib.load().rrt_launch_raymarch_dof_tiles(C.c_void_p(1), w, h, s, tile_rows, shard, n_shards, n, t, c, l if lens else None,
                                                     focus, NO_SKY, C.byref(rrt.CameraEffects()),
                                                     C.byref(prm if prm is not None else rrt.RenderParams()), None)


@pytest.mark.parametrize("n", [0, -1, 3, 5, 6, 7, 12, 32])
def test_sample_count_outside_the_set_is_refused(n):
    assert _dof(64, 36, 1, n) == INVALID and _dof_tiles(64, 36, 2, n) == INVALID


def test_the_lens_own_refusals():
    """a NULL lens_xy, a non-finite lens coordinate at any position, a focus that is not finite or <= 0"""
    assert _dof(64, 36, 1, 4, lens=False) == INVALID and _dof_tiles(64, 36, 1, 4, lens=False) == INVALID
    for bad in (NAN, INF, -INF):
        for k in (0, 1, 6, 7):
            xy = [0.1] * 8
            xy[k] = bad
            assert _dof(64, 36, 2, 4, xy=xy) == INVALID and _dof_tiles(64, 36, 2, 4, xy=xy) == INVALID, (bad, k)
    for z in (0.0, -0.0, -1.0, NAN, INF, -INF):
        assert _dof(64, 36, 2, 4, focus=z) == INVALID and _dof_tiles(64, 36, 2, 4, focus=z) == INVALID, z
        assert _dof(64, 36, 1, 1, focus=z, xy=[0.0, 0.0]) == INVALID, z        # even where no lens point needs it


def test_everything_the_blurred_launch_refuses_is_refused():
    import relativisticraytracer_amd as rrt
    for s in (0, 3, 16):
        assert _dof(64, 36, s, 4) == INVALID and _dof_tiles(64, 36, s, 4) == INVALID
    assert _dof(64, 36, 1, 4, times=False) == INVALID and _dof(64, 36, 1, 4, cams=False) == INVALID
    for bad in (NAN, INF, -INF):
        for k in (0, 3):
            tv = [1.0, 1.1, 1.2, 1.3]
            tv[k] = bad
            assert _dof(64, 36, 2, 4, tv=tv) == INVALID and _dof_tiles(64, 36, 2, 4, tv=tv) == INVALID, (bad, k)
    for n in (1, 4):
        assert _dof(64, 36, 2, n, out=0) == INVALID
        assert _dof(64, 36, 2, n, fx=False) == INVALID
        assert _dof(0, 36, 2, n) == INVALID and _dof(64, 0, 2, n) == INVALID
        assert _dof(8192, 8192, 8, n) == INVALID and _dof(8192, 8192, 4, n) == BAD_HANDLE        # the virtual frame's size
        assert _dof(1, 65536, 8, n) == INVALID and _dof_tiles(1, 65536, 8, n) == INVALID
        assert _dof(64, 36, 2, n, prm=rrt.RenderParams(max_steps=-1)) == INVALID
        assert _dof(64, 36, 2, n, prm=rrt.RenderParams(arith_mode=7)) == INVALID
        p40 = rrt.RenderParams()
        p40.struct_size = 40
        assert _dof(64, 36, 2, n, prm=p40) == ABI_MISMATCH and _dof_tiles(64, 36, 2, n, prm=p40) == ABI_MISMATCH
        for tr, sh, ns in ((0, 0, 1), (16, 1, 1), (16, -1, 2), (16, 0, 0)):
            assert _dof_tiles(64, 36, 2, n, tile_rows=tr, shard=sh, n_shards=ns) == INVALID, (tr, sh, ns)


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16])
def test_good_arguments_pass_the_checks(n):
    """... and reach the sky lookup, which refuses the made-up handle: no check said no"""
    import relativisticraytracer_amd as rrt
    for s in (1, 2, 8):
        assert _dof(37, 21, s, n) == BAD_HANDLE
        assert _dof_tiles(37, 21, s, n, tile_rows=5, shard=2, n_shards=3) == BAD_HANDLE
    assert _dof(37, 21, 2, n, focus=1e-30, xy=[-0.0] * (2 * n)) == BAD_HANDLE
    assert _dof(37, 21, 2, n, prm=rrt.RenderParams(workspace=12345, tile_order=54321, path_policy=2, pool_rounds=3,
                                                  pass_chains=2)) == BAD_HANDLE


def test_python_wrapper_counts_its_arrays():
    import relativisticraytracer_amd as rrt
    cam, fx = rrt.CameraState.default(), rrt.CameraEffects()
    with pytest.raises(ValueError):
        rrt.launch_raymarch_dof(1, 8, 8, 1, [1.0, 1.0], [cam, cam], [(0.0, 0.0)], 5.0, NO_SKY, fx)
    with pytest.raises(ValueError):
        rrt.launch_raymarch_dof_tiles(1, 8, 8, 1, 16, 0, 1, [1.0], [cam, cam], [(0.0, 0.0)], 5.0, NO_SKY, fx)
    with pytest.raises(rrt.RRTError):
        rrt.lens_points(-1.0, 4)
    with pytest.raises(rrt.RRTError):
        rrt.lens_ray(8, 8, 0, 0, cam, 0.1, 0.1, 0.0)


@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    """tests/lens/lens_exerciser.cpp under AddressSanitizer and UndefinedBehaviorSanitizer: a program with its own main"""
    exe = str(tmp_path_factory.mktemp("lens") / "lens_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "lens", "lens_exerciser.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(case):
        r = subprocess.run([exe, case], capture_output=True, text=True, timeout=300, env=env)
        assert r.returncode == 0 and r.stdout.strip() == case + " ok", (r.stdout[-500:], r.stderr[-3000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    return run


def test_lens_ray_is_clean_under_asan_and_ubsan(exerciser):
    exerciser("rays")


def test_lens_points_are_clean_under_asan_and_ubsan(exerciser):
    exerciser("points")


def test_lens_kernel_keeps_the_vacuum_step_and_the_register_budget():
    """lens_pixels runs motion_pixels' loop with a lens point per sample: its nested vacuum loop costs what motion_pixels' does per
    RK4 step in the same build, no v_mov, no scratch, no more VGPRs, and the media kernels' 5 waves per SIMD"""
    from test_supersample_host import _isa
    pairs = {"lens_pixels<true, 2, 0>": "motion_pixels<true, 2, 0>", "lens_pixels<true, 2, 2>": "motion_pixels<true, 2, 2>"}
    got, out = _isa(*pairs.keys(), *pairs.values())
    assert set(pairs) | set(pairs.values()) <= set(got), out[-2000:]
    for k, ref in pairs.items():
        assert got[k].get("unroll") == 2 and got[k]["mov"] == 0, (k, got[k])
        assert got[k]["scratch"] == 0, (k, got[k])
        assert got[k]["vgpr"] <= got[ref]["vgpr"] and got[k]["occupancy"] >= 5, (k, got[k], got[ref])
        assert got[k]["per_step"] == got[ref]["per_step"], (k, got[k], got[ref])


def test_drivers_share_the_pairing_and_the_focus():
    """headless.py's helpers: bitrev_K pairs sample m with its lens point, --focus hole is the camera's distance to the origin"""
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import headless
    assert [headless.bit_reverse(m, 8) for m in range(8)] == [0, 4, 2, 6, 1, 5, 3, 7]
    assert [headless.bit_reverse(m, 1) for m in range(1)] == [0] and [headless.bit_reverse(m, 2) for m in range(2)] == [0, 1]
    for n in (4, 16):
        assert [headless.bit_reverse(m, n) for m in range(n)] == [lr.bit_reverse(m, n) for m in range(n)]
        assert sorted(headless.bit_reverse(m, n) for m in range(n)) == list(range(n))
    cam = rrt.CameraState.default()
    x, y, z = (float(v) for v in cam.as_array()[0])
    assert headless.hole_distance(cam) == float(F(math.sqrt(x * x + y * y + z * z))) > 0


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("args,msg", rows("lens", PY), **IDS)
def test_python_driver_refuses(args, msg):
    refused(PY, args, msg)


@pytest.mark.parametrize("args,msg", rows("lens", CPP), **IDS)
def test_cpp_driver_refuses(args, msg):
    refused(CPP, args, msg)
