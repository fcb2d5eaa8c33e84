"""Stereo frames (rrt_stereo, rrt_launch_raymarch_stereo*, include/rrt.h) on a host without a GPU: the entry points are exported and
bound, the struct and defaults are as documented, every refusal happens before the library touches a device, the host query
rrt_stereo_ray equals the numpy restatement (tests/stereo_ref.py) bit for bit on whole eye frames, base 0 is the mono ray, the
kernel keeps the march's vacuum step and register budget, and both headless drivers refuse what the kernel lacks.  The frames
themselves: tests/test_gpu_stereo.py."""
import ctypes as C
import os

import numpy as np
import pytest

import projection_ref as pr
import stereo_ref as sr
from test_projection_host import _isa, cameras
from test_driver_refusals import CPP, IDS, PY, refused, rows

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
INVALID, BAD_HANDLE, ABI_MISMATCH = 1, 4, 6
NO_SKY = 0x7777000000000001          # never a registered sky: a launch that passes every check stops at the handle lookup
PUBLIC = ("rrt_stereo_default", "rrt_stereo_ray", "rrt_launch_raymarch_stereo", "rrt_launch_raymarch_stereo_tiles")


def test_symbols_are_exported_and_bound():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    bound = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in PUBLIC:
        assert name in bound and hasattr(lib, name), name
    for name in ("Stereo", "stereo_default", "stereo_ray", "launch_raymarch_stereo", "launch_raymarch_stereo_tiles"):
        assert name in rrt.__all__ and hasattr(rrt, name), name


def test_struct_layout_and_defaults():
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    S = _lib.rrt_stereo
    assert C.sizeof(S) == 24
    assert [S.layout.offset, S.base.offset, S.convergence.offset, S.pole_merge_from_deg.offset, S.pole_merge_to_deg.offset] == \
        [4, 8, 12, 16, 20]
    lib = _lib.load()
    for layout in (1, 2):
        st = S()
        assert lib.rrt_stereo_default(layout, C.byref(st)) == 0
        assert (st.struct_size, st.layout, st.base, st.convergence, st.pole_merge_from_deg, st.pole_merge_to_deg) == \
            (24, layout, 1.0, 0.0, 90.0, 90.0)
    for bad in (0, 3, -1):
        assert lib.rrt_stereo_default(bad, C.byref(S())) == INVALID
    assert lib.rrt_stereo_default(1, None) == INVALID
    assert rrt.STEREO_TOP_BOTTOM == 1 and rrt.STEREO_SIDE_BY_SIDE == 2 and rrt.EYE_LEFT == 0 and rrt.EYE_RIGHT == 1
    assert rrt.stereo_default("side-by-side").info() == {"layout": "side-by-side", "base": 1.0, "convergence": 0.0,
                                                          "pole_merge_deg": [90.0, 90.0]}
    st = rrt.Stereo("top-bottom", 0.25, 12.0, (60, 80))
    assert st.info() == {"layout": "top-bottom", "base": 0.25, "convergence": 12.0, "pole_merge_deg": [60.0, 80.0]}
    assert st.composite(64, 32) == (64, 64) and rrt.Stereo("side-by-side").composite(64, 32) == (128, 32)
    with pytest.raises(ValueError):
        rrt.Stereo("interleaved")


def _proj(kind=1):
    from relativisticraytracer_amd import _lib
    p = _lib.rrt_projection()
    assert _lib.load().rrt_projection_default(kind, C.byref(p)) == 0
    return p


def _st(layout=1, base=None, conv=None, merge=None, size=None):
    from relativisticraytracer_amd import _lib
    st = _lib.rrt_stereo()
    assert _lib.load().rrt_stereo_default(layout, C.byref(st)) == 0
    if base is not None:
        st.base = base
    if conv is not None:
        st.convergence = conv
    if merge is not None:
        st.pole_merge_from_deg, st.pole_merge_to_deg = merge
    if size is not None:
        st.struct_size = size
    return st


def _ref(x):
    return C.byref(x) if x is not None else None


def _launch(w, h, s, proj, st, out=1, cam=True, fx=True, prm=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    c, f, p = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams()
    return _lib.load().rrt_launch_raymarch_stereo(C.c_void_p(out) if out else None, None, w, h, s, _ref(proj), _ref(st), 1.0,
                                                  C.byref(c) if cam else None, NO_SKY, C.byref(f) if fx else None,
                                                  C.byref(prm if prm is not None else p), None)


def _tiles(w, h, s, proj, st, tile_rows=16, shard=0, n_shards=1, prm=None):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    c, f, p = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams()
    return _lib.load().rrt_launch_raymarch_stereo_tiles(C.c_void_p(1), w, h, s, tile_rows, shard, n_shards, _ref(proj), _ref(st),
                                                        1.0, C.byref(c), NO_SKY, C.byref(f), C.byref(prm if prm is not None else p),
                                                        None)


def _ray(proj, st, w=8, h=4, eye=0, x=0, y=0):
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    o, d, inside = (C.c_float * 3)(), (C.c_float * 3)(), C.c_int(0)
    return _lib.load().rrt_stereo_ray(_ref(proj), _ref(st), w, h, eye, x, y, C.byref(rrt.CameraState.default()), C.byref(o),
                                      C.byref(d), C.byref(inside))


def _all_refuse(proj, st, want):
    assert _launch(64, 32, 1, proj, st) == want
    assert _tiles(64, 32, 2, proj, st) == want
    assert _ray(proj, st) == want


NAN, INF = float("nan"), float("inf")
BAD_STEREO = [dict(base=-0.5), dict(base=NAN), dict(base=INF), dict(base=-INF), dict(conv=-1.0), dict(conv=NAN), dict(conv=INF),
              dict(merge=(-1.0, 90.0)), dict(merge=(0.0, 90.5)), dict(merge=(60.0, 50.0)), dict(merge=(NAN, 90.0)),
              dict(merge=(10.0, NAN)), dict(merge=(-INF, 10.0)), dict(merge=(10.0, INF))]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("bad", BAD_STEREO, ids=lambda b: "_".join(f"{k}={v}" for k, v in b.items()))
def test_bad_stereo_values_are_refused(kind, bad):
    for layout in (1, 2):
        _all_refuse(_proj(kind), _st(layout, **bad), INVALID)


def test_stereo_refusals():
    # no stereo fisheye domes, whatever the rest
    _all_refuse(_proj(2), _st(1), INVALID)
    _all_refuse(_proj(2), _st(2, base=0.0), INVALID)
    # NULL structs, unknown layouts, wrong struct sizes (of either struct)
    _all_refuse(None, _st(1), INVALID)
    _all_refuse(_proj(1), None, INVALID)
    for layout in (0, 3, -1, 7):
        st = _st(1)
        st.layout = layout
        _all_refuse(_proj(1), st, INVALID)
    for size in (0, 16, 28):
        _all_refuse(_proj(1), _st(1, size=size), ABI_MISMATCH)
    for size in (0, 12, 20):
        p = _proj(0)
        p.struct_size = size
        _all_refuse(p, _st(1), ABI_MISMATCH)
    # the projection's own spans
    p = _proj(1)
    p.vfov_deg = 200.0
    _all_refuse(p, _st(1), INVALID)
    # the host query's own: the eye's frame, the pixel, the eye, NULL outputs
    for w, h, eye, x, y in ((0, 4, 0, 0, 0), (8, 0, 0, 0, 0), (8, 4, 0, 8, 0), (8, 4, 0, 0, 4), (8, 4, 0, -1, 0), (8, 4, 1, 0, -1),
                            (8, 4, 2, 0, 0), (8, 4, -1, 0, 0)):
        assert _ray(_proj(1), _st(1), w, h, eye, x, y) == INVALID, (w, h, eye, x, y)
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    lib, p, st, cam, v = _lib.load(), _proj(1), _st(1), rrt.CameraState.default(), (C.c_float * 3)()
    assert lib.rrt_stereo_ray(C.byref(p), C.byref(st), 8, 4, 0, 0, 0, None, C.byref(v), C.byref(v), None) == INVALID
    assert lib.rrt_stereo_ray(C.byref(p), C.byref(st), 8, 4, 0, 0, 0, C.byref(cam), None, C.byref(v), None) == INVALID
    assert lib.rrt_stereo_ray(C.byref(p), C.byref(st), 8, 4, 0, 0, 0, C.byref(cam), C.byref(v), None, None) == INVALID
    assert lib.rrt_stereo_ray(C.byref(p), C.byref(st), 8, 4, 1, 7, 3, C.byref(cam), C.byref(v), C.byref(v), None) == 0
    # a pinhole's merge angles and an equirect's convergence are checked but not used
    assert _ray(_proj(0), _st(1, merge=(30.0, 60.0))) == 0 and _ray(_proj(1), _st(1, conv=5.0)) == 0


@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("kind", [0, 1])
def test_everything_ss_refuses_is_refused_for_the_composite(kind, layout):
    import relativisticraytracer_amd as rrt
    p, st = _proj(kind), _st(layout)
    for s in (0, 3, 16):
        assert _launch(64, 32, s, p, st) == INVALID and _tiles(64, 32, s, p, st) == INVALID
    assert _launch(64, 32, 1, p, st, out=0) == INVALID
    assert _launch(64, 32, 1, p, st, cam=False) == INVALID
    assert _launch(64, 32, 1, p, st, fx=False) == INVALID
    assert _launch(0, 32, 1, p, st) == INVALID and _launch(64, 0, 1, p, st) == INVALID and _launch(-4, 32, 1, p, st) == INVALID
    assert _launch(64, 32, 1, p, st, prm=rrt.RenderParams(arith_mode=7)) == INVALID
    p40 = rrt.RenderParams()
    p40.struct_size = 40
    assert _launch(64, 32, 1, p, st, prm=p40) == ABI_MISMATCH
    for tr, sh, n in ((0, 0, 1), (16, 1, 1), (16, -1, 2), (16, 0, 0)):
        assert _tiles(64, 32, 2, p, st, tile_rows=tr, shard=sh, n_shards=n) == INVALID, (tr, sh, n)
    # the composite's limits: a mono frame of the eye's size passes where the composite does not
    if layout == 1:
        assert _launch(1, 65535, 8, p, st) == INVALID                          # s 2h = 1 048 560 > 524 280 virtual rows
        assert _launch(1, 32768, 8, p, st) == INVALID and _launch(1, 32767, 8, p, st) == BAD_HANDLE     # s 2h = 524 288 / 524 272
        assert _launch(1, 262140, 1, p, st) == BAD_HANDLE and _launch(1, 262141, 1, p, st) == INVALID   # 2h vs 524 280 rows
        assert _launch(32768, 32768, 1, p, st) == INVALID                       # w 2h = 2^31
        assert _launch(4, 0x40000000, 1, p, st) == INVALID                      # 2h overflows an int
    else:
        assert _launch(32768, 32768, 1, p, st) == INVALID                       # 2w h = 2^31
        assert _launch(4096, 8192, 8, p, st) == INVALID and _launch(4096, 4096, 4, p, st) == BAD_HANDLE   # (s 2w)(s h) vs 2^31
        assert _launch(0x40000000, 1, 1, p, st) == INVALID                      # 2w overflows an int
        assert _launch(1, 65536, 8, p, st) == INVALID and _launch(1, 65535, 8, p, st) == BAD_HANDLE     # s h vs 524 280


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_good_arguments_pass_the_checks(kind, s):
    """... and reach the sky lookup, which refuses the made-up handle: no check said no"""
    import relativisticraytracer_amd as rrt
    for st in (_st(1), _st(2, base=0.0, conv=3.0, merge=(0.0, 0.0)), _st(1, base=2.5, merge=(45.0, 90.0))):
        assert _launch(37, 21, s, _proj(kind), st) == BAD_HANDLE
        assert _tiles(37, 21, s, _proj(kind), st, tile_rows=5, shard=2, n_shards=3) == BAD_HANDLE
        assert _launch(37, 21, s, _proj(kind), st, prm=rrt.RenderParams(workspace=12345, tile_order=54321, path_policy=2,
                                                                         pool_rounds=3, pass_chains=2)) == BAD_HANDLE


def host_rays(kind, fov, vfov, stereo, W, H, eye, cam):
    import relativisticraytracer_amd as rrt
    p = rrt.Projection(("pinhole", "equirect")[kind], *((fov, vfov) if kind == pr.EQUIRECT else ()))
    o, d = np.zeros((H, W, 3), np.float32), np.zeros((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            o[y, x], d[y, x], inside = rrt.stereo_ray(p, stereo, W, H, eye, x, y, cam)
            assert inside
    return o, d


# (kind, fov, vfov, base, convergence, merge, W, H): the eyes every ray test covers
RAYS = [(pr.EQUIRECT, 360.0, 180.0, 1.0, 0.0, (90.0, 90.0), 64, 32), (pr.EQUIRECT, 360.0, 180.0, 0.37, 0.0, (40.0, 75.0), 64, 32),
        (pr.EQUIRECT, 180.0, 90.0, 2.5, 7.0, (10.0, 10.0), 37, 19), (pr.EQUIRECT, 360.0, 180.0, 0.8, 0.0, (0.0, 90.0), 48, 24),
        (pr.PINHOLE, 0.0, 0.0, 1.0, 0.0, (90.0, 90.0), 40, 23), (pr.PINHOLE, 0.0, 0.0, 0.65, 14.0, (90.0, 90.0), 40, 23),
        (pr.PINHOLE, 0.0, 0.0, 3.0, 0.3, (20.0, 30.0), 33, 29)]


@pytest.mark.parametrize("frame", RAYS, ids=lambda f: "%s_b%g_c%g_m%g-%g_%dx%d" % (("pinhole", "equirect")[f[0]], f[3], f[4], *f[5], f[6], f[7]))
def test_host_query_equals_the_restatement_bit_for_bit(po, frame):
    import relativisticraytracer_amd as rrt
    kind, fov, vfov, base, conv, merge, W, H = frame
    for layout in ("top-bottom", "side-by-side"):          # the layout does not enter the ray
        st = rrt.Stereo(layout, base, conv, merge)
        for cam in cameras():
            for eye in (sr.LEFT, sr.RIGHT):
                got_o, got_d = host_rays(kind, fov, vfov, st, W, H, eye, cam)
                want_o, want_d = sr.rays(po, kind, fov, vfov, base, conv, merge, W, H, eye, cam.as_array())
                for what, g, w in (("origin", got_o, want_o), ("dir", got_d, want_d)):
                    bad = g.view(np.uint32) != w.view(np.uint32)
                    assert not bad.any(), (frame, layout, eye, what, int(bad.any(-1).sum()), np.argwhere(bad.any(-1))[:5].tolist())
                n = np.linalg.norm(got_d.astype(np.float64), axis=-1)
                assert np.all(np.abs(n - 1.0) < 1e-6), frame
                pos = cam.as_array()[0].astype(np.float64)
                r = np.linalg.norm(got_o.astype(np.float64) - pos, axis=-1)
                hb = float(sr.half_base(base))
                assert np.all(r <= hb * (1 + 1e-5) + 1e-5), frame      # every origin on (or, merged, inside) the circle of radius hb
                if kind == pr.PINHOLE or merge[0] >= 90.0:
                    assert np.allclose(r, hb, rtol=1e-4, atol=1e-5), frame


def test_the_eyes_are_where_they_should_be(po):
    """the right eye sits toward `right`, the left toward -right; ODS origins are tangent to their column's view (perpendicular to
    its horizontal direction); the pole merge pulls them onto pos; an off-axis pair converges at the zero-parallax distance"""
    import relativisticraytracer_amd as rrt
    cam = rrt.CameraState.default()
    pos, fw, rt = (v.astype(np.float64) for v in cam.as_array()[:3])
    st = rrt.Stereo("top-bottom", 2.0, 10.0)
    for kind in (pr.PINHOLE, pr.EQUIRECT):
        W, H = (40, 20) if kind == pr.PINHOLE else (64, 32)
        ol, dl = host_rays(kind, 360.0, 180.0, st, W, H, sr.LEFT, cam)
        orr, dr = host_rays(kind, 360.0, 180.0, st, W, H, sr.RIGHT, cam)
        c = (H // 2, W // 2)
        assert (orr[c] - pos) @ rt > 0.99 and (ol[c] - pos) @ rt < -0.99, kind
        if kind == pr.EQUIRECT:
            for y, x in ((16, 5), (16, 40), (10, 60)):
                assert abs((orr[y, x] - pos) @ dr[y, x]) < 1e-5, (y, x)   # tangent: the offset is perpendicular to the view
            assert np.array_equal(dl, dr)                                 # ODS: same directions, different origins
    # the pole merge: rows within `from` of the equator keep the full base, rows beyond `to` sit on pos
    stm = rrt.Stereo("top-bottom", 2.0, 0.0, (30.0, 60.0))
    o, _ = host_rays(pr.EQUIRECT, 360.0, 180.0, stm, 64, 36, sr.RIGHT, cam)
    r = np.linalg.norm(o.astype(np.float64) - pos, axis=-1)
    lat = (np.arange(36) + 0.5) / 36 * 180.0 - 90.0
    assert np.allclose(r[np.abs(lat) < 30], 1.0, rtol=1e-5) and np.all(r[np.abs(lat) > 60] == 0)
    mid = (np.abs(lat) > 30) & (np.abs(lat) < 60)
    assert np.all((r[mid] > 0) & (r[mid] < 1)), r[mid]
    # convergence: the centre rays of both eyes cross at pos + 10 fw
    W, H = 40, 20
    ol, dl = host_rays(pr.PINHOLE, 0, 0, st, W, H, sr.LEFT, cam)
    orr, dr = host_rays(pr.PINHOLE, 0, 0, st, W, H, sr.RIGHT, cam)
    for o, d in ((ol, dl), (orr, dr)):
        p = o[H // 2, W // 2].astype(np.float64)
        dd = d[H // 2, W // 2].astype(np.float64)
        t = ((pos + 10 * fw - p) @ fw) / (dd @ fw)
        assert np.linalg.norm(p + t * dd - (pos + 10 * fw)) < 2e-3


def test_base_zero_is_the_mono_ray():
    """base 0: origin == pos bit for bit (a signed-zero pos included) and dir == rrt_projection_ray's, every pixel, both eyes"""
    import relativisticraytracer_amd as rrt
    cams = cameras() + [rrt.CameraState((-0.0, 0.0, -0.0), *rrt.CameraState.default().as_array()[1:])]
    for kind, W, H in (("pinhole", 40, 23), ("equirect", 48, 24)):
        p = rrt.Projection(kind)
        for st in (rrt.Stereo("top-bottom", 0.0, 5.0, (20.0, 40.0)), rrt.Stereo("side-by-side", 0.0)):
            for cam in cams:
                pos = cam.as_array()[0]
                for eye in (0, 1):
                    o, d = host_rays(p.kind, 360.0, 180.0, st, W, H, eye, cam)
                    assert np.array_equal(o.reshape(-1, 3).view(np.uint32), np.tile(pos, (W * H, 1)).view(np.uint32)), (kind, eye)
                    want = np.array([[rrt.projection_ray(p, W, H, x, y, cam)[0] for x in range(W)] for y in range(H)], np.float32)
                    assert np.array_equal(d.view(np.uint32), want.view(np.uint32)), (kind, eye)


def test_stereo_kernel_keeps_the_vacuum_step_and_the_register_budget():
    """The stereo kernel runs the single kernel's march unchanged: its nested vacuum loop costs what panorama_pixels' does per RK4
    step (276 VALU strict, 216 FMAD, no v_mov), with panorama_pixels' VGPRs and occupancy and no scratch: the eye, the origin and
    the off-axis shift before the march cost nothing inside it."""
    strict, fmad = "stereo_pixels<true, 2, 0>", "stereo_pixels<true, 2, 2>"
    ref_strict, ref_fmad = "panorama_pixels<true, 2, 0>", "panorama_pixels<true, 2, 2>"
    got, out = _isa(strict, fmad, ref_strict, ref_fmad)
    assert {strict, fmad, ref_strict, ref_fmad} <= set(got), out[-2000:]
    for k, ref in ((strict, ref_strict), (fmad, ref_fmad)):
        assert got[k].get("unroll") == 2 and got[k]["mov"] == 0, (k, got[k])
        assert got[k]["scratch"] == 0, (k, got[k])
        assert got[k]["vgpr"] == got[ref]["vgpr"] and got[k]["occupancy"] == got[ref]["occupancy"], (k, got[k], got[ref])
        assert got[k]["per_step"] == got[ref]["per_step"], (k, got[k], got[ref])
    assert got[strict]["per_step"] == 276.0 and got[fmad]["per_step"] == 216.0, got


# ---- the drivers' refusals: the rows are tests/test_driver_refusals.py's, run here under the names they have always had
@pytest.mark.parametrize("args,msg", rows("stereo", PY), **IDS)
def test_python_driver_refuses(args, msg):
    refused(PY, args, msg)


@pytest.mark.parametrize("args,msg", rows("stereo", CPP), **IDS)
def test_cpp_driver_refuses(args, msg):
    refused(CPP, args, msg)


def test_python_driver_refuses_other_layouts():
    for args, msg in rows("stereo-layout", PY):
        refused(PY, args, msg)
