"""The march cache's sample records (csrc/rrt_device.h: SampleRecord): a retained sample is rewritten at fill
time into the values `time` cannot move, and every replayed frame is evaluated from them.

1. the `sample_records` hook (include/rrt_test_records.h): the same samples through today's raw-row evaluation and through derive-then-evaluate-from-record
   (the production pass 2 itself: its non-KEEP instance, and its KEEP instance as a fill and as replays), bit for bit, on points
   that straddle every gate above the seam by a few ulps -- after a CPU check that they really do -- for the three arithmetics, tables off / dense / banded, times inside and outside the table's window, spin 0 and 0.9.
2. served sequences in which the noise table is switched off and on and the sky is swapped between hits: the record depends on
   neither, so every frame has the uncached launch's bytes.
3. the fill really prunes: lanes whose two envelopes are +0 leave the rows' input masks."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as g
import march_ref as mr
from march_cache_util import BUDGET, VIEWS, delta, fresh, plain, uncached

pytestmark = pytest.mark.gpu

F = np.float32
STRICT, FAST, FMAD = 0, 1, 2
TIMES = (1.0, 7.5, 40.0)            # the tables below cover [0, 8]: 40.0 runs the arithmetic instance


def _ladder(x, k):
    """x and its 2k float32 neighbours, k ulps to either side"""
    out = [F(x)]
    lo = hi = F(x)
    for _ in range(k):
        lo = np.nextafter(lo, F(-np.inf)); hi = np.nextafter(hi, F(np.inf))
        out += [lo, hi]
    return np.array(sorted(out), F)


def _on_axis(rc, y, axis):
    """points of cylindrical radius exactly rc (sqrt(fl(rc^2)) == rc): along +x, +z, -x or -z"""
    rc, y = np.broadcast_arrays(np.asarray(rc, F), np.asarray(y, F))
    z = np.zeros_like(rc)
    cols = {0: (rc, y, z), 1: (z, y, rc), 2: (-rc, y, z), 3: (z, y, -rc)}[axis]
    return np.stack(cols, 1).astype(F)


def _envelope_acc(rc, y):
    """getAccretionDensity's envelope (densities.h:23-33) in float64, and its slab exponent"""
    rc, y = np.asarray(rc, np.float64), np.asarray(y, np.float64)
    q = 10.0 / rc
    thick = 0.8 * np.sqrt(q)
    arg = -(y * y) / (2.0 * thick * thick + 1e-7)
    rim = np.where(rc > 21.25, (1.0 - (rc - 21.25) / 3.75) ** 2, 1.0)
    return np.exp(arg) * q ** 0.4 * rim, arg


def _envelope_dust(rc, y):
    rc, y = np.asarray(rc, np.float64), np.asarray(y, np.float64)
    sm = lambda e0, e1, x: (lambda t: t * t * (3 - 2 * t))(np.clip((x - e0) / (e1 - e0), 0, 1))      # noqa: E731
    thick = 0.25 * (10.0 / rc) ** 0.2
    return np.exp(-(y * y) / (2 * thick * thick + 1e-7)) * sm(25.0, 20.0, rc) * sm(10.0, 15.0, rc)


def _bisect(f, lo, hi):
    """x in [lo, hi] with f(x) = 0 for a monotone f"""
    flo = f(lo)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if (f(mid) > 0) == (flo > 0): lo = mid
        else: hi = mid
    return 0.5 * (lo + hi)


def gate_points():
    """name -> (points (n, 3) float32, the gate's quantity per point in the arithmetic named below, its threshold).  Every group
    has points strictly on both sides of its threshold (asserted on the CPU by test_points_straddle_every_gate)."""
    groups = {}
    r_of = lambda p: mr.radius(p)                                                          # noqa: E731
    # cylindrical radius: the radial gate 10 / 25 and the rim's start 21.25 (float32: exact, the points lie on an axis)
    for name, rc0 in (("rc=10", 10.0), ("rc=21.25", 21.25), ("rc=25", 25.0)):
        pts = np.concatenate([_on_axis(_ladder(rc0, 4), F(y), ax) for y, ax in ((0.1, 0), (0.6, 1), (-2.0, 2))])
        groups[name] = (pts, np.abs(pts[:, [0, 2]]).max(1), F(rc0))
    # zone heights
    for name, y0 in (("|y|=4", 4.0), ("|y|=0.75", F(0.5) * F(1.5))):
        ys = np.concatenate([_ladder(y0, 4), -_ladder(y0, 4)])
        pts = np.concatenate([_on_axis(F(rc), ys, ax) for rc, ax in ((12.0, 0), (17.5, 3))])
        groups[name] = (pts, np.abs(pts[:, 1]), F(y0))
    # the march's radius: near_bh 18, the cloud zone 25, the disk zone 30, the redshift factor's tame range [9, 64)
    for name, r0, y in (("r=9", 9.0, 0.3), ("r=18", 18.0, 0.3), ("r=25", 25.0, 0.2), ("r=30", 30.0, 3.9), ("r=64", 64.0, 0.5)):
        x0 = np.sqrt(float(r0) ** 2 - y * y)
        pts = np.concatenate([_on_axis(_ladder(x0, 12), F(y), ax) for ax in (0, 1)])
        groups[name] = (pts, r_of(pts), F(r0))
    # disk_point's slab cut y^2 rc = 135
    pts = np.concatenate([_on_axis(F(rc), s * _ladder(np.sqrt(135.0 / rc), 6), ax) for rc, ax, s in ((12.0, 0, 1), (20.0, 1, -1), (24.0, 2, 1))])
    groups["y^2 rc=135"] = (pts, (pts[:, 1] * pts[:, 1]) * np.abs(pts[:, [0, 2]]).max(1), F(135.0))
    # the accretion slab exponent -10.5 (y^2 rc = 134.4 there: inside the cut above)
    sets = []
    for rc, ax in ((11.0, 0), (16.0, 1), (20.5, 3)):
        y0 = _bisect(lambda y: _envelope_acc(rc, y)[1] + 10.5, 1.0, 4.0)
        sets.append(_on_axis(F(rc), _ladder(y0, 32), ax))
    pts = np.concatenate(sets)
    groups["slab_arg=-10.5"] = (pts, _envelope_acc(np.abs(pts[:, [0, 2]]).max(1), pts[:, 1])[1], -10.5)
    # envelope * 30.02 = 0.001: through the slab (y) and through the rim (rc -> 25)
    sets = []
    for rc, ax in ((11.0, 0), (16.0, 1), (20.5, 3)):
        y0 = _bisect(lambda y: _envelope_acc(rc, y)[0] * 30.02 - 0.001, 1.0, 4.0)
        sets.append(_on_axis(F(rc), _ladder(y0, 16), ax))
    for y, ax in ((0.0, 0), (0.4, 2)):
        rc0 = _bisect(lambda rc: _envelope_acc(rc, y)[0] * 30.02 - 0.001, 24.0, 25.0)
        sets.append(_on_axis(_ladder(rc0, 16), F(y), ax))
    pts = np.concatenate(sets)
    groups["env_acc*30.02=0.001"] = (pts, _envelope_acc(np.abs(pts[:, [0, 2]]).max(1), pts[:, 1])[0] * 30.02, 0.001)
    # the dust envelope 0.001: through the inner and the outer smoothstep
    sets = []
    for lo, hi, y, ax in ((10.0, 11.0, 0.0, 0), (24.0, 25.0, 0.05, 1), (10.0, 11.0, 0.1, 3)):
        rc0 = _bisect(lambda rc: _envelope_dust(rc, y) - 0.001, lo, hi)
        sets.append(_on_axis(_ladder(rc0, 16), F(y), ax))
    pts = np.concatenate(sets)
    groups["env_dust=0.001"] = (pts, _envelope_dust(np.abs(pts[:, [0, 2]]).max(1), pts[:, 1]), 0.001)
    # the redshift factor's m2 = x^2 + z^2 range [1, 4096)
    for name, rc0 in (("m2=1", 1.0), ("m2=4096", 64.0)):
        pts = np.concatenate([_on_axis(_ladder(rc0, 4), F(0.2), ax) for ax in (0, 3)])
        rc = np.abs(pts[:, [0, 2]]).max(1)
        groups[name] = (pts, rc * rc, F(rc0 * rc0))
    return groups


def sample_set():
    """(points, velocities) float32: the gate groups, then wave-coherent in-zone samples (64 neighbours a few hundredths apart, as
    a 4K frame's wavefronts produce, so that the table switches are on), padded to whole wavefronts.  Velocities: unit vectors;
    every 7th has a non-finite vel.y (inf or NaN) -- the marker that travels as a NaN in the row's vel.x."""
    rng = np.random.default_rng(4711)
    gates = np.concatenate([v[0] for v in gate_points().values()])
    waves = 48
    rc = rng.uniform(10.0, 25.0, waves); ang = rng.uniform(-np.pi, np.pi, waves)
    yc = np.where(rng.random(waves) < 0.6, rng.uniform(-0.7, 0.7, waves), rng.uniform(-3.0, 3.0, waves))
    centre = np.stack([rc * np.cos(ang), yc, rc * np.sin(ang)], 1)
    spread = np.exp(rng.uniform(np.log(1e-3), np.log(0.3), waves))[:, None, None]
    bulk = (centre[:, None, :] + spread * rng.uniform(-0.5, 0.5, (waves, 64, 3))).reshape(-1, 3).astype(F)
    pad = (-len(gates)) % 64
    pts = np.concatenate([gates, bulk[:pad], bulk]).astype(F)
    vel = rng.normal(size=(len(pts), 3))
    vel = (vel / np.linalg.norm(vel, axis=1, keepdims=True)).astype(F)
    vel[::7, 1] = np.where(np.arange(len(vel[::7])) % 2 == 0, F(np.inf), F(np.nan))
    return pts, vel, len(gates)


def test_points_straddle_every_gate():
    """CPU only (it rides in this module for the points' sake): every gate group has points strictly on both sides of its
    threshold, in the float32 arithmetic of the kernels for the gates that are plain compares, and by a margin of many float32
    roundings (float64 restatement) for the three that sit behind an exp / pow."""
    groups = gate_points()
    assert len(groups) == 16
    for name, (pts, val, thr) in groups.items():
        below, above = int((val < thr).sum()), int((val > thr).sum())
        print(name, len(pts), below, above)
        assert below >= 2 and above >= 2, name
    for name in ("slab_arg=-10.5", "env_acc*30.02=0.001", "env_dust=0.001"):
        pts, val, thr = groups[name]
        rel = np.abs(np.asarray(val, np.float64) / thr - 1.0)
        assert rel.max() > 16 * 2.0 ** -23, name       # the ladders are consecutive floats; their ends are >= 16 ulps of the quantity out
    # with the oracle-independent restatements: the gate points cover taken and never-taken samples
    pts = np.concatenate([v[0] for v in groups.values()])
    rc = np.sqrt(pts[:, 0].astype(np.float64) ** 2 + pts[:, 2].astype(np.float64) ** 2)
    inside = (rc > 10.0) & (rc < 25.0)
    e = _envelope_acc(np.where(inside, rc, 15.0), pts[:, 1])[0] * inside
    assert (e * 30.02 > 0.001).any() and (e * 30.02 < 0.001).any()


def _tables(rrt):
    with rrt._lib.using_test_library():
        return {"off": None, "dense": rrt.NoiseTable(8.0), "banded": rrt.NoiseTable(8.0, 0.0, 16)}


@pytest.fixture(scope="module")
def tables():
    import relativisticraytracer_amd as rrt
    t = _tables(rrt)
    yield t
    for nt in t.values():
        if nt is not None:
            nt.destroy()


@pytest.fixture(scope="module")
def samples():
    pts, vel, n_gates = sample_set()
    return g.dev(pts), g.dev(vel), pts, vel, n_gates


@pytest.mark.parametrize("table", ("off", "dense", "banded"))
@pytest.mark.parametrize("spin", (0.9, 0.0))
@pytest.mark.parametrize("arith", (STRICT, FMAD, FAST))
def test_record_evaluation_equals_the_raw_row_evaluation(samples, tables, arith, spin, table):
    import torch
    from conftest import same_bits
    d_p, d_v, pts, vel, n_gates = samples
    n, nt = len(pts), tables[table]
    times = (C.c_float * len(TIMES))(*TIMES)
    has_raw = torch.full((len(TIMES) * n,), -1, dtype=torch.int32, device="cuda"); has_rec = has_raw.clone()
    out_raw = torch.full((len(TIMES) * n * 4,), float("nan"), device="cuda"); out_rec = out_raw.clone()
    rec = torch.full((n * 7,), float("nan"), device="cuda")
    kept = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    from relativisticraytracer_amd import _lib
    ptr = lambda t: C.c_void_p(t.data_ptr())                                               # noqa: E731
    _lib.check(_lib.records_hooks().sample_records(n, ptr(d_p), ptr(d_v), float(spin), arith, nt.id if nt else 0, len(TIMES), times,
                                                   ptr(has_raw), ptr(out_raw), ptr(has_rec), ptr(out_rec), ptr(rec), ptr(kept),
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "sample_records")
    hr, hc = g.host(has_raw).reshape(len(TIMES), n), g.host(has_rec).reshape(len(TIMES), n)
    orr, oc = g.host(out_raw).reshape(len(TIMES), n, 4), g.host(out_rec).reshape(len(TIMES), n, 4)
    r, kept = g.host(rec).reshape(n, 7), g.host(kept)
    assert set(np.unique(hr)) <= {0, 1} and np.array_equal(hr, hc)
    assert np.array_equal(orr.view(np.uint32), oc.view(np.uint32)), "emission / transmittance bits"
    assert same_bits(orr[hr == 0], np.broadcast_to(F([0, 0, 0, 1]), orr[hr == 0].shape))
    taken = hr.any(0)
    print(arith, spin, table, "taken", hr.mean(1), "of", n, "| prunable", (~((r[:, 5] != 0) | (r[:, 6] != 0))).mean())
    assert 0.1 < hr[0].mean() < 0.9 and not np.array_equal(orr[0], orr[1]), "the samples must be taken, and move with time"
    # the records themselves: a taken sample is never prunable; both envelopes +0 (bits) where they are 0
    prunable = ~((r[:, 5] != 0) | (r[:, 6] != 0))
    assert not (taken & prunable).any() and prunable[:n_gates].any() and (~prunable[:n_gates]).any()
    assert np.array_equal(kept, (~prunable).astype(np.int32)), "exactly the prunable lanes leave the input masks"
    assert np.all(r[prunable][:, 5:].view(np.uint32) == 0)
    # the non-finite vel.y marker arrives in shift_g where the redshift factor is evaluated at all
    marked = ~np.isfinite(vel[:, 1])
    assert np.isnan(r[marked & ~prunable, 3]).all() and (marked & ~prunable).sum() > 50
    assert np.isfinite(r[~marked & ~prunable, 3]).all()
    if arith == STRICT:
        # the gates really are hit on both sides ON THE DEVICE: within each envelope group some records keep the envelope, some
        # store +0 (plane 5: accretion, plane 6: dust).  (slab_arg = -10.5 is a pre-test of the envelope gate -- both of its
        # sides store +0, by the proof next to it -- and the zone and radius gates do not show in a plane.)
        o = 0
        for name, (gp, _, _) in gate_points().items():
            k = {"env_acc*30.02=0.001": 5, "env_dust=0.001": 6, "rc=10": 5}.get(name)
            if k is not None:
                e = r[o:o + len(gp), k]
                assert (e == 0).any() and (e != 0).any(), name
            o += len(gp)
        assert np.array_equal(r[:, 1].view(np.uint32), pts[:, 1].view(np.uint32)) and same_bits(r[:, 4], mr.radius(pts))


SEQ_SIZES = ((61, 37), (157, 83))


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd.sky import synthetic_sky
    tex = rrt.SkyTexture(sky)
    other = np.ascontiguousarray(sky[::-1, ::-1])                 # another sky of the same size
    assert not np.array_equal(other, sky)
    tex2 = rrt.SkyTexture(other)
    nt = rrt.NoiseTable(8.0)
    yield torch, rrt, tex, tex2, nt
    rrt.march_cache_release()
    rrt.march_cache_configure(BUDGET)
    nt.destroy(); tex2.destroy(); tex.destroy()


@pytest.mark.parametrize("size", SEQ_SIZES)
@pytest.mark.parametrize("view", ("key1", "in_disk"))
def test_served_frames_when_table_and_sky_change_between_hits(ctx, view, size):
    """miss, fill (table on), then hits with the table off, on again, another sky, another time outside the table's window: the
    record was derived once, by the fill, and every served frame has the uncached launch's bytes."""
    torch, rrt, tex, tex2, nt = ctx
    w, h = size
    cam, fx = rrt.CameraState.from_angles(*VIEWS[view]), rrt.CameraEffects()
    on, off = rrt.RenderParams(spin=0.9, noise_table=nt.id), rrt.RenderParams(spin=0.9)
    seq = [(1.0, tex, on), (1.0, tex, on), (1.016, tex, off), (7.5, tex, on), (7.5, tex2, on), (3.0, tex2, off), (40.0, tex, on), (1.0, tex, on)]
    want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, s, fx, p) for t, s, p in seq])
    s0 = fresh(rrt)
    got = [plain(torch, rrt, w, h, t, cam, s, fx, p) for t, s, p in seq]
    d = delta(rrt, s0)
    print(view, size, d)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), f"frame {i} of the sequence"
    assert not np.array_equal(want[3], want[4]) and not np.array_equal(want[1], want[3])
    assert d["fills"] == 1 and d["hits"] == len(seq) - 2 and d["misses"] == 1


def test_the_fill_prunes_lanes_that_can_never_be_taken(sky):
    """key1 at 157 x 83 through the test library's cache: the fill's pass 2 cleared lanes from the retained rows' input masks
    (the `march_cache_fill` hook), and the frames served from the pruned rows have the uncached bytes."""
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    w, h = 157, 83
    with _lib.using_test_library() as lib:
        tex = rrt.SkyTexture(sky)
        try:
            cam, fx, prm = rrt.CameraState.from_angles(*VIEWS["key1"]), rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
            times = (1.0, 1.0, 1.5, 9.0)
            want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in times])
            s0 = fresh(rrt)
            got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in times]
            d = delta(rrt, s0)
            blocks, pruned = C.c_uint(0), C.c_ulonglong(0)
            _lib.check(_lib.records_hooks().march_cache_fill(-1, C.byref(blocks), C.byref(pruned)), "march_cache_fill")
            print("blocks", blocks.value, "pruned lanes", pruned.value, rrt.march_cache_stats())
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
            assert d["fills"] == 1 and d["hits"] == 2
            assert blocks.value == rrt.march_cache_stats()["blocks_used"] > 0
            assert 0 < pruned.value < blocks.value * 8 * 64
        finally:
            rrt.march_cache_release()
            rrt.march_cache_configure(BUDGET)
            tex.destroy()
