"""The production march loop on rays the test chose (rrt_unit_march, include/rrt_test.h: march_inline and vacuum_run themselves,
64 consecutive rays one wavefront) against tests/march_ref.py::march_ref, the numpy restatement that tests/test_march_ref.py
proves against the oracle.

The design's promise is that a ray's bits do not depend on the other 63 lanes of its wavefront: the wave-uniform vacuum step
gives the bits of the generic step, a wave that leaves the vacuum loop because one lane escaped brings the others back
unchanged, and the wave's scalar step counter stays right when lanes end at different steps.  Frames only test that for the
waves an 8x8 pixel tile happens to hold; here the test decides who shares a wave.

Strict and FMAD arithmetic: every ray's (position, velocity, steps, hit) equals march_ref in that arithmetic bit for bit, in
every arrangement -- FMAD's is march_ref(arith=FMAD), the fixed fused tree of the oracle, so a fused term
in the wrong order, or a template instance that fuses what another does not, fails here even where every arrangement agrees
with every other.  FAST (a hardware reciprocal root: no restatement) runs the loop without a vacuum path: the partial-wave and
non-finite cases only, between arrangements.  No tolerance anywhere."""
import numpy as np
import pytest

import march_ref as mr

pytestmark = pytest.mark.gpu

STRICT, FAST, FMAD = 0, 1, 2
W, H = 61, 37


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import gpu_util
    return gpu_util


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def run(g, p, v, spin, arith, max_steps, first_step=None, n=None):
    """rrt_unit_march on the first n rays of (p, v) -> (p, v, steps, hit) of ALL rows: rows past n must come back untouched
    (steps / hit keep their -7 fill)"""
    import torch
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    n = len(p) if n is None else n
    dp, dv = g.dev(p), g.dev(v)
    steps = torch.full((len(p),), -7, dtype=torch.int32, device="cuda")
    hit = torch.full((len(p),), -7, dtype=torch.int32, device="cuda")
    fs = None if first_step is None else g.dev(np.ascontiguousarray(first_step, np.int32))
    g.unit("march", n, dp, dv, float(spin), int(arith), int(max_steps), fs, steps, hit)
    return g.host(dp).reshape(-1, 3), g.host(dv).reshape(-1, 3), g.host(steps), g.host(hit)


def same(a, b, sel=slice(None)):
    """bit equality of two (p, v, steps, hit) results on the rows `sel`"""
    return (np.array_equal(_bits(a[0][sel]), _bits(b[0][sel])) and np.array_equal(_bits(a[1][sel]), _bits(b[1][sel]))
            and np.array_equal(a[2][sel], b[2][sel]) and np.array_equal(a[3][sel], b[3][sel]))


def refs(po, p, v, spin, max_steps, first_step=None):
    """march_ref in both restated arithmetics: {STRICT: ..., FMAD: ...}"""
    return {a: mr.march_ref(p, v, spin, max_steps, first_step=first_step, po=po, arith=a) for a in (STRICT, FMAD)}


def pick(res, idx):
    return tuple(x[idx] for x in res)


def vacuum_fillers(rng, n=63):
    """far-vacuum rays: 120 <= r <= 200, moving roughly tangentially -- they stay beyond r = 30 for the whole march, and escape
    at different steps some 500-900 steps in"""
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    t = np.cross(d, rng.normal(size=(n, 3))); t /= np.linalg.norm(t, axis=1, keepdims=True)
    p = d * rng.uniform(120.0, 200.0, (n, 1))
    v = t + 0.2 * d * rng.uniform(-1.0, 1.0, (n, 1)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    return p.astype(np.float32), v.astype(np.float32)


def near_hole_rays(rng, n):
    """rays started at 3 <= r <= 9 in random directions: generic steps from step 0, some fall in within a few dozen steps"""
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    v = rng.normal(size=(n, 3)); v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (d * rng.uniform(3.0, 9.0, (n, 1))).astype(np.float32), v.astype(np.float32)


def solo_waves(p, v, fp, fv, first_step=None):
    """every ray alone in a wavefront of its own whose other 63 lanes hold the fillers; ray i sits in lane (7 i + 3) mod 64.
    Returns (p, v, first_step, rows of the rays)"""
    n = len(p)
    P, V = np.tile(np.concatenate([fp, fp[:1]]), (n, 1)), np.tile(np.concatenate([fv, fv[:1]]), (n, 1))
    rows = np.arange(n) * 64 + (7 * np.arange(n) + 3) % 64
    P[rows], V[rows] = p, v
    fs = None
    if first_step is not None:
        fs = np.zeros(n * 64, np.int32)
        fs[rows] = first_step
    return P, V, fs, rows


def check_arrangements(g, po, p, v, spin, max_steps, ariths, rng, first_step=None, what=""):
    """the rays in the given order, in a seeded random order, and each alone among 63 far-vacuum rays: strict and FMAD ==
    march_ref in that arithmetic, every mode the same bits in all three; returns the strict march_ref's result"""
    n = len(p)
    ref = refs(po, p, v, spin, max_steps, first_step)
    fref = None
    perm = rng.permutation(n)
    fp, fv = vacuum_fillers(rng)
    sp, sv, sfs, rows = solo_waves(p, v, fp, fv, first_step)
    for arith in ariths:
        a = run(g, p, v, spin, arith, max_steps, first_step)
        b = run(g, p[perm], v[perm], spin, arith, max_steps, None if first_step is None else first_step[perm])
        c = run(g, sp, sv, spin, arith, max_steps, sfs)
        lim = np.maximum(max_steps, 0 if first_step is None else first_step)
        assert (a[2] >= 0).all() and (a[2] <= lim).all() and set(np.unique(a[3])) <= {0, 1}, (what, arith)
        if arith in ref:
            assert same(a, ref[arith]), (what, arith, "image order", int((a[2] != ref[arith][2]).sum()))
        inv = np.empty(n, np.int64); inv[perm] = np.arange(n)
        assert same(pick(b, inv), a), (what, arith, "permuted", int((b[2][inv] != a[2]).sum()))
        assert same(pick(c, rows), a), (what, arith, "alone among vacuum rays", int((c[2][rows] != a[2]).sum()))
        if arith in ref and first_step is None:               # the fillers too: the same 63 rays whoever the 64th lane is
            fref = fref or refs(po, fp, fv, spin, max_steps)
            other = np.setdiff1d(np.arange(64), rows[:1] % 64)
            assert same(pick(c, other), pick(fref[arith], np.where(other < 63, other, 0))), (what, arith, "fillers")
    return ref[STRICT]


@pytest.mark.parametrize("view,spin,budget", [("default", 0.9, 1000), ("default", 0.0, 1000), ("skimmer", 0.9, 1000),
                                              ("in_disk", 0.0, 1500)])
def test_frame_rays_in_three_arrangements(g, po, sky, view, spin, budget):
    """a frame's primary rays in image order, permuted, and 64 chosen ones each alone among 63 far-vacuum rays: the chosen
    rays are those the oracle says hit, escaped, ran out of steps, or crossed the disk"""
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(20261016)
    cam = rrt.CameraState.from_angles(*mr.VIEWS[view]).as_array()
    p0, v0 = mr.primary_rays(po, cam, W, H, sky, spin=spin)
    o = po.render(po.camera(cam[0], cam[1], cam[2], cam[3]), po.default_effects(), po.default_params(spin=spin, max_steps=budget),
                  0.0, W, H, sky, want=("diag",))
    out = (o["steps"] == budget) & (o["hit"] == 0)
    classes = {"hit": o["hit"] == 1, "out": out, "escaped": (o["hit"] == 0) & ~out, "disk": o["n_samples"] > 0}
    chosen = []
    for name, m in classes.items():
        assert m.any(), (view, spin, budget, name)                 # the view and budget offer every kind of ray
        idx = np.setdiff1d(np.flatnonzero(m), chosen)
        chosen += list(rng.choice(idx, min(16, len(idx)), replace=False))
    rest = np.setdiff1d(np.arange(W * H), chosen)
    chosen = np.array(chosen + list(rng.choice(rest, 64 - len(chosen), replace=False)))
    assert len(np.unique(chosen)) == 64
    # the whole frame: image order and a permutation (check_arrangements' third arrangement is run on the 64 chosen rays)
    ref = refs(po, p0, v0, spin, budget)
    assert np.array_equal(ref[STRICT][2], o["steps"]) and np.array_equal(ref[STRICT][3], o["hit"])
    assert not same(ref[FMAD], ref[STRICT])                         # the FMAD equalities below are not the strict ones again
    perm = rng.permutation(W * H)
    inv = np.empty(W * H, np.int64); inv[perm] = np.arange(W * H)
    for arith in (STRICT, FMAD):
        a = run(g, p0, v0, spin, arith, budget)
        b = run(g, p0[perm], v0[perm], spin, arith, budget)
        assert same(a, ref[arith]), (view, spin, arith, int((a[2] != ref[arith][2]).sum()))
        assert same(pick(b, inv), a), (view, spin, arith, int((b[2][inv] != a[2]).sum()))
        assert (a[2] <= budget).all()
    check_arrangements(g, po, p0[chosen], v0[chosen], spin, budget, (STRICT, FMAD), rng, what=(view, spin, "chosen"))


@pytest.mark.parametrize("spin", mr.SPINS)
def test_one_near_hole_ray_among_vacuum_rays_and_the_reverse(g, po, spin):
    rng = np.random.default_rng(77)
    hp, hv = near_hole_rays(rng, 64)
    fp, fv = vacuum_fillers(rng, 64)
    mixed_p = np.concatenate([hp[:1], fp[1:], fp[:1], hp[1:]])
    mixed_v = np.concatenate([hv[:1], fv[1:], fv[:1], hv[1:]])
    pure_p, pure_v = np.concatenate([hp, fp]), np.concatenate([hv, fv])
    to_pure = np.concatenate([[0], 64 + np.arange(1, 64), [64], np.arange(1, 64)])       # mixed row -> the same ray's pure row
    for budget in (40, 333, 900):
        both = refs(po, pure_p, pure_v, spin, budget)
        ref = both[STRICT]
        assert not ref[3][64:].any() and (budget < 900 or (ref[3][:64].any() and not ref[3][:64].all()))     # some near-hole rays fall in
        for arith in (STRICT, FMAD):
            pure = run(g, pure_p, pure_v, spin, arith, budget)
            mixed = run(g, mixed_p, mixed_v, spin, arith, budget)
            assert same(pure, both[arith]), (spin, budget, arith)
            assert same(mixed, pick(pure, to_pure)), (spin, budget, arith, int((mixed[2] != pure[2][to_pure]).sum()))


@pytest.mark.parametrize("spin", mr.SPINS)
def test_lanes_escape_at_different_steps_and_the_budget_ends_among_them(g, po, spin):
    """64 rays of one wave just inside r = 250, heading outward from staggered radii: they escape one after the other, at both
    positions of the vacuum loop's doubled body.  The budget is set to the step at which the first, the middle and the last
    one escapes, and to one less than each."""
    rng = np.random.default_rng(250)
    d = rng.normal(size=(64, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    r0 = 250.0 - 0.11 - 0.3 * rng.permutation(64) * 0.83                    # 0.3 = the vacuum step: ~one lane per step
    p, v = (d * r0[:, None]).astype(np.float32), d.astype(np.float32)
    free = mr.march_ref(p, v, spin, 400, po=po)
    e = free[2]
    assert not free[3].any() and e.max() < 400 and len(np.unique(e)) >= 40   # all escape, at many different steps
    assert len(set(np.unique(e) % 2)) == 2
    srt = np.sort(e)
    budgets = sorted({int(b) for s in (srt[0], srt[32], srt[-1]) for b in (s, s - 1) if s - 1 >= 0})
    assert len(budgets) >= 5 and {b % 2 for b in budgets} == {0, 1}
    for budget in budgets:
        ref = check_arrangements(g, po, p, v, spin, budget, (STRICT, FMAD), rng, what=("staggered", spin, budget))
        assert np.array_equal(ref[2], np.minimum(e, budget))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 127])
def test_partial_waves(g, po, sky, n):
    """n rays of 128: the first n march exactly as in the full launch, the rows past n are not touched"""
    import relativisticraytracer_amd as rrt
    cam = rrt.CameraState.from_angles(*mr.VIEWS["default"]).as_array()
    p0, v0 = mr.primary_rays(po, cam, W, H, sky, spin=0.9)
    rows = np.random.default_rng(n).choice(W * H, 128, replace=False)
    p, v = p0[rows], v0[rows]
    ref = refs(po, p, v, 0.9, 700)
    for arith in (STRICT, FMAD, FAST):
        full = run(g, p, v, 0.9, arith, 700)
        part = run(g, p, v, 0.9, arith, 700, n=n)
        if arith in ref:
            assert same(full, ref[arith]), (n, arith)
        assert same(part, full, slice(0, n)), (n, arith)
        assert np.array_equal(_bits(part[0][n:]), _bits(p[n:])) and np.array_equal(_bits(part[1][n:]), _bits(v[n:])), (n, arith)
        assert (part[2][n:] == -7).all() and (part[3][n:] == -7).all(), (n, arith)
        # the same n rays in reverse order: other lanes, and for n = 65 / 127 other wave-mates
        rev = run(g, p[:n][::-1], v[:n][::-1], 0.9, arith, 700)
        assert same(pick(rev, np.arange(n)[::-1]), pick(full, np.arange(n))), (n, arith, "reversed")


@pytest.mark.parametrize("kind", ["vacuum", "near_hole"])
def test_non_finite_lanes_terminate_and_leave_their_wave_mates_alone(g, po, kind):
    """a NaN position, an Inf velocity and a ray at the origin among 61 ordinary rays: the ordinary rays march as if the three
    were ordinary too; the three only have to come back, within the budget"""
    rng = np.random.default_rng(404)
    p, v = vacuum_fillers(rng, 64) if kind == "vacuum" else near_hole_rays(rng, 64)
    bad = np.array([5, 17, 40])
    good = np.setdiff1d(np.arange(64), bad)
    bp, bv = p.copy(), v.copy()
    bp[5] = (np.nan, 1.0, 2.0)
    bv[17] = (np.inf, 0.0, 0.0)
    bp[40] = (0.0, 0.0, 0.0)
    budget = 300
    ref = refs(po, p, v, 0.9, budget)
    for arith in (STRICT, FMAD, FAST):
        clean = run(g, p, v, 0.9, arith, budget)
        dirty = run(g, bp, bv, 0.9, arith, budget)
        if arith in ref:
            assert same(clean, ref[arith]), (kind, arith)
        assert same(dirty, clean, good), (kind, arith, int((dirty[2][good] != clean[2][good]).sum()))
        assert (dirty[2][bad] >= 0).all() and (dirty[2][bad] <= budget).all(), (kind, arith, dirty[2][bad])
        assert dirty[2][40] == 0 and dirty[3][40] == 1                       # r = 0 is inside the horizon: ends at step 0


@pytest.mark.parametrize("spin", mr.SPINS)
def test_rays_resumed_from_staggered_steps(g, po, sky, spin):
    """d_first_step: the instance a resumed ray runs (per-lane step counter), started from steps 0..7 within a wave"""
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(8)
    cam = rrt.CameraState.from_angles(*mr.VIEWS["skimmer"]).as_array()
    p0, v0 = mr.primary_rays(po, cam, W, H, sky, spin=spin)
    rows = rng.choice(W * H, 128, replace=False)
    p, v = p0[rows], v0[rows]
    fp, fv = vacuum_fillers(rng, 64)
    p, v = np.concatenate([p, fp]), np.concatenate([v, fv])               # two mixed waves and a pure vacuum wave
    first = (rng.permutation(len(p)) % 8).astype(np.int32)
    for budget in (5, 9, 150, 601):
        ref = check_arrangements(g, po, p, v, spin, budget, (STRICT, FMAD), rng, first_step=first, what=("resumed", spin, budget))
        late = first >= budget
        assert np.array_equal(ref[2][late], first[late]) and np.array_equal(_bits(ref[0][late]), _bits(p[late]))
    # first step 0 everywhere is the other instance's result
    zero = np.zeros(len(p), np.int32)
    for arith in (STRICT, FMAD):
        assert same(run(g, p, v, spin, arith, 333, zero), run(g, p, v, spin, arith, 333))
