"""Frames SERVED by the march cache (retained geodesics) at every exit of the march loop, in every
arithmetic mode and across refills and reallocations: what test_gpu_march_cache.py (the policy: keys, streams, threads, graphs,
budgets) leaves open, because its byte comparisons use strict arithmetic, the default max_steps and frames that fit the first fill.

A fill is march_defer + eval_sample_rows<KEEP> + composite_and_shade<KEEP>; a hit is the last two with kp.replay = 1, over the
first min(kp.n_blocks, block_capacity) retained blocks and the 28 B terminal state of every ray.  Here they run on

  * the (view, spin, budget) set of test_gpu_step_budget.py -- whose CPU test proves that it holds whole frames out of steps in
    the vacuum loop (both parities), rays out of steps near the hole and in the middle of the medium, and mixed frames -- in
    strict, FMAD and FAST arithmetic, through the plain, the _rows and the _tiles call sites;
  * a key whose first fill overflows the pool and whose refill, at kGrowFactor times the capacity, does not;
  * keys of different geometry taking turns on one device's memory (PoolLayout moves, a smaller key uses all an earlier one left);
  * max_steps on both sides of the three-pass bookkeeping's limit.

A SERVED SEQUENCE of a key is the same launch at times (1.0, 1.75, T, T, 9.25): a miss, a fill and three hits, the last one
outside the noise table's window (the arithmetic kernels take over passes 2 and 3).  Every frame of it is compared with the
same launch rendered while the cache is configured to 0 bytes (the single kernel), by equality; in strict and FMAD arithmetic the
first hit at T is the oracle's frame in that arithmetic too.  The counters are asserted after every sequence, so that no case passes without being served."""
import numpy as np
import pytest

from march_cache_util import BUDGET, VIEWS, delta, frame, fresh, plain, uncached
from test_gpu_step_budget import BUDGETS, H, SPINS, T, THREE_PASS_MAX_STEPS, W, camera, coverage, fx_of, oracle
from test_gpu_step_budget import VIEWS as BUDGET_VIEWS

pytestmark = pytest.mark.gpu

SERVED_TIMES = (1.0, 1.75, T, T, 9.25)
SERVED = {"fills": 1, "hits": 3, "drops": 0, "misses": 1, "uncacheable": 0}
ARITH = {"strict": 0, "fmad": 2, "fast": 1}
MIN_BLOCKS = 16384                      # rrt_march_cache.h: kMinBlocks, the first fill's capacity of every small frame


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    nt = rrt.NoiseTable(4.0)            # 9.25 lies outside its window
    yield torch, rrt, tex, nt
    rrt.march_cache_release()
    rrt.march_cache_configure(BUDGET)
    nt.destroy()
    tex.destroy()


def serve(rrt, fn, times=SERVED_TIMES):
    """fn(t) at every time through the device's cache AS IT IS (no release): the frames, and what the counters did meanwhile"""
    s0 = rrt.march_cache_stats()
    got = [fn(t) for t in times]
    return got, delta(rrt, s0)


def same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, "frame", i, "pixels differing", int((a.reshape(-1, 4) != b.reshape(-1, 4)).any(-1).sum()))
    assert len(got) == len(want)


@pytest.mark.parametrize("arith", list(ARITH))
@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("view", BUDGET_VIEWS)
def test_served_frames_at_every_budget(ctx, po, sky, view, spin, arith):
    """61 x 37 with chromatic aberration, every budget of test_gpu_step_budget.py: the served sequence has the uncached launch's
    bytes in the same arithmetic mode; in strict and FMAD arithmetic the first hit at T is the oracle's frame (in that arithmetic)
    at that budget; from inside
    the disk rows really were retained."""
    torch, rrt, tex, nt = ctx
    cam, fx = camera(view), fx_of(rrt)
    prm = {n: rrt.RenderParams(spin=spin, arith_mode=ARITH[arith], max_steps=n, noise_table=nt.id) for n in BUDGETS}
    want = uncached(rrt, lambda: {n: [plain(torch, rrt, W, H, t, cam, tex, fx, prm[n]) for t in SERVED_TIMES] for n in BUDGETS})
    used = {}
    for n in BUDGETS:
        fresh(rrt)
        got, d = serve(rrt, lambda t: plain(torch, rrt, W, H, t, cam, tex, fx, prm[n]))
        st = rrt.march_cache_stats()
        used[n] = st["blocks_used"]
        same(got, want[n], (view, spin, arith, n))
        assert d == SERVED, (view, spin, arith, n, d)
        assert st["state"] == "ready" and st["blocks_used"] <= st["blocks_capacity"], (view, spin, arith, n, st)
        if arith in ("strict", "fmad"):       # the two arithmetics the oracle restates (FMAD: its fixed fused tree)
            o = oracle(po, sky, view, spin, n, arith=ARITH[arith])
            assert np.array_equal(got[2].reshape(H, W, 4), o["rgba8"]), (view, spin, arith, n, "oracle")
        if view == "in_disk":
            assert st["blocks_used"] > 0, (spin, arith, n, st)
    print(view, spin, arith, "blocks retained by budget", used)


# (view, budgets): two budgets at which rays of the 61 x 37 frame run out of steps in the middle of the medium and one at which
# the frame mixes escaped, fallen-in and out-of-steps rays -- coverage() says so, and the test asserts it
ROW_TILE_BUDGETS = {"skimmer": (150, 300, 1000), "in_disk": (17, 300, 1114)}


@pytest.mark.parametrize("arith", ("fmad", "strict"))
@pytest.mark.parametrize("view", list(ROW_TILE_BUDGETS))
def test_row_and_tile_launches_are_served_at_a_budget(ctx, po, sky, view, arith):
    """157 x 83 (ragged against the 8 x 8 wave tiles both ways): a _rows launch with an odd first row and shards 1 and 2 of 3 of a
    _tiles launch with 16-row tiles, at budgets that end in the medium: served sequences with the uncached launches' bytes.  (The
    skimmer's thin disk misses the tiles of shard 1 at every budget -- those rays end in the vacuum or near the hole --; shard 2
    holds the frame's middle.)  No noise table here: passes 2 and 3 run the arithmetic media kernels throughout."""
    torch, rrt, tex, nt = ctx
    w, h, R, shard, world, y0, y1 = 157, 83, 16, 1, 3, 11, 41
    cov = coverage(po, sky)
    mid = {c[2] for c in cov["mid_medium"] if c[0] == view and c[1] == 0.9}
    mixed = {c[2] for c in cov["mixed"] if c[0] == view and c[1] == 0.9}
    budgets = ROW_TILE_BUDGETS[view]
    assert len(set(budgets)) == 3 and set(budgets) <= mid | mixed, (view, sorted(mid), sorted(mixed))
    assert len(set(budgets) & mid) >= 2 and set(budgets) & mixed, (view, sorted(mid), sorted(mixed))
    cam, fx = camera(view), fx_of(rrt)
    n_tile_rows = {s_: rrt.tile_shard_rows(h, R, s_, world) for s_ in (shard, shard + 1)}

    def tiles(prm, s_):
        return lambda t: frame(torch, n_tile_rows[s_] * w * 4, lambda o: rrt.launch_raymarch_tiles(o, w, h, R, s_, world, t, cam, tex, fx, prm))

    def kinds(prm):
        return {"rows": lambda t: frame(torch, (y1 - y0) * w * 4, lambda o: rrt.launch_raymarch_rows(o, w, h, y0, y1, t, cam, tex, fx, prm)),
                "tiles": tiles(prm, shard), "tiles_mid": tiles(prm, shard + 1)}
    cases = [(n, kind) for n in budgets for kind in ("rows", "tiles", "tiles_mid")]
    prm = {n: rrt.RenderParams(spin=0.9, arith_mode=ARITH[arith], max_steps=n) for n in budgets}
    want = uncached(rrt, lambda: {(n, kind): [kinds(prm[n])[kind](t) for t in SERVED_TIMES] for n, kind in cases})
    media = {}                              # rows retained, and frames that move with time: else a case shows little
    for n, kind in cases:
        fresh(rrt)
        got, d = serve(rrt, kinds(prm[n])[kind])
        same(got, want[(n, kind)], (view, arith, n, kind))
        assert d == SERVED, (view, arith, n, kind, d)
        media[(n, kind)] = rrt.march_cache_stats()["blocks_used"] > 0 and not np.array_equal(want[(n, kind)][0], want[(n, kind)][-1])
    print(view, arith, media)
    assert all(v for (n, kind), v in media.items() if view == "in_disk" or kind != "tiles"), media


# a key from inside the disk whose pool need lies above kMinBlocks and inside what kGrowFactor x kMinBlocks leaves of 1 GiB
REFILL = dict(w=256, h=128, view="in_disk", spin=0.9, max_steps=600, budget=1 << 30)
REFILL_TIMES = (1.0, 1.75, T, 4.0, 9.25)


def _refill_case(ctx, arith, max_steps=REFILL["max_steps"]):
    torch, rrt, tex, nt = ctx
    cam, fx = camera(REFILL["view"]), fx_of(rrt)
    prm = rrt.RenderParams(spin=REFILL["spin"], arith_mode=ARITH[arith], max_steps=max_steps, noise_table=nt.id)
    return lambda t: plain(torch, rrt, REFILL["w"], REFILL["h"], t, cam, tex, fx, prm)


@pytest.mark.parametrize("arith", ("strict", "fmad"))
def test_overflowed_fill_is_refilled_larger_and_then_served(ctx, arith):
    """256 x 128 from inside the disk, max_steps 600, 1 GiB: five launches at five times are a miss, a fill that overflows the
    16 384 blocks of a first fill (its own frame is still right: those rays finish in line), a refill into a reallocated pool
    whose headers are zeroed again, and two hits -- all with the uncached launch's bytes.

    Measured on an MI355X, strict and FMAD alike: the refill uses blocks_used = 18 192 of blocks_capacity = 57 603 (what 1 GiB
    holds of the 131 072 blocks asked for; 1 073 724 480 bytes held), the first fill had blocks_capacity = 16 384 in 306 061 824 bytes."""
    torch, rrt, tex, nt = ctx
    fn = _refill_case(ctx, arith)
    want = uncached(rrt, lambda: [fn(t) for t in REFILL_TIMES])
    rrt.march_cache_release()
    rrt.march_cache_configure(REFILL["budget"])
    s0 = rrt.march_cache_stats()
    got, trail = [], []
    for t in REFILL_TIMES:
        got.append(fn(t))
        trail.append({k: v for k, v in rrt.march_cache_stats().items() if k in ("state", "why", "blocks_used", "blocks_capacity", "bytes")})
    d, st = delta(rrt, s0), rrt.march_cache_stats()
    print(arith, d, trail)
    same(got, want, ("refill", arith))
    assert not np.array_equal(want[3], want[4]), "the media must move with time, or the hits show nothing"
    assert d["fills"] == 2 and d["hits"] == 2 and d["uncacheable"] == 0 and d["misses"] == 1 and d["drops"] == 0, d
    assert st["state"] == "ready", st
    assert st["blocks_used"] > MIN_BLOCKS, st                 # rrt_march_cache.h: kMinBlocks -- the first fill could not hold it
    assert st["blocks_used"] <= st["blocks_capacity"], st
    assert trail[1]["blocks_capacity"] == MIN_BLOCKS and trail[2]["blocks_capacity"] > MIN_BLOCKS, trail
    assert trail[2]["bytes"] > trail[1]["bytes"] and st["bytes"] <= REFILL["budget"], trail


def test_a_key_that_inherits_a_grown_pool_fills_once(ctx):
    """after the refill above, WITHOUT a release, the same view at max_steps 599 -- another key, with the same appetite: its own
    capacity rule asks for kMinBlocks, it is given all the grown pool holds (march_cache_reserve: have > blocks), and pass 2's
    planes must sit behind THAT many input blocks.  One fill, no refill, more than kMinBlocks blocks used, the uncached bytes."""
    torch, rrt, tex, nt = ctx
    first, second = _refill_case(ctx, "strict"), _refill_case(ctx, "strict", REFILL["max_steps"] - 1)
    want = uncached(rrt, lambda: [second(t) for t in SERVED_TIMES])
    rrt.march_cache_release()
    rrt.march_cache_configure(REFILL["budget"])
    _, d0 = serve(rrt, first, REFILL_TIMES[:4])
    grown = rrt.march_cache_stats()
    assert d0["fills"] == 2 and d0["hits"] == 1 and grown["state"] == "ready" and grown["blocks_capacity"] > MIN_BLOCKS, (d0, grown)
    got, d = serve(rrt, second)
    st = rrt.march_cache_stats()
    print(grown, st)
    same(got, want, "inherited pool")
    assert d == dict(SERVED, drops=1), d
    assert st["state"] == "ready" and st["bytes"] == grown["bytes"] and st["blocks_capacity"] >= grown["blocks_capacity"], (grown, st)
    assert MIN_BLOCKS < st["blocks_used"] <= st["blocks_capacity"], st


def test_keys_of_different_geometry_reuse_one_devices_memory(ctx):
    """one device cache and no release: 157 x 83 key1, 61 x 37 from inside the disk (smaller: it uses what the first key left, with
    its own PoolLayout), key1 again (dropped in between: it fills again, over the other key's stale rows and masks), 320 x 200
    skimmer in FMAD (larger bookkeeping: the minimum block count no longer fits what is there, so the memory is reallocated).
    Every frame has its uncached bytes; 4 fills, 12 hits, 3 drops; the memory held never shrinks."""
    torch, rrt, tex, nt = ctx
    fx = fx_of(rrt)

    def key(w, h, view, arith):
        cam = rrt.CameraState.from_angles(*VIEWS[view])
        prm = rrt.RenderParams(spin=0.9, arith_mode=ARITH[arith], noise_table=nt.id)
        return lambda t: plain(torch, rrt, w, h, t, cam, tex, fx, prm)
    key1 = key(157, 83, "key1", "strict")
    keys = [("key1 157x83", key1), ("in_disk 61x37", key(61, 37, "in_disk", "strict")), ("key1 157x83 again", key1),
            ("skimmer 320x200 fmad", key(320, 200, "skimmer", "fmad"))]
    want = uncached(rrt, lambda: [[fn(t) for t in SERVED_TIMES] for _, fn in keys])
    s0 = fresh(rrt)
    held, trail = [0], []
    for (name, fn), w_ in zip(keys, want):
        got, d = serve(rrt, fn)
        st = rrt.march_cache_stats()
        trail.append((name, d, st["bytes"], st["blocks_used"], st["blocks_capacity"]))
        same(got, w_, name)
        assert d == dict(SERVED, drops=0 if len(held) == 1 else 1), (name, d)
        assert st["state"] == "ready" and 0 < st["blocks_used"] <= st["blocks_capacity"], (name, st)
        assert st["bytes"] >= held[-1], (name, st["bytes"], held)
        held.append(st["bytes"])
    print(trail)
    assert delta(rrt, s0) == {"fills": 4, "hits": 12, "drops": 3, "misses": 4, "uncacheable": 0}
    assert trail[1][4] >= trail[0][4], "the smaller key is given all the blocks the first one left"
    assert held[4] > held[3], "the larger frame's bookkeeping does not fit beside kMinBlocks blocks in what was there"
    assert len({w_[2].tobytes() for w_ in want}) == 3, "three different keys, three different frames"


def test_above_the_three_pass_limit_nothing_is_cached(ctx):
    """max_steps one above what the three-pass bookkeeping represents, on the far view: three launches at three times have the
    cache-off launch's bytes and move no counter -- not even a miss -- and the memory a served key holds stays as it is; AT the
    limit the same launch is served."""
    torch, rrt, tex, nt = ctx
    cam, fx = camera("far"), fx_of(rrt)
    times = (1.0, T, 9.25)
    above = rrt.RenderParams(spin=0.9, max_steps=THREE_PASS_MAX_STEPS + 1, noise_table=nt.id)
    at = rrt.RenderParams(spin=0.9, max_steps=THREE_PASS_MAX_STEPS, noise_table=nt.id)
    want_above, want_at = uncached(rrt, lambda: ([plain(torch, rrt, W, H, t, cam, tex, fx, above) for t in times],
                                                 [plain(torch, rrt, W, H, t, cam, tex, fx, at) for t in times]))
    s0 = fresh(rrt)
    got, d = serve(rrt, lambda t: plain(torch, rrt, W, H, t, cam, tex, fx, at), times)
    same(got, want_at, "at the limit")
    assert d == {"fills": 1, "hits": 1, "drops": 0, "misses": 1, "uncacheable": 0}, d
    before = rrt.march_cache_stats()
    assert before["bytes"] > 0 and before["state"] == "ready"
    got, d = serve(rrt, lambda t: plain(torch, rrt, W, H, t, cam, tex, fx, above), times)
    same(got, want_above, "above the limit")
    assert d == {"fills": 0, "hits": 0, "drops": 0, "misses": 0, "uncacheable": 0}, d
    assert rrt.march_cache_stats() == before
    assert want_above[1].reshape(H, W, 4)[..., :3].std() > 5.0, "a frame with something in it"
    assert delta(rrt, s0)["hits"] == 1
