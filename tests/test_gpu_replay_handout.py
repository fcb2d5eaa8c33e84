"""The march cache's replay hands pass 2's rows out: a replaying wave of eval_sample_rows takes
CHUNK whole pool blocks at a time from one device-side cursor until the cursor has passed the blocks in use, on a grid sized from
the occupancy query; pass 3 of the same launch puts the cursor back to 0.  Which wave evaluates a row never mattered to the bytes,
so every frame here is compared, by equality, with the same launch at a cache budget of 0 bytes (march_cache_util.uncached).

What can go wrong is bookkeeping: a block handed out twice or never (the last, partial chunk; a grid far smaller or larger than
the pool), a cursor that is not 0 when the next replay starts (consecutive hits, hits from another stream, a key change, a refill),
an empty row whose out-mask keeps another frame's bits, and a wave that starts late because something else is resident.  The
tests drive those: replay grids of 1 and 3 workgroups through the test library's `replay_grid` hook, the sized grid on a pool
with more chunks than the grid has waves, and sequences of launches.

A SERVED SEQUENCE is the same launch at SERVED_TIMES: a miss, a fill and five hits at different times, the last one outside the
noise table's window (the arithmetic instances take over passes 2 and 3).  Strict and FMAD arithmetic."""
import ctypes as C

import numpy as np
import pytest

from march_cache_util import BUDGET, VIEWS, delta, fresh, plain, uncached
from march_ref import VIEWS as REF_VIEWS

pytestmark = pytest.mark.gpu

CHUNK = 2                               # rrt_kernels.h: kReplayChunk, blocks a wave takes from the cursor at once
SERVED_TIMES = (1.0, 1.75, 2.5, 2.516, 3.25, 0.5, 9.25)
SERVED = {"fills": 1, "hits": 5, "drops": 0, "misses": 1, "uncacheable": 0}
ARITH = {"strict": 0, "fmad": 2}
MIN_BLOCKS = 16384                      # rrt_march_cache.h: kMinBlocks


def same(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), (what, "frame", i, "pixels differing", int((a.reshape(-1, 4) != b.reshape(-1, 4)).any(-1).sum()))


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


@pytest.fixture(scope="module")
def hooked(sky):
    """the whole package on the test library (its own handle registries and its own device cache), with the hooks' table"""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    with _lib.using_test_library():
        tex = rrt.SkyTexture(sky)
        nt = rrt.NoiseTable(4.0)
        hooks = _lib.records_hooks()
        try:
            yield torch, rrt, tex, nt, hooks, _lib
        finally:
            _lib.check(hooks.replay_grid(-1, 0), "replay_grid")
            rrt.march_cache_release()
            rrt.march_cache_configure(BUDGET)
            nt.destroy()
            tex.destroy()


# (view, (w, h), max_steps or None): the bench view at 61 x 37 and key 1 at 157 x 83 at their default budget (412 and 3 056
# blocks in strict arithmetic, measured), and budgets at which the fill uses no block at all (every replaying wave leaves on its
# first look at the cursor), a handful (14: fewer chunks than a grid of 3 workgroups has waves) and odd counts (159, 39)
SMALL_GRID_CASES = (("bench", (61, 37), None), ("key1", (157, 83), None), ("bench", (61, 37), 4), ("bench", (61, 37), 200),
                    ("key1", (157, 83), 100), ("skimmer", (157, 83), 100))
_small_want = {}


def _camera(rrt, view):
    return rrt.CameraState.from_angles(*(VIEWS[view] if view in VIEWS else REF_VIEWS[view]))


@pytest.mark.parametrize("grid", (1, 3))
@pytest.mark.parametrize("arith", list(ARITH))
def test_small_replay_grids_serve_the_uncached_bytes(hooked, arith, grid):
    """replay grids of 1 and 3 workgroups (4 and 12 waves) through the hook: every wave comes back for more many times and the
    last chunk is partial wherever the count is no multiple of CHUNK.  The blocks used are read from the `march_cache_fill` hook;
    across the cases the count is below one chunk's worth per wave of the grid, ragged against the chunk (where CHUNK > 1 allows
    it) and many chunks per wave."""
    torch, rrt, tex, nt, hooks, _lib = hooked
    fx = rrt.CameraEffects()
    counts = {}
    try:
        for view, (w, h), steps in SMALL_GRID_CASES:
            cam = _camera(rrt, view)
            prm = rrt.RenderParams(spin=0.9, arith_mode=ARITH[arith], noise_table=nt.id, **({} if steps is None else {"max_steps": steps}))
            key = (view, w, h, steps, arith)
            if key not in _small_want:
                _small_want[key] = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in SERVED_TIMES])
            s0 = fresh(rrt)
            _lib.check(hooks.replay_grid(-1, grid), "replay_grid")
            got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in SERVED_TIMES]
            d = delta(rrt, s0)
            blocks, pruned = C.c_uint(0), C.c_ulonglong(0)
            _lib.check(hooks.march_cache_fill(-1, C.byref(blocks), C.byref(pruned)), "march_cache_fill")
            counts[key] = blocks.value
            same(got, _small_want[key], (key, grid))
            assert d == SERVED, (key, grid, d)
            assert blocks.value == rrt.march_cache_stats()["blocks_used"], (key, blocks.value, rrt.march_cache_stats())
    finally:
        _lib.check(hooks.replay_grid(-1, 0), "replay_grid")
    print(arith, grid, counts)
    n = list(counts.values())
    waves = 4 * grid
    assert any(c < CHUNK for c in n), ("no case below one chunk", counts)
    assert any(c > CHUNK and c % CHUNK != 0 for c in n), ("no case with a partial last chunk", counts)
    assert any(c >= 64 * CHUNK * waves for c in n), ("no case with many chunks per wave", counts)
    assert any(CHUNK <= c < CHUNK * 12 for c in n), ("no case with fewer chunks than three workgroups have waves", counts)
    assert not np.array_equal(_small_want[("key1", 157, 83, None, arith)][1], _small_want[("key1", 157, 83, None, arith)][5])


REFILL = dict(w=256, h=128, view="in_disk", spin=0.9, max_steps=600, budget=1 << 30)
REFILL_BLOCKS = 18192                   # what that refill uses, strict and FMAD alike (test_gpu_march_cache_exits.py)
SIZED_GRID_WAVES = 256 * 8 * 4          # an MI355X: 256 CUs x 8 workgroups of 4 waves


@pytest.mark.parametrize("arith", list(ARITH))
def test_more_chunks_than_waves_after_a_refill(hooked, arith):
    """256 x 128 from inside the disk, max_steps 600, 1 GiB: a miss, a fill that overflows the first 16 384 blocks, a refill
    (18 192 blocks measured) and five hits on the SIZED grid -- more blocks than the grid has waves times CHUNK, so no wave can
    take the pool in one helping; where CHUNK makes 18 192 too few the hook's grid of 64 workgroups stands in.  This is also the
    cursor's path through a refill: the reallocated header region is zeroed by the refill, the hits follow it."""
    torch, rrt, tex, nt, hooks, _lib = hooked
    cam, fx = _camera(rrt, REFILL["view"]), rrt.CameraEffects()
    prm = rrt.RenderParams(spin=REFILL["spin"], arith_mode=ARITH[arith], max_steps=REFILL["max_steps"], noise_table=nt.id)
    times = (1.0,) + SERVED_TIMES
    fn = lambda t: plain(torch, rrt, REFILL["w"], REFILL["h"], t, cam, tex, fx, prm)      # noqa: E731
    want = uncached(rrt, lambda: [fn(t) for t in times])
    rrt.march_cache_release()
    rrt.march_cache_configure(REFILL["budget"])
    waves = SIZED_GRID_WAVES
    try:
        if REFILL_BLOCKS <= waves * CHUNK:
            _lib.check(hooks.replay_grid(-1, 64), "replay_grid")
            waves = 64 * 4
        s0 = rrt.march_cache_stats()
        got = [fn(t) for t in times]
        d, st = delta(rrt, s0), rrt.march_cache_stats()
    finally:
        _lib.check(hooks.replay_grid(-1, 0), "replay_grid")
        rrt.march_cache_release()
        rrt.march_cache_configure(BUDGET)
    print(arith, d, st)
    same(got, want, ("refill", arith))
    assert d == {"fills": 2, "hits": 5, "drops": 0, "misses": 1, "uncacheable": 0}, d
    assert st["state"] == "ready" and st["blocks_used"] > MIN_BLOCKS and st["blocks_used"] > waves * CHUNK, st
    assert not np.array_equal(want[3], want[4])


@pytest.mark.parametrize("arith", list(ARITH))
def test_the_cursor_across_launches(ctx, arith):
    """key 1 at 157 x 83 on the sized grid: a miss, a fill and ten consecutive hits; then hits alternating between two streams
    without the host waiting in between; then another key takes the cache (miss, fill, hits) and the first comes back (miss,
    fill, hits again).  Every hit finds the cursor at 0 or its frame would lack rows."""
    torch, rrt, tex, nt = ctx
    w, h = 157, 83
    cams = [_camera(rrt, "key1"), _camera(rrt, "in_disk")]
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, arith_mode=ARITH[arith], noise_table=nt.id)
    times = [1.0, 1.0] + [1.25 + 0.5 * k for k in range(9)] + [9.25]
    want = uncached(rrt, lambda: [[plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in times] for cam in cams])
    s0 = fresh(rrt)
    got = [plain(torch, rrt, w, h, t, cams[0], tex, fx, prm) for t in times]
    same(got, want[0], "ten hits")
    assert delta(rrt, s0) == {"fills": 1, "hits": 10, "drops": 0, "misses": 1, "uncacheable": 0}
    # the same key from two streams taking turns, queued back to back
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in times]
    torch.cuda.synchronize()
    for k, t in enumerate(times):
        rrt.launch_raymarch(outs[k], w, h, t, cams[0], tex, fx, prm, stream=streams[k % 2])
    torch.cuda.synchronize()
    same([o.cpu().numpy() for o in outs], want[0], "two streams")
    assert delta(rrt, s0)["hits"] == 10 + len(times)
    # another key and back
    for j in (1, 0):
        got = [plain(torch, rrt, w, h, t, cams[j], tex, fx, prm) for t in times[:6]]
        same(got, want[j][:6], ("key change", j))
    assert delta(rrt, s0) == {"fills": 3, "hits": 10 + len(times) + 8, "drops": 2, "misses": 3, "uncacheable": 0}


@pytest.mark.parametrize("arith", list(ARITH))
def test_hits_beside_a_resident_probe(ctx, arith):
    """hits with rrt.clock_probe -- one wavefront that sleeps 2 ms, the project's bounded probe -- started on a side stream right
    in front of each: a workgroup of pass 2 may find its slot taken and start late; the bytes are the same."""
    torch, rrt, tex, nt = ctx
    w, h = 157, 83
    cam, fx = _camera(rrt, "key1"), rrt.CameraEffects()
    prm = rrt.RenderParams(spin=0.9, arith_mode=ARITH[arith], noise_table=nt.id)
    want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in SERVED_TIMES])
    side = torch.cuda.Stream()
    cbuf = torch.zeros(2, dtype=torch.int64, device="cuda")
    s0 = fresh(rrt)
    got = []
    for k, t in enumerate(SERVED_TIMES):
        if k >= 2:
            rrt.clock_probe(cbuf, 2000, stream=side)
        got.append(plain(torch, rrt, w, h, t, cam, tex, fx, prm))
    same(got, want, "beside the probe")
    assert delta(rrt, s0) == SERVED
    assert int(cbuf.cpu()[1]) > 0, "the probe ran"


def test_workspace_and_captured_launches_take_their_own_paths(ctx):
    """a launch with a caller-owned workspace and a launch captured into a graph, between hits of the same key: neither touches
    the cache's statistics, both have the uncached bytes, and the key is still served afterwards."""
    torch, rrt, tex, nt = ctx
    w, h = 157, 83
    cam, fx = _camera(rrt, "key1"), rrt.CameraEffects()
    prm = rrt.RenderParams(spin=0.9, noise_table=nt.id)
    want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in SERVED_TIMES])
    s0 = fresh(rrt)
    got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in SERVED_TIMES[:4]]
    before = rrt.march_cache_stats()
    ws = rrt.Workspace(64 << 20)
    try:
        wprm = rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2, pass_chains=2)
        assert np.array_equal(plain(torch, rrt, w, h, SERVED_TIMES[4], cam, tex, fx, wprm), want[4])
        assert ws.stats()["rounds_enqueued"] >= 1, "the workspace's three-pass path ran"
    finally:
        ws.destroy()
    g_out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch(g_out, w, h, SERVED_TIMES[5], cam, tex, fx, prm)
    for _ in range(2):
        g_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(g_out.cpu().numpy(), want[5])
    assert rrt.march_cache_stats() == before
    got += [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in SERVED_TIMES[4:]]
    same(got, want, "around the other paths")
    assert delta(rrt, s0) == SERVED
