"""The march cache (retained geodesics of a still camera; include/rrt.h) on the GPU: a frame served from
retained geodesics has the bytes of the same launch without the cache -- whatever `time`, the sky, the noise table and the
post-march effects do --, every field of the key invalidates, and the hidden state is safe under streams, threads and graphs.

The reference of every comparison is the SAME launch with the device's cache configured to 0 bytes (the uncached path: the
single kernel), in the same process.  rrt_march_cache_stats says which path a frame took, so that no test can pass by never
caching."""
import ctypes as C
import threading

import numpy as np
import pytest

from march_cache_util import BUDGET, VIEWS, delta, frame, fresh, plain, uncached

pytestmark = pytest.mark.gpu

TIMES = (1.0, 1.0, 1.016, 1.032, 7.5, 31.9)
SIZES = ((61, 37), (157, 83))           # the second: ragged against the 8x8 wave tiles in both directions


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    nt = rrt.NoiseTable(32.0)
    yield torch, rrt, tex, nt
    rrt.march_cache_release()
    rrt.march_cache_configure(BUDGET)
    nt.destroy()
    tex.destroy()


@pytest.mark.parametrize("spin", (0.9, 0.0))
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("view", list(VIEWS))
def test_time_really_varies(ctx, view, size, spin):
    """time = 1.0, 1.0 again, 1.016, 1.032, 7.5, 31.9 through one device's cache: every frame has the uncached launch's bytes;
    1 fill and 4 hits."""
    torch, rrt, tex, nt = ctx
    w, h = size
    cam = rrt.CameraState.from_angles(*VIEWS[view])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=spin, noise_table=nt.id)
    want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES])
    s0 = fresh(rrt)
    got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES]
    d = delta(rrt, s0)
    print(view, size, spin, d, rrt.march_cache_stats())
    for t, a, b in zip(TIMES, got, want):
        assert np.array_equal(a, b), f"t={t}"
    assert not np.array_equal(want[1], want[-1]), "the media must move with time, or this test shows nothing"
    assert d["fills"] == 1 and d["hits"] >= 4 and d["misses"] == 1


def test_row_and_tile_launches_are_cached(ctx):
    """launch_raymarch_tiles with a shard, and launch_raymarch_rows: served from the cache, same bytes."""
    torch, rrt, tex, nt = ctx
    w, h, R, shard, world = 157, 83, 16, 1, 3
    cam = rrt.CameraState.from_angles(*VIEWS["key1"])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    rows = rrt.tile_shard_rows(h, R, shard, world)

    def tiles(t):
        return frame(torch, rows * w * 4, lambda o: rrt.launch_raymarch_tiles(o, w, h, R, shard, world, t, cam, tex, fx, prm))

    def band(t):
        return frame(torch, 30 * w * 4, lambda o: rrt.launch_raymarch_rows(o, w, h, 11, 41, t, cam, tex, fx, prm))

    for fn in (tiles, band):
        want = uncached(rrt, lambda: [fn(t) for t in TIMES])
        s0 = fresh(rrt)
        got = [fn(t) for t in TIMES]
        d = delta(rrt, s0)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert d["fills"] == 1 and d["hits"] == 4


def test_sampled_launch_kinds_are_left_out(ctx):
    """_ss, _mb, _pano and _stereo launches do not go through the cache: its statistics stay where they were."""
    torch, rrt, tex, nt = ctx
    w, h = 64, 40
    cam = rrt.CameraState.default()
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    s0 = fresh(rrt)
    out = torch.zeros(2 * h * w * 4, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        rrt.launch_raymarch_ss(out, w, h, 2, 1.0, cam, tex, fx, prm)
        rrt.launch_raymarch_mb(out, w, h, 1, [0.9, 1.0], [cam, cam], tex, fx, prm)
        rrt.launch_raymarch_pano(out, w, h, 1, rrt.Projection("equirect"), 1.0, cam, tex, fx, prm)
        rrt.launch_raymarch_stereo(out, w, h, 1, rrt.Projection("equirect"), rrt.Stereo("top-bottom"), 1.0, cam, tex, fx, prm)
    torch.cuda.synchronize()
    assert delta(rrt, s0) == {"fills": 0, "hits": 0, "drops": 0, "misses": 0, "uncacheable": 0}
    assert rrt.march_cache_stats()["bytes"] == 0


def _ulp(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _bump_cam(i):
    def f(c):
        vec = ("pos", "forward", "right", "up")[i // 3]
        v = getattr(c["cam"], vec)
        v[i % 3] = _ulp(v[i % 3])
    return f


def _set(where, name, value):
    def f(c):
        setattr(c[where], name, value(getattr(c[where], name)) if callable(value) else value)
    return f


def _setk(name, value):
    def f(c):
        c[name] = value(c[name]) if callable(value) else value
    return f


KEY_FIELDS = [("cam_%d" % i, _bump_cam(i)) for i in range(12)] + [
    ("width", _setk("w", lambda v: v - 1)),
    ("height", _setk("h", lambda v: v - 1)),
    ("one_row_fewer", _setk("y1", lambda v: v - 1)),
    ("first_row", _setk("y0", lambda v: v + 1)),
    ("spin", _set("prm", "spin", _ulp)),
    ("max_steps", _set("prm", "max_steps", lambda v: v - 1)),
    ("nudge_ulps", _set("prm", "nudge_ulps", 1)),
    ("arith_mode", _set("prm", "arith_mode", 2)),
    ("lens_off", _set("fx", "use_lens_distortion", 0)),
    ("distortion_amount", _set("fx", "distortion_amount", _ulp)),
]


def _case(rrt, nt):
    return {"w": 96, "h": 61, "y0": 3, "y1": 58, "cam": rrt.CameraState.from_angles(*VIEWS["key1"]), "fx": rrt.CameraEffects(),
            "prm": rrt.RenderParams(spin=0.9, noise_table=nt.id)}


def _rows(torch, rrt, tex, c, t):
    return frame(torch, (c["y1"] - c["y0"]) * c["w"] * 4,
                 lambda o: rrt.launch_raymarch_rows(o, c["w"], c["h"], c["y0"], c["y1"], t, c["cam"], tex, c["fx"], c["prm"]))


@pytest.mark.parametrize("name,change", KEY_FIELDS, ids=[n for n, _ in KEY_FIELDS])
def test_every_key_field_invalidates(ctx, name, change):
    """render three times (miss, fill, hit), change ONE field of the key by the smallest amount, render: the uncached bytes of
    the changed launch, and the statistics show a drop, not a hit."""
    torch, rrt, tex, nt = ctx
    c = _case(rrt, nt)
    changed = _case(rrt, nt)
    change(changed)
    want = uncached(rrt, lambda: _rows(torch, rrt, tex, changed, 2.5))
    s0 = fresh(rrt)
    for t in (1.0, 1.5, 2.0):
        _rows(torch, rrt, tex, c, t)
    assert delta(rrt, s0) == {"fills": 1, "hits": 1, "drops": 0, "misses": 1, "uncacheable": 0}
    got = _rows(torch, rrt, tex, changed, 2.5)
    d = delta(rrt, s0)
    assert np.array_equal(got, want)
    assert d["hits"] == 1 and d["drops"] == 1 and d["misses"] == 2


# the tile selection of launch_raymarch_tiles: each case changes ONE of (tile_rows, shard, n_shards) and keeps the launch's row
# count (32 rows of the 96-row frame), so that nothing else in the key moves
TILE_BASE = (16, 1, 3)                    # tiles 1, 4
TILE_FIELDS = [("tile_rows", (8, 1, 3)),  # tiles 1, 4, 7, 10 of 8 rows
               ("shard", (16, 2, 3)),     # tiles 2, 5
               ("n_shards", (16, 1, 4))]  # tiles 1, 5


@pytest.mark.parametrize("name,sel", TILE_FIELDS, ids=[n for n, _ in TILE_FIELDS])
def test_tile_selection_invalidates(ctx, name, sel):
    """shard 1 of 3 three times (miss, fill, hit), then another tile size / shard / world with the same number of rows: the
    uncached bytes of THAT selection, a drop and not a hit -- a host that renders its shards one after the other through the
    plain call site must never be served another shard's geodesics."""
    torch, rrt, tex, nt = ctx
    w, h = 96, 96
    cam = rrt.CameraState.from_angles(*VIEWS["key1"])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    assert rrt.tile_shard_rows(h, *TILE_BASE) == rrt.tile_shard_rows(h, *sel) == 32

    def tiles(s_, t):
        R, shard, world = s_
        return frame(torch, 32 * w * 4, lambda o: rrt.launch_raymarch_tiles(o, w, h, R, shard, world, t, cam, tex, fx, prm))
    want_base, want = uncached(rrt, lambda: (tiles(TILE_BASE, 2.5), tiles(sel, 2.5)))
    assert not np.array_equal(want_base, want)
    s0 = fresh(rrt)
    for t in (1.0, 1.5, 2.0):
        tiles(TILE_BASE, t)
    assert delta(rrt, s0) == {"fills": 1, "hits": 1, "drops": 0, "misses": 1, "uncacheable": 0}
    got = tiles(sel, 2.5)
    d = delta(rrt, s0)
    assert np.array_equal(got, want)
    assert d["hits"] == 1 and d["drops"] == 1 and d["misses"] == 2


def test_nudge_seed_and_volumetrics(ctx):
    """the nudge seed is part of the key while a nudge is on; a launch without volumetrics does not touch the cache at all"""
    torch, rrt, tex, nt = ctx
    c = _case(rrt, nt)
    c["prm"].nudge_ulps = 4
    c["prm"].nudge_seed = 7
    changed = _case(rrt, nt)
    changed["prm"].nudge_ulps = 4
    changed["prm"].nudge_seed = 8
    novol = _case(rrt, nt)
    novol["prm"].volumetrics = 0
    want, want_novol, want_c = uncached(rrt, lambda: (_rows(torch, rrt, tex, changed, 2.5), _rows(torch, rrt, tex, novol, 2.5),
                                                       _rows(torch, rrt, tex, c, 3.0)))
    s0 = fresh(rrt)
    for t in (1.0, 1.5, 2.0):
        _rows(torch, rrt, tex, c, t)
    d0 = delta(rrt, s0)
    assert np.array_equal(_rows(torch, rrt, tex, novol, 2.5), want_novol)
    assert delta(rrt, s0) == d0                                       # not even a miss
    assert np.array_equal(_rows(torch, rrt, tex, c, 3.0), want_c)      # ... so the key is still served
    assert delta(rrt, s0)["hits"] == d0["hits"] + 1
    assert np.array_equal(_rows(torch, rrt, tex, changed, 2.5), want)
    d = delta(rrt, s0)
    assert d["drops"] == 1 and d["hits"] == d0["hits"] + 1


def test_what_is_not_in_the_key_hits(ctx, sky):
    """time (inside and outside the noise table's window), the sky, the noise table, the sky filter and the effects applied
    after the march: hits, and still the uncached bytes."""
    torch, rrt, tex, nt = ctx
    w, h = 157, 83
    cam = rrt.CameraState.from_angles(*VIEWS["key1"])
    other_sky = rrt.SkyTexture(np.ascontiguousarray(sky[::-1, ::-1]))
    base_fx = rrt.CameraEffects()
    no_bloom = rrt.CameraEffects(use_bloom=0)
    bloom2 = rrt.CameraEffects(bloom_threshold=0.5, bloom_intensity=0.9)
    no_vig = rrt.CameraEffects(use_vignette=0)
    vig2 = rrt.CameraEffects(vignette_intensity=0.7)
    ca = rrt.CameraEffects(use_chromatic_aberration=1, ca_amount=0.01)
    variants = [(1.0, tex, base_fx, dict(noise_table=nt.id)), (1.0, tex, base_fx, dict(noise_table=nt.id)),
                (2.0, tex, base_fx, dict(noise_table=nt.id)), (40.0, tex, base_fx, dict(noise_table=nt.id)),        # outside the table
                (3.0, tex, base_fx, dict(noise_table=0)), (3.0, other_sky, base_fx, dict(noise_table=nt.id)),
                (3.0, tex, base_fx, dict(noise_table=nt.id, sky_frac_bits=4)),
                (3.25, tex, base_fx, dict(noise_table=nt.id, pass_chains=2)),     # steers caller-owned workspaces only
                (3.5, tex, no_bloom, dict(noise_table=nt.id)), (3.5, tex, bloom2, dict(noise_table=nt.id)),
                (3.5, tex, no_vig, dict(noise_table=nt.id)), (3.5, tex, vig2, dict(noise_table=nt.id)), (3.5, tex, ca, dict(noise_table=nt.id))]

    def run():
        return [plain(torch, rrt, w, h, t, cam, s, fx, rrt.RenderParams(spin=0.9, **kw)) for t, s, fx, kw in variants]
    want = uncached(rrt, run)
    s0 = fresh(rrt)
    got = run()
    d = delta(rrt, s0)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a, b), i
    assert len({a.tobytes() for a in want[2:]}) == len(want) - 2, "every variant must change the frame, or it tests nothing"
    assert d == {"fills": 1, "hits": len(variants) - 2, "drops": 0, "misses": 1, "uncacheable": 0}
    other_sky.destroy()


def test_two_streams_alternating_two_keys(ctx):
    """two streams, each with its own key, taking turns on one device: every launch changes the key, so nothing is ever filled
    and every frame is right; then each stream repeats its key and is served, the other stream's replay waiting for the fill"""
    torch, rrt, tex, nt = ctx
    w, h = 157, 83
    cams = [rrt.CameraState.from_angles(*VIEWS["key1"]), rrt.CameraState.from_angles(*VIEWS["skimmer"])]
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    want = uncached(rrt, lambda: [[plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in (1.0, 2.0, 3.0, 4.0)] for cam in cams])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    s0 = fresh(rrt)
    outs = [[torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(4)] for _ in cams]
    torch.cuda.synchronize()
    for k, t in enumerate((1.0, 2.0, 3.0, 4.0)):
        for j in (0, 1):
            rrt.launch_raymarch(outs[j][k], w, h, t, cams[j], tex, fx, prm, stream=streams[j])
    torch.cuda.synchronize()
    d = delta(rrt, s0)
    assert d["fills"] == 0 and d["hits"] == 0 and d["misses"] == 8
    for j in (0, 1):
        for k in range(4):
            assert np.array_equal(outs[j][k].cpu().numpy(), want[j][k]), (j, k)
    # the same key from both streams without waiting in between: miss, fill on stream 0, replays on streams 1, 0, 1
    s0 = fresh(rrt)
    outs = [torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda") for _ in range(5)]
    torch.cuda.synchronize()
    for k, t in enumerate((1.0, 1.0, 2.0, 3.0, 4.0)):
        rrt.launch_raymarch(outs[k], w, h, t, cams[0], tex, fx, prm, stream=streams[k % 2])
    torch.cuda.synchronize()
    d = delta(rrt, s0)
    assert d["fills"] == 1 and d["hits"] == 3
    for k, kw in enumerate((0, 0, 1, 2, 3)):
        assert np.array_equal(outs[k].cpu().numpy(), want[0][kw]), k


def test_two_host_threads(ctx):
    """two host threads launching the same key and another one through one device's cache: every frame is right"""
    torch, rrt, tex, nt = ctx
    w, h = 96, 61
    cams = [rrt.CameraState.from_angles(*VIEWS["key1"]), rrt.CameraState.from_angles(*VIEWS["bench"])]
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    times = [1.0 + 0.25 * k for k in range(12)]
    want = uncached(rrt, lambda: [[plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in times] for cam in cams])
    fresh(rrt)
    bad = []

    def worker(j, which):
        torch.cuda.set_device(0)
        st = torch.cuda.Stream()
        for k, t in enumerate(times):
            cam_i = which(k)
            got = plain(torch, rrt, w, h, t, cams[cam_i], tex, fx, prm, stream=st)
            if not np.array_equal(got, want[cam_i][k]):
                bad.append((j, k, int((got != want[cam_i][k]).sum()), int((got != 0).sum())))

    th = [threading.Thread(target=worker, args=(0, lambda k: 0)), threading.Thread(target=worker, args=(1, lambda k: 0 if k % 4 else 1))]
    for t_ in th:
        t_.start()
    for t_ in th:
        t_.join()
    assert not bad


def test_graph_capture_ignores_the_cache(ctx):
    """a launch captured into a graph between two cached ones takes the uncached path and records nothing; replayed after the
    cache has been refilled with another key, its bytes are still right"""
    torch, rrt, tex, nt = ctx
    w, h = 128, 72
    cam_a, cam_b = rrt.CameraState.from_angles(*VIEWS["key1"]), rrt.CameraState.from_angles(*VIEWS["in_disk"])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    want_a, want_b = uncached(rrt, lambda: (plain(torch, rrt, w, h, 2.0, cam_a, tex, fx, prm), plain(torch, rrt, w, h, 2.0, cam_b, tex, fx, prm)))
    s0 = fresh(rrt)
    for t in (1.0, 1.5, 2.0):
        got = plain(torch, rrt, w, h, t, cam_a, tex, fx, prm)
    assert np.array_equal(got, want_a)
    before = rrt.march_cache_stats()
    g_out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch(g_out, w, h, 2.0, cam_a, tex, fx, prm)
    assert rrt.march_cache_stats() == before
    assert np.array_equal(plain(torch, rrt, w, h, 2.0, cam_a, tex, fx, prm), want_a)          # still served
    assert delta(rrt, s0)["hits"] == 2
    for t in (1.0, 1.5, 2.0):                                                               # another key takes the cache over
        got = plain(torch, rrt, w, h, t, cam_b, tex, fx, prm)
    assert np.array_equal(got, want_b)
    for _ in range(2):
        g_out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(g_out.cpu().numpy(), want_a)
    assert delta(rrt, s0) == {"fills": 2, "hits": 3, "drops": 1, "misses": 2, "uncacheable": 0}


def test_budget_too_small_and_release(ctx):
    """a budget that cannot hold the frame: the launches stay on the uncached path, no error, and the statistics say why;
    after rrt_march_cache_release the next launches fill again"""
    torch, rrt, tex, nt = ctx
    w, h = 157, 83
    cam = rrt.CameraState.from_angles(*VIEWS["key1"])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES])
    rrt.march_cache_release()
    rrt.march_cache_configure(1 << 20)
    s0 = rrt.march_cache_stats()
    got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES]
    st = rrt.march_cache_stats()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert delta(rrt, s0) == {"fills": 0, "hits": 0, "drops": 0, "misses": 1, "uncacheable": len(TIMES) - 1}
    assert st["state"] == "uncacheable" and st["why"] == "budget" and st["bytes"] == 0 and st["max_bytes"] == 1 << 20
    s0 = fresh(rrt)
    got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert delta(rrt, s0)["fills"] == 1 and delta(rrt, s0)["hits"] == 4
    st = rrt.march_cache_stats()
    assert st["state"] == "ready" and 0 < st["blocks_used"] <= st["blocks_capacity"] and 0 < st["bytes"] <= BUDGET
    rrt.march_cache_release()
    st = rrt.march_cache_stats()
    assert st["bytes"] == 0 and st["state"] == "none"
    s1 = rrt.march_cache_stats()
    got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES]
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert rrt.march_cache_stats()["fills"] == s1["fills"] + 1


def test_pool_overflow_refills_once_then_gives_up(ctx):
    """a budget that holds the bookkeeping and the smallest pool but not this view's samples (a 4K-wide band from inside the
    disk): the fill overflows (its frame is still right: those rays finish in line), cannot grow, and the key stays on the
    uncached path with why = overflow"""
    torch, rrt, tex, nt = ctx
    w, h = 1024, 256
    cam = rrt.CameraState.from_angles(*VIEWS["in_disk"])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9, noise_table=nt.id)
    want = uncached(rrt, lambda: [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES])
    rrt.march_cache_release()
    rrt.march_cache_configure(48 << 20)           # ~2 000 blocks beside 9 MB of bookkeeping
    s0 = rrt.march_cache_stats()
    got = [plain(torch, rrt, w, h, t, cam, tex, fx, prm) for t in TIMES]
    st = rrt.march_cache_stats()
    print(st, delta(rrt, s0))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert st["state"] == "uncacheable" and st["why"] == "overflow"
    assert st["bytes"] == 0                       # a key that has been given up holds no memory
    assert delta(rrt, s0)["hits"] == 0 and delta(rrt, s0)["fills"] == 1


_CHILD = r"""
import hashlib, json, sys
sys.path.insert(0, sys.argv[1])
import torch
import relativisticraytracer_amd as rrt
from relativisticraytracer_amd.sky import synthetic_sky
w, h = 157, 83
tex = rrt.SkyTexture(synthetic_sky())
cam = rrt.CameraState.from_angles((15.0, 3.0, -30.0), -20.0, -5.0)
fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
sha = []
for t in json.loads(sys.argv[2]):
    out.zero_()
    rrt.launch_raymarch(out, w, h, t, cam, tex, fx, prm)
    torch.cuda.synchronize()
    sha.append(hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest())
print("RESULT " + json.dumps({"sha": sha, "stats": rrt.march_cache_stats()}))
"""


def test_environment_switch_in_a_child_process(ctx, sky):
    """RRT_MARCH_CACHE=0 in a fresh child process: the same frames as through this process's cache, and the child's statistics
    stay at zero (no object, no memory, budget 0)."""
    import hashlib
    import json
    import os
    import subprocess
    import sys
    torch, rrt, tex, nt = ctx
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    env = dict(os.environ, RRT_MARCH_CACHE="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, json.dumps(list(TIMES))], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    st = child["stats"]
    assert all(st[k] == 0 for k in ("fills", "hits", "drops", "misses", "uncacheable", "bytes", "max_bytes")) and st["state"] == "none"
    w, h = 157, 83
    cam = rrt.CameraState.from_angles(*VIEWS["key1"])
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    s0 = fresh(rrt)
    got = [hashlib.sha256(plain(torch, rrt, w, h, t, cam, tex, fx, prm).tobytes()).hexdigest() for t in TIMES]
    assert got == child["sha"]
    assert delta(rrt, s0)["fills"] == 1 and delta(rrt, s0)["hits"] == 4


def test_new_symbols_are_exported():
    from relativisticraytracer_amd import _lib
    lib = _lib.load()
    for name in ("rrt_march_cache_configure", "rrt_march_cache_stats", "rrt_march_cache_release"):
        assert hasattr(lib, name)
    info = _lib.rrt_march_cache_info()
    assert lib.rrt_march_cache_stats(-1, C.byref(info)) == 0 and C.sizeof(info) == 80
