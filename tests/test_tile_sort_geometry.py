"""The tile sort's launch geometry (csrc/rrt_tile_sort.h) switches where no production frame goes: a second batch per block past
kBatch * kMaxBlocks = 2 097 152 wave tiles (an 8K frame has 518 400), a second round of the scatter's column walk past 64 blocks,
last blocks whose later batches and wavefronts hold no key.  tests/test_gpu_tile_sort.py runs the kernels on grids that reach
those branches, on keys it chose.

COVERAGE IS A CONDITION: this file asserts, without a GPU, that every one of those shapes still reaches what it is there for.  It
asks the library's own planner (rrt_unit_tile_sort_plan, host only) and reads the constants out of the header
(tests/tile_sort_ref.py), so a retuned constant fails here and names the shape that stopped covering its branch -- the GPU tests
alone would go on passing while covering nothing."""
import ctypes as C

import pytest

import test_gpu_frames as tf             # the tables are read inside the tests: collecting this file needs no GPU
import test_gpu_tile_sort as tt
import tile_sort_ref as ts

# what each shape is there for: (batches per block, blocks, keys of the last block, wavefronts of the last block's scatter that hold
# keys, later batches of the last block's histogram that hold none, rounds of the column walk, valid lanes of the last 64-key step)
REACHES = {
    (1, 1): (1, 1, 1, 1, 0, 1, 1),
    (63, 1): (1, 1, 63, 1, 0, 1, 63),
    (1, 65): (1, 1, 65, 1, 0, 1, 1),
    (2047, 1): (1, 1, 2047, 16, 0, 1, 63),
    (2048, 1): (1, 1, 2048, 16, 0, 1, 64),
    (683, 3): (1, 2, 1, 1, 0, 1, 1),
    (1, 4097): (1, 3, 1, 1, 0, 1, 1),
    (4096, 32): (1, 64, 2048, 16, 0, 1, 64),
    (32769, 4): (1, 65, 4, 1, 0, 2, 4),
    (2048, 1024): (1, 1024, 2048, 16, 0, 16, 64),
    (2049, 1024): (2, 513, 1024, 4, 1, 9, 64),
    (33, 63557): (2, 513, 229, 1, 1, 9, 37),
    (262143, 9): (2, 576, 4087, 16, 0, 9, 55),
    (2048, 2048): (2, 1024, 4096, 16, 0, 16, 64),
    (4097, 1024): (4, 513, 1024, 2, 3, 9, 64),
    (65535, 65): (4, 520, 8127, 16, 0, 9, 63),
}


def plan(n):
    from relativisticraytracer_amd import _lib
    reps, blocks, words = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
    assert _lib.load_test().rrt_unit_tile_sort_plan(n, C.byref(reps), C.byref(blocks), C.byref(words)) == 0
    return reps.value, blocks.value, words.value


def test_the_constants_are_the_ones_the_shapes_were_chosen_for():
    s = ts.SORT
    assert (s["kThreads"], s["kBatch"], s["kMaxBlocks"], s["kWalk"]) == (1024, 2048, 1024, 16)
    assert (s["kItems"], s["kWaves"], s["kParts"], s["kScratchWords"]) == (2, 16, 4, 524288)
    assert ts.TILE_COST_SORT_LO == 6
    first = s["kBatch"] * s["kMaxBlocks"]                   # the last n at one batch per block
    assert [ts.reps_for(n) for n in (1, first, first + 1, 2 * first, 2 * first + 1, 4 * first, 4 * first + 1)] == [1, 1, 2, 2, 4, 4, 8]
    assert [ts.blocks_for(n) for n in (1, 2048, 2049, first, first + 1, 2 * first + 1)] == [1, 1, 2, 1024, 513, 513]


@pytest.mark.parametrize("gx,gy", list(REACHES), ids=[f"{gx}x{gy}" for gx, gy in REACHES])
def test_shape_reaches_its_branch(gx, gy):
    """the library's planner, the restatement the GPU file places its patterns with, and what the shape's row says"""
    assert (gx, gy) in tt.SHAPES
    n = gx * gy
    assert 1 <= gx < 1 << 18 and 1 <= gy <= 65535 and n < 1 << 30          # static_tile's preconditions: inside the contract
    reps, blocks, words = plan(n)
    assert (reps, blocks, words) == (ts.reps_for(n), ts.blocks_for(n), ts.SORT["kScratchWords"]), (gx, gy)
    assert blocks <= ts.SORT["kMaxBlocks"] and 2 * 256 * blocks <= words
    assert ts.reach(n) == REACHES[(gx, gy)], ((gx, gy), ts.reach(n))


def test_shapes_together_reach_every_branch():
    assert set(REACHES) == set(tt.SHAPES) and len(tt.SHAPES) == len(set(tt.SHAPES))
    reach = {s: ts.reach(s[0] * s[1]) for s in tt.SHAPES}
    kmax = ts.SORT["kMaxBlocks"]
    assert {r[0] for r in reach.values()} == {1, 2, 4}
    assert {1, 64, 65, kmax} <= {r[1] for r in reach.values()}
    assert any(r[:2] == (1, kmax) for r in reach.values()) and any(r[:2] == (2, kmax) for r in reach.values())
    for reps in (1, 2, 4):
        assert any(r[0] == reps and r[6] < 64 for r in reach.values()), reps       # a ragged last 64-key step
    assert {1, 2} <= {r[5] for r in reach.values()}                                  # the column walk: one round exactly, a second one
    assert any(r[0] == 2 and r[4] == 1 for r in reach.values())                      # a later batch without a key: histogram's r > 0 on padding only
    assert any(r[0] > 1 and r[3] < ts.SORT["kWaves"] for r in reach.values())        # wavefronts without a key in every batch
    assert any(r[0] > 1 and r[4] == 0 and r[2] % ts.SORT["kBatch"] for r in reach.values())   # a later batch partly filled
    assert {1, 65535, 262143} <= {s[0] for s in tt.SHAPES} and max(s[0] for s in tt.SHAPES) == (1 << 18) - 1       # grid_x up to its limit
    assert 1 in {s[1] for s in tt.SHAPES} and max(s[1] for s in tt.SHAPES) > 60000                                  # quotients near 2^16
    # which patterns run where: the whole set up to FULL_SET_MAX_N, the monotone ones while 16 bits can be strictly monotone
    for gx, gy in tt.SHAPES:
        n, names = gx * gy, tt.patterns_for(gx, gy)
        assert set(ts.LARGE_PATTERNS) <= set(names)
        assert (set(names) == set(ts.PATTERNS)) == (n <= ts.MONOTONE_MAX_N)
        assert (set(ts.PATTERNS) - set(names) <= {"increasing", "decreasing"}) == (n <= tt.FULL_SET_MAX_N)
    assert tt.LO_BIT_SHAPE in tt.SHAPES and {c[3] for c in tt.CASES} == {0, ts.TILE_COST_SORT_LO, 16}


def test_the_frames_of_the_dispatch_test_run_one_batch_per_block():
    """the gap: every geometry tests/test_gpu_frames.py sends through a tile-order object sorts at reps == 1"""
    assert len(tf.ORDERED_FRAME_SIZES) == 5
    for w, h in tf.ORDERED_FRAME_SIZES:
        n = ((w + 7) // 8) * ((h + 7) // 8)
        reps, blocks, _ = plan(n)
        assert reps == 1 and blocks == (n + ts.SORT["kBatch"] - 1) // ts.SORT["kBatch"], (w, h)
    assert max(plan(((w + 7) // 8) * ((h + 7) // 8))[1] for w, h in tf.ORDERED_FRAME_SIZES) == 514


def test_the_patterns_hold_what_they_are_there_for():
    """the key patterns on a three-block grid: host arithmetic only"""
    import numpy as np
    gx, gy = 1, 4097
    n = gx * gy
    for name in ts.PATTERNS:
        for lo in (0, 6, 16):
            cost = ts.pattern_cost(name, gx, gy, lo, seed=3)
            e = ts.expected(cost, gx, gy, lo)
            assert np.array_equal(np.sort(e["perm"]), np.arange(n)), name
            assert np.array_equal(e["perm"], e["static"][np.argsort(-e["keys"].astype(np.int64), kind="stable")]), name   # the plain form
            by_tile = (cost >> np.uint32(lo)) & np.uint32(0xffff)
            assert np.all(np.diff(by_tile[e["perm"]].astype(np.int64)) <= 0), name          # longest first
            assert e["hist0"].sum() == n and e["hist1"].sum() == n
            outside = cost & ~np.uint32((0xffff << lo) & 0xffffffff)
            assert np.unique(outside).size > 1000, name                                       # random bits outside the window
    rng = np.random.default_rng(0)
    assert np.all(np.diff(ts.pattern_keys("increasing", n, rng).astype(np.int64)) > 0)
    assert np.all(np.diff(ts.pattern_keys("decreasing", n, rng).astype(np.int64)) < 0)
    assert np.unique(ts.pattern_keys("uniform", 1 << 17, rng) & 255).size == 256 and np.unique(ts.pattern_keys("uniform", 1 << 17, rng) >> 8).size == 256
    assert np.unique(ts.pattern_keys("low_byte_only", n, rng) >> 8).size == 1 and np.unique(ts.pattern_keys("high_byte_only", n, rng) & 255).size == 1
    k = ts.pattern_keys("high_byte_is_block", n, rng)
    assert np.array_equal(k >> 8, np.arange(n) // 2048)
    k = ts.pattern_keys("frame_like", 1 << 17, rng)
    assert 0.99 <= np.mean(k == np.bincount(k).argmax()) < 1.0 and 200 <= np.sum(k != np.bincount(k).argmax()) <= 300
    k = ts.pattern_keys("zero_tail", n, rng)
    assert np.all(k[4096:] == 0) and n - 4096 == 1
    k = ts.pattern_keys("zero_tail", 2 * 64 + 37, rng)
    assert np.all(k[128:] == 0) and np.count_nonzero(k[:128]) > 100


def test_the_hook_refuses_what_static_tile_cannot_take():
    """RRT_ERR_INVALID_ARGUMENT before any launch: the pointers below are never dereferenced (a launch on this host would be a HIP
    error, status 3, not 1)"""
    from relativisticraytracer_amd import _lib
    lib = _lib.load_test()
    p = [C.c_void_p(0x1000 * k) for k in range(1, 6)]
    words = ts.SORT["kScratchWords"]
    call = lambda gx, gy, lo=6, cost=p[0], keys=p[1], vals=p[2], scratch=p[3], sw=words, perm=p[4]: \
        lib.rrt_unit_tile_sort(gx, gy, cost, lo, keys, vals, scratch, sw, perm, None)
    for gx, gy in ((0, 1), (1, 0), (1 << 18, 1), (1, 65536), (1 << 15, 1 << 15), (262143, 4097)):
        assert call(gx, gy) == 1, (gx, gy)
    assert call(8, 8, lo=-1) == 1 and call(8, 8, lo=17) == 1
    assert call(8, 8, sw=words - 1) == 1 and call(8, 8, sw=0) == 1
    for name in ("cost", "keys", "vals", "scratch", "perm"):
        assert call(8, 8, **{name: None}) == 1, name
    assert lib.rrt_unit_tile_sort_plan(0, None, None, None) == 1 and lib.rrt_unit_tile_sort_plan(1 << 30, None, None, None) == 1
    assert lib.rrt_unit_tile_sort_plan((1 << 30) - 1, None, None, None) == 0
    assert plan((1 << 30) - 1) == (512, 1024, words)


@pytest.mark.parametrize("gx", (1, 2, 3, 683, 2049, 65535, 262143))
def test_static_tile_divides_by_multiplication_exactly(gx):
    """static_tile's claim, in Python integers: with inv = ceil(2^48 / grid_x), (slot * inv) >> 48 == slot // grid_x and the product
    fits 64 bits -- for every slot within +-2 of each multiple of grid_x, up to the largest n a tested grid of this width has
    (grid_y <= 65 535, n < 2^30)"""
    inv = ((1 << 48) + gx - 1) // gx
    n = min(gx * 65535, (1 << 30) - 1)
    assert n >= max([x * y for x, y in tt.SHAPES if x == gx], default=0)
    worst = 0
    for m in range(0, n + gx, gx):
        for slot in range(max(m - 2, 0), min(m + 3, n)):
            prod = slot * inv
            assert prod >> 48 == slot // gx, (gx, slot)
            worst = max(worst, prod)
    assert worst < 1 << 64
