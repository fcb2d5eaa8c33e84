"""The tile sort behind cost-ordered dispatch (csrc/rrt_tile_sort.h) on keys the test chose, at every chunking, against numpy.

rrt_unit_tile_sort (include/rrt_test.h) calls rrt_sort::enqueue -- the instance the launches through a tile-order object call -- on
a cost array per wave tile.  The order it hands out is used as a permutation (a slot duplicated or missing is a tile rendered twice
or never), so every bar here is EQUALITY of words:
  * perm == static[argsort(-keys, stable)] with keys = (cost[static] >> lo_bit) & 0xffff over the static dispatch order;
  * keys_tmp / vals_tmp == the cost words and tiles after a stable sort on the low digit alone (pass 0's output);
  * the two hist[block][digit] matrices == the digit counts of every block's chunk (pass 0 over the static order, pass 1 over pass
    0's output); every other scratch word, and 4 096 words behind each of keys_tmp, vals_tmp and perm, still hold the sentinel;
  * a second run into fresh buffers leaves the same words.
The frames of tests/test_gpu_frames.py reach the sort with measured clocks for keys (nearly all equal) and at one batch per block
only; SHAPES below reach every chunking: one block, the column walk's second round, kMaxBlocks blocks, 2 and 4 batches per block,
last blocks whose later batches and wavefronts are empty.  tests/test_tile_sort_geometry.py asserts, without a GPU, that each shape
still reaches what its comment says.  No case asks the kernels for anything outside their contract."""
import ctypes as C

import numpy as np
import pytest

import tile_sort_ref as ts

pytestmark = pytest.mark.gpu

SHAPES = [                      # (grid_x, grid_y)
    (1, 1),                     # one tile
    (63, 1), (1, 65),           # less than a wavefront; one lane into the second 64-key step
    (2047, 1), (2048, 1),       # around one full block
    (683, 3),                   # 2 049: the second block holds one key
    (1, 4097),                  # 3 blocks, grid_x = 1
    (4096, 32),                 # 64 blocks: exactly one round of the kWalk * kParts column walk
    (32769, 4),                 # 65 blocks: a second walk round, 4 keys in the last block
    (2048, 1024),               # n_blocks == kMaxBlocks at one batch per block
    (2049, 1024),               # 2 batches, 513 blocks, 1 024 keys in the last: its wavefronts 4 .. 15 hold none
    (33, 63557),                # 2 batches, 229 keys in the last block: its second batch is empty; a tall narrow grid
    (262143, 9),                # 2 batches, the largest grid_x, last block 9 keys short
    (2048, 2048),               # 2 batches with n_blocks == kMaxBlocks
    (4097, 1024),               # 4 batches
    (65535, 65),                # 4 batches, grid_x = 65 535, ragged last block (8 127 keys, the last step 63 lanes)
]
FULL_SET_MAX_N = 131076         # the whole pattern set up to here, ts.LARGE_PATTERNS above
LO_BIT_SHAPE = (32769, 4)       # the other two windows (lo_bit 0 and 16), once each
SENTINEL = 0xA5A5A5A5           # no tile index (< 2^30), no digit count
GUARD = 4096


def patterns_for(gx, gy):
    n = gx * gy
    if n > FULL_SET_MAX_N:
        return ts.LARGE_PATTERNS
    return tuple(p for p in ts.PATTERNS if n <= ts.MONOTONE_MAX_N or p not in ("increasing", "decreasing"))


CASES = [(gx, gy, p, ts.TILE_COST_SORT_LO) for gx, gy in SHAPES for p in patterns_for(gx, gy)]
CASES += [LO_BIT_SHAPE + (p, lo) for lo in (0, 16) for p in ("uniform", "frame_like")]


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import gpu_util
    return gpu_util


def plan(n):
    from relativisticraytracer_amd import _lib
    reps, blocks, words = C.c_uint(0), C.c_uint(0), C.c_size_t(0)
    _lib.check(_lib.load_test().rrt_unit_tile_sort_plan(n, C.byref(reps), C.byref(blocks), C.byref(words)), "rrt_unit_tile_sort_plan")
    return reps.value, blocks.value, words.value


def run_sort(g, cost, gx, gy, lo_bit, scratch_words):
    """one run into fresh, sentinel-filled buffers: {name: every word of the buffer, guard words included}"""
    import torch
    n = gx * gy
    fresh = lambda words: torch.full((words,), SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    bufs = {"keys_tmp": fresh(n + GUARD), "vals_tmp": fresh(n + GUARD), "perm": fresh(n + GUARD), "scratch": fresh(scratch_words + GUARD)}
    d_cost = g.dev(cost.view(np.int32))
    g.unit("tile_sort", gx, gy, d_cost, lo_bit, bufs["keys_tmp"], bufs["vals_tmp"], bufs["scratch"], scratch_words, bufs["perm"])
    return {k: g.host(v).view(np.uint32) for k, v in bufs.items()}


@pytest.mark.parametrize("gx,gy,pattern,lo_bit", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-lo{c[3]}" for c in CASES])
def test_tile_sort_matches_the_stable_sort(g, gx, gy, pattern, lo_bit):
    n = gx * gy
    reps, blocks, scratch_words = plan(n)
    assert (reps, blocks, scratch_words) == (ts.reps_for(n), ts.blocks_for(n), ts.SORT["kScratchWords"])
    cost = ts.pattern_cost(pattern, gx, gy, lo_bit, seed=n + 7 * lo_bit)
    want = ts.expected(cost, gx, gy, lo_bit)
    got, again = (run_sort(g, cost, gx, gy, lo_bit, scratch_words) for _ in range(2))
    # the intermediates first: a failure names the pass that broke
    hist1_at = scratch_words // 2
    assert np.array_equal(got["scratch"][:blocks * 256], want["hist0"]), "pass 0's histogram"
    assert np.array_equal(got["keys_tmp"][:n], want["keys_tmp"]), "pass 0's scatter: keys"
    assert np.array_equal(got["vals_tmp"][:n], want["vals_tmp"]), "pass 0's scatter: tiles"
    assert np.array_equal(got["scratch"][hist1_at:hist1_at + blocks * 256], want["hist1"]), "pass 1's histogram"
    assert np.array_equal(got["perm"][:n], want["perm"]), "pass 1's scatter"
    # nothing else was written
    assert np.all(got["scratch"][blocks * 256:hist1_at] == SENTINEL) and np.all(got["scratch"][hist1_at + blocks * 256:] == SENTINEL)
    for name in ("keys_tmp", "vals_tmp", "perm"):
        assert np.all(got[name][n:] == SENTINEL), name
    # the same words again
    for name in got:
        assert np.array_equal(got[name], again[name]), name
    # what the pattern is there for
    if pattern in ("all_equal", "decreasing"):
        assert np.array_equal(got["perm"][:n], want["static"])
    elif pattern == "increasing":
        assert np.array_equal(got["perm"][:n], want["static"][::-1])
    elif pattern == "zero_tail":
        assert np.all(want["keys"][(n - 1) // 64 * 64:] == 0)
