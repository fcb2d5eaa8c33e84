"""The tile sort (csrc/rrt_tile_sort.h) restated for the tests, in numpy and plain Python: its launch geometry from the header's
constants (read as text), the static dispatch order it sorts over, what its two passes and its hist[block][digit] matrices must
hold, and the key patterns tests/test_gpu_tile_sort.py drives it with.  tests/test_tile_sort_geometry.py asserts, without a GPU,
that the shapes of the GPU file still reach the branches they are there for.  No GPU, no library: numpy only."""
import functools
import os
import re

import numpy as np

import post_geometry as pg

_TEXT = open(os.path.join(pg.CSRC, "rrt_tile_sort.h")).read()
_M = re.search(r"^#define\s+RRT_SORT_THREADS\s+(\d+)\s*$", _TEXT, flags=re.M)
assert _M and re.search(r"\bkThreads\s*=\s*RRT_SORT_THREADS\s*;", _TEXT), "rrt_tile_sort.h no longer takes kThreads from RRT_SORT_THREADS"
SORT = dict(pg.constants("rrt_tile_sort.h", ("kBatch", "kMaxBlocks", "kWalk")), kThreads=int(_M.group(1)))
SORT["kItems"] = SORT["kBatch"] // SORT["kThreads"]
SORT["kWaves"] = SORT["kThreads"] // 64
SORT["kParts"] = SORT["kThreads"] // 256
SORT["kScratchWords"] = 2 * 256 * SORT["kMaxBlocks"]

TILE_COST_SORT_LO = pg.constants("rrt_kernels.h", ("kTileCostSortLo",))["kTileCostSortLo"]       # production's window


def reps_for(n):
    """batches per block (rrt_tile_sort.h: reps_for)"""
    r = 1
    while (n + SORT["kBatch"] * r - 1) // (SORT["kBatch"] * r) > SORT["kMaxBlocks"]:
        r *= 2
    return r


def blocks_for(n):
    c = SORT["kBatch"] * reps_for(n)
    return (n + c - 1) // c


def reach(n):
    """what a sort of n keys runs through: (reps, n_blocks, keys of the last block, wavefronts of the last block's scatter that hold
    keys, later batches of the last block's histogram that hold none, rounds of the scatter's column walk, valid lanes of the last
    64-key step that holds keys)"""
    reps, blocks = reps_for(n), blocks_for(n)
    last = n - (blocks - 1) * SORT["kBatch"] * reps
    share = SORT["kItems"] * 64 * reps                       # consecutive keys per wavefront of a scatter block
    waves = (last + share - 1) // share
    empty = reps - (last + SORT["kBatch"] - 1) // SORT["kBatch"]
    walk = (blocks + SORT["kWalk"] * SORT["kParts"] - 1) // (SORT["kWalk"] * SORT["kParts"])
    return reps, blocks, last, waves, empty, walk, (n - 1) % 64 + 1


@functools.lru_cache(maxsize=2)
def static_order(gx, gy):
    """dispatch slot -> wave tile of the static launch: row blocks from the middle outwards (rrt_tile_sort.h: static_tile); read-only"""
    j = np.arange(gy, dtype=np.int64)
    mid = (gy - 1) >> 1
    rb = np.where(j & 1, mid + ((j + 1) >> 1), mid - (j >> 1))
    order = (rb[:, None] * gx + np.arange(gx, dtype=np.int64)[None, :]).reshape(-1).astype(np.uint32)
    order.flags.writeable = False
    return order


def block_digit_counts(keys, shift, n):
    """hist[b * 256 + d]: how many keys of block b's chunk of `keys` have the (inverted) digit d"""
    chunk = SORT["kBatch"] * reps_for(n)
    digit = 255 - ((keys.astype(np.int64) >> shift) & 255)
    return np.bincount((np.arange(n, dtype=np.int64) // chunk) * 256 + digit, minlength=blocks_for(n) * 256).astype(np.uint32)


def expected(cost, gx, gy, lo_bit):
    """everything a run leaves behind: the permutation, pass 0's output (32-bit cost words and tiles, stably sorted on the low digit
    alone) and the two hist matrices (pass 0 counts over the static order, pass 1 over pass 0's output)"""
    n = gx * gy
    static = static_order(gx, gy)
    words = cost[static]                                                  # pass 0 carries the whole cost word along
    keys = (words >> np.uint32(lo_bit)) & np.uint32(0xffff)
    # descending and stable = stable ascending sort of the inverted key (16 / 8 bit integers: numpy's stable sort is a radix sort)
    by_key = np.argsort((0xffff - keys).astype(np.uint16), kind="stable")
    by_low = np.argsort((255 - (keys & 255)).astype(np.uint8), kind="stable")
    return {"static": static, "keys": keys, "perm": static[by_key], "keys_tmp": words[by_low], "vals_tmp": static[by_low],
            "hist0": block_digit_counts(keys, 0, n), "hist1": block_digit_counts(keys[by_low], 8, n)}


PATTERNS = ("all_equal", "increasing", "decreasing", "uniform", "low_byte_only", "high_byte_only", "alternate_lane",
            "alternate_wave", "alternate_chunk", "high_byte_is_block", "frame_like", "zero_tail")
LARGE_PATTERNS = ("uniform", "frame_like", "high_byte_is_block")
MONOTONE_MAX_N = 65536                                       # strictly monotone 16-bit keys exist up to here


def pattern_keys(name, n, rng):
    """the 16-bit keys of a pattern, along the STATIC order (element i = dispatch slot i)"""
    i = np.arange(n, dtype=np.int64)
    chunk = SORT["kBatch"] * reps_for(n)
    if name == "all_equal":
        k = np.full(n, 0x1234)
    elif name == "increasing":
        k = 65536 - n + i                                     # ends at 0xffff: every key its own value
    elif name == "decreasing":
        k = 65535 - i                                         # starts at 0xffff
    elif name == "uniform":
        k = rng.integers(0, 65536, n)
    elif name == "low_byte_only":
        k = 0x4200 | rng.integers(0, 256, n)
    elif name == "high_byte_only":
        k = (rng.integers(0, 256, n) << 8) | 0x5a
    elif name == "alternate_lane":
        k = np.where(i & 1, 0x0180, 0x8001)
    elif name == "alternate_wave":
        k = np.where((i >> 6) & 1, 0x0180, 0x8001)
    elif name == "alternate_chunk":
        k = np.where((i // chunk) & 1, 0x0180, 0x8001)
    elif name == "high_byte_is_block":
        k = (((i // chunk) & 255) << 8) | rng.integers(0, 256, n)
    elif name == "frame_like":
        k = np.full(n, 0x0107)
        heavy = rng.choice(n, size=min(300, max(1, n // 100)), replace=False)
        k[heavy] = rng.integers(0x0108, 65536, heavy.size)
    elif name == "zero_tail":
        k = rng.integers(0, 65536, n)
        k[(n - 1) // 64 * 64:] = 0                            # the valid lanes of the last 64-key step: digit 255, like the padding
    else:
        raise KeyError(name)
    return k.astype(np.uint32)


def pattern_cost(name, gx, gy, lo_bit, seed):
    """32-bit cost words per wave TILE whose window (bits lo_bit .. lo_bit+15) holds the pattern along the static order; the bits
    outside the window are random in every pattern: they must not matter"""
    n = gx * gy
    rng = np.random.default_rng(seed)
    keys = pattern_keys(name, n, rng)
    window = np.uint32((0xffff << lo_bit) & 0xffffffff)
    noise = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32) & ~window
    cost = np.empty(n, np.uint32)
    cost[static_order(gx, gy)] = (keys << np.uint32(lo_bit)) | noise
    return cost
