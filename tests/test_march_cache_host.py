"""The march cache's host bookkeeping (csrc/rrt_march_cache.h: key, policy state machine, capacity rule) driven with synthetic
keys on the CPU through tests/march_cache/policy_exerciser.cpp, and the new C ABI symbols (tests/test_capi.py checks the whole
export list; these are the cache's own checks)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TODAY, FILL, REPLAY = 0, 1, 2
NONE, SEEN, PENDING, REFILL, READY, OFF = range(6)


@pytest.fixture(scope="module")
def exerciser(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("march_cache") / "policy_exerciser")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "march_cache", "policy_exerciser.cpp"), "-o", exe],
                   check=True)

    def run(*cmds):
        out = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True, check=True).stdout
        return [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    return run


def test_second_launch_fills_third_replays(exerciser):
    r = exerciser("launch 0", "launch 0", "pending 0", "verify 1", "launch 0", "launch 0", "launch 0")
    # (result, state, why, fills, hits, drops, misses, uncacheable)
    assert r[0] == (TODAY, SEEN, 0, 0, 0, 0, 1, 0)
    assert r[1] == (FILL, PENDING, 0, 1, 0, 0, 1, 0)
    assert r[2][0] == 1
    assert r[3][1] == READY
    assert [x[0] for x in r[4:]] == [REPLAY] * 3 and r[-1][3:] == (1, 3, 0, 1, 0)


def test_a_moving_camera_never_fills(exerciser):
    r = exerciser(*["launch %d" % (1 + k % 5) for k in range(40)])
    assert all(x[0] == TODAY for x in r) and r[-1][3:] == (0, 0, 0, 40, 0)


def test_any_other_key_drops_back_to_the_first_state(exerciser):
    r = exerciser("launch 0", "launch 0", "verify 1", "launch 0", "launch 3", "launch 0", "launch 0", "verify 1", "launch 0")
    assert r[3][0] == REPLAY
    assert r[4][:2] == (TODAY, SEEN) and r[4][5] == 1            # a drop, not a hit
    assert r[5][:2] == (TODAY, SEEN) and r[5][5] == 1            # the old key is a new key again
    assert r[6][0] == FILL and r[8][0] == REPLAY
    assert r[8][3:] == (2, 2, 1, 3, 0)
    # a key change while the fill is still unverified is a drop too
    r = exerciser("launch 0", "launch 0", "launch 1")
    assert r[2][:2] == (TODAY, SEEN) and r[2][5] == 1


def test_overflow_refills_once_then_gives_up(exerciser):
    r = exerciser("launch 0", "launch 0", "verify 0", "launch 0", "verify 0", "launch 0", "launch 0", "launch 1", "launch 1")
    assert r[2][1] == REFILL
    assert r[3][:2] == (FILL, PENDING) and r[3][3] == 2
    assert r[4][1:3] == (OFF, 2)
    assert r[5][0] == TODAY and r[6][0] == TODAY and r[6][7] == 2 and r[6][4] == 0
    assert r[7][:2] == (TODAY, SEEN) and r[8][0] == FILL          # another key starts afresh
    # a refill that fits is served
    r = exerciser("launch 0", "launch 0", "verify 0", "launch 0", "verify 1", "launch 0")
    assert r[5][0] == REPLAY and r[5][3:] == (2, 1, 0, 1, 0)


def test_fill_that_cannot_be_enqueued(exerciser):
    r = exerciser("launch 0", "launch 0", "failed 1", "launch 0", "launch 0")
    assert r[2][1:4] == (OFF, 1, 0) and r[2][7] == 1              # the fill is not counted, the launch is
    assert r[3][0] == TODAY and r[4][0] == TODAY and r[4][7] == 3 and r[4][4] == 0


def test_reset_forgets_the_key(exerciser):
    r = exerciser("launch 0", "launch 0", "verify 1", "reset", "launch 0", "launch 0")
    assert r[3][1] == NONE and r[3][5] == 1
    assert r[4][0] == TODAY and r[5][0] == FILL


def test_every_word_of_the_key_is_compared(exerciser):
    n = exerciser("words")[0][0]
    assert n == 27
    r = exerciser(*["same 0 %d" % (k + 1) for k in range(n)], "same 0 0", "same 5 5")
    assert [x[0] for x in r] == [0] * n + [1, 1]


def test_fields_that_cannot_matter_are_cleared(exerciser):
    # use_lens, distortion bits, nudge_ulps, nudge_seed, volumetrics
    assert exerciser("canon 0 1042536202 0 77 1")[0] == (0, 0, 0, 0, 1)
    assert exerciser("canon 255 1042536202 3 77 5")[0] == (1, 1042536202, 3, 77, 1)


def test_capacity_rule(exerciser):
    in_b, out_b = 10368, 8256        # kBlockBytes = 8 x 1280 + 8 x 8 + 64, kOutBlockBytes = 8 x 1024 + 8 x 8
    # the 4K bench frame: 448 B per ray of rows
    wanted, fit = exerciser("blocks 8294400 %d 0 %d 240000000 %d" % (in_b, 8 << 30, in_b + out_b))[0]
    assert wanted == 8294400 * 448 // in_b and fit == wanted
    # a small frame takes the minimum, eight times that when it has overflowed once
    assert exerciser("blocks 2257 %d 0 %d 100000 %d" % (in_b, 8 << 30, in_b + out_b))[0] == (16384, 16384)
    assert exerciser("blocks 2257 %d 1 %d 100000 %d" % (in_b, 8 << 30, in_b + out_b))[0] == (131072, 131072)
    # the budget cuts it down; below 1024 blocks there is no cache
    w, f = exerciser("blocks 2257 %d 0 %d 100000 %d" % (in_b, 100000 + 5000 * (in_b + out_b), in_b + out_b))[0]
    assert (w, f) == (16384, 5000)
    assert exerciser("blocks 2257 %d 0 %d 100000 %d" % (in_b, 100000 + 1000 * (in_b + out_b), in_b + out_b))[0][1] == 0
    assert exerciser("blocks 2257 %d 0 %d 100000 %d" % (in_b, 1 << 10, in_b + out_b))[0][1] == 0


def test_library_exports_the_cache_entry_points():
    from relativisticraytracer_amd import _lib
    lib = _lib.load()
    for name in ("rrt_march_cache_configure", "rrt_march_cache_stats", "rrt_march_cache_release"):
        assert hasattr(lib, name), name
    assert C.sizeof(_lib.rrt_march_cache_info) == 80
    assert lib.rrt_march_cache_stats(0, None) != 0                 # NULL out: invalid argument, before any device call
