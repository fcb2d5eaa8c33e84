"""rrt_deflate_launch_geometry and rrt_deflate_plan without a GPU: the fixtures of tests/test_gpu_deflate.py still reach the branches
they are there for -- one segment and several, a last segment of one byte, more workgroups than one CU holds, the byte path at the
input's ends and the input that has no whole 16-byte word -- and the kernels' layout is the one DESIGN.md section 4 describes."""
import pytest

import deflate_ref as dr

LDS_PER_CU = 160 * 1024


def _rrt():
    import relativisticraytracer_amd as rrt
    return rrt


@pytest.fixture(scope="module")
def sizes():
    return {name: (data.size, stream_bytes) for name, (data, stream_bytes) in dr.synthetic_fixtures().items()}


def test_three_kernels_and_two_workgroups_per_cu():
    rrt = _rrt()
    g = rrt.deflate_launch_geometry(3840 * 3 * 2160 + 2160, 92 * 11521)                  # a 4K depth-8 payload in its 24 slices
    assert (g["segments"]["threads"], g["offsets"]["threads"], g["gather"]["threads"]) == (256, 256, 256)
    assert g["segments"]["grid"] == g["gather"]["grid"] == 23 * 33 + 16 == 775 and g["offsets"]["grid"] == 1
    assert 64 * 1024 < g["segments"]["lds_bytes"] <= LDS_PER_CU // 2                     # input, bit buffer, tables: two fit a CU, three do not
    assert g["offsets"]["lds_bytes"] == 1024 and g["gather"]["lds_bytes"] == 0
    assert (g["head_bytes"], g["tail_bytes"], g["wide_loads"]) == (0, (3840 * 3 * 2160 + 2160) % 16, (3840 * 3 * 2160 + 2160) // 16)
    plan = rrt.deflate_plan(3840 * 3 * 2160 + 2160, 92 * 11521)
    assert (plan["streams"], plan["segments"]) == (24, 775)
    assert plan["out_bound"] == 3840 * 3 * 2160 + 2160 + 10 * 775 and plan["scratch_bytes"] > plan["out_bound"]


CUS = 256                    # an MI355X: two workgroups of deflate_segments share a CU's LDS
FRAME_4K = (3840 * 3 * 2160 + 2160, 92 * 11521)


def _branches(rrt, n, stream_bytes):
    """what a launch of this cut asks of deflate_offsets and of the chip, from the plan and the header's constants alone"""
    from relativisticraytracer_amd import deflate
    plan = rrt.deflate_plan(n, stream_bytes)
    segments, streams = plan["segments"], plan["streams"]
    per_stream = -(-min(n, stream_bytes) // deflate.SEGMENT_BYTES)
    full = sum(b - a == deflate.SEGMENT_BYTES for segs in dr.cuts(n, stream_bytes) for a, b in segs)
    rounds = -(-segments // deflate.THREADS)
    out = set()
    if rounds >= 3:
        out.add("the carry is carried on: three rounds of the length table or more")
    if per_stream > 1:
        out.add("per_stream > 1")
    if per_stream > 1 and segments > deflate.THREADS:
        out.add("per_stream > 1 behind the first round")
    if segments % per_stream:
        out.add("a last stream with fewer segments")
    if any(g % per_stream for g in range(deflate.THREADS, segments, deflate.THREADS)):
        out.add("a round boundary inside a stream")
    if streams > deflate.THREADS:
        out.add("a second round of the size loop")
    if full > 2 * CUS:
        out.add("more full-size workgroups than the chip holds at once")
    return out, rounds, per_stream, full


def test_the_large_fixtures_reach_a_frames_branches():
    """tests/deflate_ref.py's large fixtures from their sizes alone (LARGE_CUTS: nothing is generated here)"""
    from relativisticraytracer_amd import deflate
    rrt = _rrt()
    want = {"three per stream": (181, 541, 3), "two per stream": (300, 599, 2), "frame cut": (17, 560, 34)}
    reached = set()
    for name, (stream_bytes, streams, last) in dr.LARGE_CUTS.items():
        n = stream_bytes * streams + last
        plan, g = rrt.deflate_plan(n, stream_bytes), rrt.deflate_launch_geometry(n, stream_bytes)
        branches, rounds, per_stream, full = _branches(rrt, n, stream_bytes)
        assert (plan["streams"], plan["segments"], per_stream) == want[name], name
        assert g["segments"]["grid"] == g["gather"]["grid"] == plan["segments"] and g["offsets"]["grid"] == 1, name
        assert g["segments"]["threads"] == g["offsets"]["threads"] == g["gather"]["threads"] == deflate.THREADS
        assert rounds == -(-plan["segments"] // deflate.THREADS) >= 3, name
        assert plan["segments"] % per_stream != 0, name                                   # the last stream is short
        assert plan["out_bound"] == n + 10 * plan["segments"]
        reached |= branches
        if name == "two per stream":
            assert plan["streams"] > deflate.THREADS and "a second round of the size loop" in branches
        if name == "three per stream":
            assert (deflate.THREADS % per_stream, 2 * deflate.THREADS % per_stream) == (1, 2)      # both round boundaries inside streams
        if name == "frame cut":
            assert full == 543 > CUS * (LDS_PER_CU // g["segments"]["lds_bytes"]) == 2 * CUS
    for name in dr.LARGE_SINGLE:
        assert rrt.deflate_launch_geometry(dr.SEGMENT, 1 << 20)["segments"]["grid"] == 1, name
    # the 4K frame: no fewer rounds than `frame cut`, and no branch the three do not reach
    plan = rrt.deflate_plan(*FRAME_4K)
    branches, rounds, per_stream, full = _branches(rrt, *FRAME_4K)
    assert (plan["streams"], plan["segments"], per_stream, plan["segments"] % per_stream) == (24, 775, 33, 16)
    assert rounds == 4 >= _branches(rrt, 17828971, dr.LARGE_CUTS["frame cut"][0])[1] == 3
    assert full > 2 * CUS and branches and branches <= reached, branches - reached
    # the longest loops of a full stored fragment: the slot copy's quads, and deflate_gather's destination words in rounds of a workgroup
    longest = deflate.SEGMENT_BYTES + 10
    assert (longest + 15) // 16 == 2049 and (15 + longest + 15) // 16 == 2050 and -(-2050 // deflate.THREADS) == 9


def test_the_fixtures_reach_their_branches(sizes):
    rrt = _rrt()
    grid = {name: rrt.deflate_launch_geometry(n, sb)["segments"]["grid"] for name, (n, sb) in sizes.items()}
    assert [grid[f"n={n}"] for n in (0, 1, 32767, 32768, 32769, 65541)] == [1, 1, 1, 1, 2, 3]
    assert grid["300 streams of 1 byte"] == 300 > 2 * (LDS_PER_CU // rrt.deflate_launch_geometry(300, 1)["segments"]["lds_bytes"])
    assert grid["runs at segment starts"] == len(dr.RUNS) and grid["run across the segment boundary"] == 2
    assert grid["last stream of 1 byte"] == 3 and grid["zeros"] == 3
    for name, (n, sb) in sizes.items():
        layout = dr.cuts(n, sb)
        plan = rrt.deflate_plan(n, sb)
        assert (plan["streams"], plan["segments"]) == (len(layout), sum(len(s) for s in layout)) and grid[name] == plan["segments"], name
    # off the grid: the first bytes up to the next 16-byte word, and the last ones behind the last whole word, go one by one
    n, sb = sizes["n=32769"]
    for shift in range(1, 16):
        g = rrt.deflate_launch_geometry(n, sb, 0x7f0000000000 + shift)
        assert (g["head_bytes"], g["tail_bytes"]) == (16 - shift, (shift + n) % 16) and g["wide_loads"] == (n - g["head_bytes"] - g["tail_bytes"]) // 16
        small = rrt.deflate_launch_geometry(3, 7, shift)                                 # no whole word: the byte path alone
        assert (small["head_bytes"], small["tail_bytes"], small["wide_loads"]) == (3, 0, 0)
    aligned = rrt.deflate_launch_geometry(n, sb, 0)
    assert (aligned["head_bytes"], aligned["tail_bytes"], aligned["wide_loads"]) == (0, 1, 2048)
