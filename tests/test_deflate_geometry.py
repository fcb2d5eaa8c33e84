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
