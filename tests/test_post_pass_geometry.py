"""The glow's and the exposure meter's launch geometry switches at sizes every production frame crosses: glow_hpass cuts a row into
segments of 2048 outputs (1024 once the staged halo would pass 64 KiB of LDS), launch_glow sends the taps 960 floats a launch, and
exposure_meter's capped grid strides over frames of more than 2^20 pixels in rounds.  tests/test_gpu_glow.py and
tests/test_gpu_exposure.py run the kernels on the smallest frames that reach those branches.

COVERAGE IS A CONDITION: this file asserts, without a GPU, that every one of those cases still reaches what it is there for.  It
reads the constants out of the headers (tests/post_geometry.py), so a retuned constant fails here and names the case that stopped
covering its branch -- the GPU tests alone would go on passing while covering nothing."""
import math

import pytest

import post_geometry as pg
import test_gpu_exposure as te          # the case tables are read inside the tests: collecting this file needs none of them
import test_gpu_glow as tg

# what each glow case is there for: (outputs per segment, each segment's width, each glow_load_weights launch's count)
GLOW_REACHES = {
    "last_segment_one_pixel": (2048, [2048, 1], [74]),
    "three_segments_one_row": (2048, [2048, 2048, 1], [74]),
    "the_4k_row": (2048, [2048, 1792], [784]),
    "widest_2048_segment_halo": (2048, [2048, 1], [960, 847]),
    "first_1024_segment_radius": (1024, [1024, 1024, 1], [960, 849]),
    "maximum_radius_four_lobes": (1024, [1024, 76], [960, 960, 960, 960, 4]),
    "exactly_one_full_chunk": (2048, [70], [960]),
    "one_chunk_and_a_sliver": (2048, [70], [960, 1]),
}
# what each strided shape is there for: (rounds, waves that take the last round, whether a workgroup is split by it, pixels of the
# last wave's run inside the frame, past-the-end lanes of that run)
METER_REACHES = {
    (1024, 1024): (1, 4096, 0, 256, 0),
    (61681, 17): (2, 1, 1, 1, 255),
    (1049, 1000): (2, 2, 1, 168, 88),
    (1031, 1019): (2, 8, 0, 221, 35),
    (1920, 1080): (2, 4004, 0, 256, 0),
}


def test_the_constants_are_the_ones_the_cases_were_chosen_for():
    assert pg.GLOW == {"kGlowHThreads": 128, "kGlowM": 16, "kGlowLdsBytes": 65536, "kGlowWeightChunk": 960, "kGlowMaxRadius": 1024}
    assert pg.METER == {"kMeterThreads": 256, "kMeterRun": 4, "kMeterCUs": 256, "kMeterGroupsPerCU": 4}
    assert pg.glow_hpass_lds(2048, 903) == 65520 and pg.glow_hpass_lds(1024, 1024) == 52240
    assert [pg.glow_seg(r) for r in (1, 208, 903, 904, 1024)] == [2048, 2048, 2048, 1024, 1024]
    assert [pg.meter_groups(n) for n in (1, 1024, 1025, 60000, 1 << 20, (1 << 20) + 1, 3840 * 2160)] == [1, 1, 2, 59, 1024, 1024, 1024]


@pytest.mark.parametrize("name", list(GLOW_REACHES))
def test_glow_case_reaches_its_branch(name):
    """the planner's R (from the library's taps, on the host), the segment size, every segment's width, every weight launch's count"""
    import relativisticraytracer_amd as rrt
    w, h, lobes, radius, threshold, intensity, radii = tg.GEOMETRY_CASES[name]
    g = rrt.GlowSettings(lobes=lobes, radius=radius, threshold=threshold, intensity=intensity)
    got = tuple((rrt.glow_weights(g, h, l).size - 1) // 2 for l in range(lobes))
    assert got == radii, (name, got)
    assert radii == tuple(math.ceil(3.0 * (float(g.radius) * h) * 2 ** l) for l in range(lobes)), name   # float32(radius), in double
    seg, widths, chunks = GLOW_REACHES[name]
    assert pg.glow_segments(w, radii[-1]) == (seg, widths), (name, pg.glow_segments(w, radii[-1]))
    assert pg.glow_chunks(radii) == chunks, (name, pg.glow_chunks(radii))
    n_taps = sum(2 * r + 1 for r in radii)
    assert rrt.glow_scratch_bytes(w, h, g) == lobes * w * h * 16 + (n_taps * 4 + 15) // 16 * 16, name
    assert pg.glow_hpass_lds(seg, radii[-1]) <= pg.GLOW["kGlowLdsBytes"], name
    if seg < 2048:
        assert pg.glow_hpass_lds(2 * seg, radii[-1]) > pg.GLOW["kGlowLdsBytes"], name


def test_glow_cases_together_reach_every_branch():
    assert set(GLOW_REACHES) == set(tg.GEOMETRY_CASES)
    reach = {name: (pg.glow_segments(c[0], c[6][-1]), pg.glow_chunks(c[6]), c[6]) for name, c in tg.GEOMETRY_CASES.items()}
    segs = {name: r[0] for name, r in reach.items()}
    assert any(s == 2048 and len(ws) == 2 and ws[-1] == 1 for s, ws in segs.values())            # x0 = 2048, a segment of one pixel
    assert any(s == 2048 and len(ws) >= 3 for s, ws in segs.values())                             # a middle segment, both halos live
    assert any(s == 2048 and len(ws) >= 2 and ws[-1] % 64 == 0 and ws[-1] < s for s, ws in segs.values())   # whole waves, fewer
    assert any(s == 1024 and len(ws) >= 3 for s, ws in segs.values())                             # seg = 1024, a middle segment
    assert {903, 904, 1024} <= {r[2][-1] for r in reach.values()}                                 # both sides of the switch, the limit
    assert any(s == 1024 and len(r) > 1 and r[0] < r[-1] for (s, _), _, r in reach.values())      # rmax - r > 0 into the staged row
    counts = [r[1] for r in reach.values()]
    assert [960] in counts and [960, 1] in counts and any(len(c) >= 5 and c[-1] < 960 for c in counts)
    # none of it is reached by the cases from before: one segment, one weight launch
    for w, h, lobes, radius, _, _ in tg.CASES:
        radii = [math.ceil(3.0 * radius * h * 2 ** l) for l in range(lobes)]
        assert len(pg.glow_segments(w, radii[-1])[1]) == 1 and len(pg.glow_chunks(radii)) == 1 and radii[-1] < 904, (w, h)


def test_driver_case_reaches_two_segments():
    (mode, w, h, intensity, radius, lobes), = [c for c in tg.DRIVER_CASES if c[1] > 2048]
    assert (w, h) == (2064, 16) and intensity == 0.25
    rmax = math.ceil(3.0 * radius * h * 2 ** (lobes - 1))
    assert rmax >= 16 and pg.glow_segments(w, rmax) == (2048, [2048, 16])


@pytest.mark.parametrize("w,h", list(METER_REACHES), ids=[f"{w}x{h}" for w, h in METER_REACHES])
def test_meter_shape_reaches_its_rounds(w, h):
    assert (w, h) in te.STRIDED_SHAPES
    assert pg.meter_groups(w * h) == 1024
    assert pg.meter_rounds(w * h) == METER_REACHES[(w, h)], ((w, h), pg.meter_rounds(w * h))


def test_meter_shapes_together_reach_every_branch():
    STRIDED_SHAPES, RAGGED_SHAPES, VARIANT_SHAPE, SHAPES = te.STRIDED_SHAPES, te.RAGGED_SHAPES, te.VARIANT_SHAPE, te.SHAPES
    assert set(METER_REACHES) == set(STRIDED_SHAPES) and set(RAGGED_SHAPES) <= set(STRIDED_SHAPES) and VARIANT_SHAPE in STRIDED_SHAPES
    cap = pg.meter_groups(1 << 40) * pg.METER["kMeterThreads"] * pg.METER["kMeterRun"]
    assert cap == 1 << 20
    sizes = {w * h for w, h in STRIDED_SHAPES}
    assert {cap, cap + 1, 1920 * 1080} <= sizes
    reach = [pg.meter_rounds(n) for n in sizes]
    assert any(r[:2] == (2, 1) and r[3] == 1 for r in reach)                     # one wave, one lane inside the frame
    assert any(r[0] == 2 and r[1] > 1 and r[2] == 1 for r in reach)              # some waves of a workgroup and not the others
    assert any(r[0] == 2 and r[1] > 4 and 0 < r[4] < 64 for r in reach)          # a run whose last 64 lanes are partly inside
    for w, h in RAGGED_SHAPES + [VARIANT_SHAPE]:
        assert pg.meter_rounds(w * h)[0] == 2 and pg.meter_rounds(w * h)[4] > 0, (w, h)
    # none of it is reached by the shapes from before: one round, at most 59 workgroups
    assert all(pg.meter_rounds(w * h)[0] == 1 and pg.meter_groups(w * h) <= 59 for w, h in SHAPES)
