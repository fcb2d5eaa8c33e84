"""The launch geometry of the two post passes, restated for the tests: the constants are read out of csrc/rrt_glow.h and
csrc/rrt_exposure.h as text, glow_seg and exposure_meter_groups are written again in a few lines.  tests/test_gpu_glow.py and
tests/test_gpu_exposure.py place their inputs with it (spikes at the segment seams); tests/test_post_pass_geometry.py asserts, without
a GPU, that their cases still reach the branches they are there for.  No GPU, no library: plain Python."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "relativisticraytracer_amd", "csrc")


def constants(header, names):
    """{name: int} of a header's integer constants (`kName = <product of literals and other constants>`, found by regex)"""
    text = open(os.path.join(CSRC, header)).read()

    def value(name):
        m = re.search(r"\b%s\s*=\s*([\w\s*]+?)\s*[,;]" % re.escape(name), text)
        assert m, f"{header} no longer defines {name} as a product of integers"
        v = 1
        for f in m.group(1).split("*"):
            f = f.strip()
            v *= int(f) if f.isdigit() else value(f)
        return v

    return {n: value(n) for n in names}


GLOW = constants("rrt_glow.h", ("kGlowHThreads", "kGlowM", "kGlowLdsBytes", "kGlowWeightChunk", "kGlowMaxRadius"))
METER = constants("rrt_exposure.h", ("kMeterThreads", "kMeterRun", "kMeterCUs", "kMeterGroupsPerCU"))


def glow_hpass_lds(seg, rmax):
    """bytes of LDS a segment of `seg` outputs and its halo take (rrt_glow.h: glow_hpass_lds)"""
    n = seg + 2 * rmax
    return (n + n // GLOW["kGlowM"] + 1) * 16


def glow_seg(rmax):
    """glow_hpass' outputs per segment (rrt_glow.h: glow_seg)"""
    seg = GLOW["kGlowHThreads"] * GLOW["kGlowM"]
    while seg > GLOW["kGlowM"] and glow_hpass_lds(seg, rmax) > GLOW["kGlowLdsBytes"]:
        seg //= 2
    return seg


def glow_segments(width, rmax):
    """(seg, [each segment's width]) of a row"""
    seg = glow_seg(rmax)
    return seg, [min(seg, width - x0) for x0 in range(0, width, seg)]


def glow_seams(width, rmax):
    """the columns on both sides of every segment boundary, and the last column"""
    seg, widths = glow_segments(width, rmax)
    cols = []
    for k in range(1, len(widths)):
        cols += [k * seg - 1, k * seg]
    return sorted(set(cols + [width - 1]))


def glow_chunks(radii):
    """[count of each glow_load_weights launch] for lobes of these radii"""
    n, c = sum(2 * r + 1 for r in radii), GLOW["kGlowWeightChunk"]
    return [min(c, n - off) for off in range(0, n, c)]


def meter_groups(n):
    """exposure_meter's grid for n pixels (rrt_exposure.h: exposure_meter_groups)"""
    per_group = METER["kMeterThreads"] * METER["kMeterRun"]
    return min((n + per_group - 1) // per_group, METER["kMeterCUs"] * METER["kMeterGroupsPerCU"])


def meter_rounds(n):
    """what exposure_meter's `base += stride` loop does on n pixels: (rounds, waves that take the last round, workgroups of which only
    some waves take it, pixels inside the frame of the last wave's last run, past-the-end lanes of that run)"""
    run = 64 * METER["kMeterRun"]                       # a wave's pixels per round
    waves_per_group = METER["kMeterThreads"] // 64
    groups = meter_groups(n)
    stride = groups * waves_per_group * run
    rounds = (n + stride - 1) // stride
    left = n - (rounds - 1) * stride                    # the last round's pixels, from wave 0 upwards
    waves = min((left + run - 1) // run, groups * waves_per_group)
    split = 1 if waves % waves_per_group else 0
    live = left - (waves - 1) * run
    return rounds, waves, split, live, run - live
