"""What both headless drivers refuse, in one table (no GPU needed: every refusal here happens before a device is touched).

A row is (driver, argv, env, expected).  Both drivers exit with status 2.  rrt_headless writes the refusal, and nothing else, to stderr;
headless.py ends its stderr, after argparse's usage block, with `relativisticraytracer_amd.headless: error: ` and the refusal.  `expected`
is that whole text.  Where argparse itself words the refusal (`invalid choice`, `expected one argument`, a `type=` function's message
behind `argument --x: `) the row is ArgparseSays(a part of the last line): that wording belongs to the Python version.

The rows are grouped by feature.  A feature's rows run under the test names they have always had, in that feature's host module
(tests/test_*_host.py), through `rows` and `refused` below; the parser's quirks run here."""
import collections
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CPP, PY = "rrt_headless", "headless.py"
TWO_RANKS = {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}
ArgparseSays = collections.namedtuple("ArgparseSays", "part")

FOV_RANGE = "--fov DEG in (0, 360], --vfov DEG in (0, 180]"
GLOW_VALUES = "--glow INTENSITY >= 0, --glow-radius R > 0 (a fraction of the height; widest lobe <= 1024 px), --glow-threshold T >= 0"
STEREO_VALUES = "--stereo-base B >= 0, --convergence Z >= 0, --pole-merge FROM TO with 0 <= FROM <= TO <= 90"
STEREO_NEEDED = "--stereo-base / --convergence / --pole-merge need --stereo top-bottom | side-by-side"
EXPOSURE_VALUES = "--auto-exposure KEY > 0, --exposure-speed UP DOWN >= 0 (seconds), --exposure-range MIN MAX with MIN <= MAX, --exposure-percentiles LOW HIGH >= 0 with LOW + HIGH < 1000"
EXPOSURE_NEEDED = "--exposure-speed / --exposure-range / --exposure-percentiles need --exposure EV | --auto-exposure [KEY]"
DOF_APERTURE = "--dof APERTURE: the lens radius in scene units, >= 0"
DOF_PINHOLE = "--dof: a thin lens in front of a pinhole camera, not with --projection equirect | fisheye"
DOF_NEEDED = "--focus / --dof-samples need --dof APERTURE"
ADAPTIVE_NEEDS_SS = "--adaptive needs --supersample 2 | 4 | 8"
PANO_ONE_INSTANT = "a panorama renders one instant per frame (--motion-blur 1)"

ROWS = {
    "lens": [
        (PY, ["--dof", "0.3", "--projection", "equirect"], None, DOF_PINHOLE),
        (PY, ["--dof", "0.3", "--projection", "fisheye"], None, DOF_PINHOLE),
        (PY, ["--dof", "0.3", "--stereo", "side-by-side"], None, "--dof: not with --stereo"),
        (PY, ["--dof", "0.3", "--supersample", "2", "--adaptive"], None, "--dof: not with --adaptive"),
        (PY, ["--dof", "0.3", "--motion-blur", "4", "--dof-samples", "8"], None, "--dof-samples: with --motion-blur M > 1 the lens samples are the shutter's sub-frames (K = M)"),
        (PY, ["--focus", "12"], None, DOF_NEEDED),
        (PY, ["--dof-samples", "4"], None, DOF_NEEDED),
        (PY, ["--dof", "-0.3"], None, DOF_APERTURE),
        (PY, ["--dof", "nan"], None, DOF_APERTURE),
        (PY, ["--dof", "0.3", "--focus", "0"], None, ArgparseSays("a distance > 0 along forward, or `hole`")),
        (PY, ["--dof", "0.3", "--focus", "-2"], None, ArgparseSays("a distance > 0 along forward, or `hole`")),
        (PY, ["--dof", "0.3", "--focus", "inf"], None, ArgparseSays("a distance > 0 along forward, or `hole`")),
        (PY, ["--dof", "0.3", "--focus", "ring"], None, ArgparseSays("a distance > 0 along forward, or `hole`")),
        (PY, ["--dof", "0.3", "--dof-samples", "3"], None, ArgparseSays("--dof-samples")),
        (CPP, ["--dof", "0.3", "--projection", "equirect"], None, "usage: " + DOF_PINHOLE),
        (CPP, ["--dof", "0.3", "--projection", "fisheye"], None, "usage: " + DOF_PINHOLE),
        (CPP, ["--dof", "0.3", "--stereo", "side-by-side"], None, "usage: --dof: not with --stereo"),
        (CPP, ["--dof", "0.3", "--supersample", "2", "--adaptive"], None, "usage: --dof: not with --adaptive"),
        (CPP, ["--dof", "0.3", "--motion-blur", "4", "--dof-samples", "8"], None, "usage: --dof-samples: with --motion-blur M > 1 the lens samples are the shutter's sub-frames (K = M)"),
        (CPP, ["--focus", "12"], None, "usage: " + DOF_NEEDED),
        (CPP, ["--dof-samples", "4"], None, "usage: " + DOF_NEEDED),
        (CPP, ["--dof", "-0.3"], None, "usage: " + DOF_APERTURE),
        (CPP, ["--dof", "nan"], None, "usage: " + DOF_APERTURE),
        (CPP, ["--dof", "0.3", "--focus", "0"], None, "usage: --focus: a distance > 0 along forward, or `hole`"),
        (CPP, ["--dof", "0.3", "--focus", "-2"], None, "usage: --focus: a distance > 0 along forward, or `hole`"),
        (CPP, ["--dof", "0.3", "--focus", "inf"], None, "usage: --focus: a distance > 0 along forward, or `hole`"),
        (CPP, ["--dof", "0.3", "--focus", "ring"], None, "usage: --focus: a distance > 0 along forward, or `hole`"),
        (CPP, ["--dof", "0.3", "--dof-samples", "3"], None, "usage: --dof-samples 1 | 2 | 4 | 8 | 16 (lens samples per sub-sample)"),
        (CPP, ["--dof"], None, "usage: " + DOF_APERTURE),
        (CPP, ["--dof", "wide"], None, "usage: " + DOF_APERTURE),
    ],
    "stereo": [
        (PY, ["--stereo", "top-bottom", "--projection", "fisheye"], None, "--stereo: pinhole or equirect (no stereo fisheye domes)"),
        (PY, ["--stereo", "side-by-side", "--motion-blur", "4"], None, "--stereo renders one instant per frame (--motion-blur 1)"),
        (PY, ["--stereo", "top-bottom", "--glow", "0.25"], None, "--stereo: not with --glow"),
        (PY, ["--stereo-base", "0.5"], None, STEREO_NEEDED),
        (PY, ["--convergence", "10"], None, STEREO_NEEDED),
        (PY, ["--pole-merge", "60", "80", "--projection", "equirect"], None, STEREO_NEEDED),
        (PY, ["--stereo", "top-bottom", "--projection", "equirect", "--convergence", "10"], None, "--convergence: pinhole only"),
        (PY, ["--stereo", "top-bottom", "--pole-merge", "60", "80"], None, "--pole-merge: equirect only"),
        (PY, ["--stereo", "top-bottom", "--stereo-base", "-1"], None, STEREO_VALUES),
        (PY, ["--stereo", "side-by-side", "--stereo-base", "nan"], None, STEREO_VALUES),
        (PY, ["--stereo", "side-by-side", "--convergence", "-3"], None, STEREO_VALUES),
        (PY, ["--stereo", "top-bottom", "--projection", "equirect", "--pole-merge", "70", "60"], None, STEREO_VALUES),
        (PY, ["--stereo", "top-bottom", "--projection", "equirect", "--pole-merge", "60", "95"], None, STEREO_VALUES),
        (CPP, ["--stereo", "top-bottom", "--projection", "fisheye"], None, "usage: --stereo: pinhole or equirect (no stereo fisheye domes)"),
        (CPP, ["--stereo", "side-by-side", "--motion-blur", "4"], None, "usage: --stereo renders one instant per frame (--motion-blur 1)"),
        (CPP, ["--stereo", "top-bottom", "--glow", "0.25"], None, "usage: --stereo: not with --glow"),
        (CPP, ["--stereo-base", "0.5"], None, "usage: " + STEREO_NEEDED),
        (CPP, ["--convergence", "10"], None, "usage: " + STEREO_NEEDED),
        (CPP, ["--pole-merge", "60", "80", "--projection", "equirect"], None, "usage: " + STEREO_NEEDED),
        (CPP, ["--stereo", "top-bottom", "--projection", "equirect", "--convergence", "10"], None, "usage: --convergence: pinhole only"),
        (CPP, ["--stereo", "top-bottom", "--pole-merge", "60", "80"], None, "usage: --pole-merge: equirect only"),
        (CPP, ["--stereo", "top-bottom", "--stereo-base", "-1"], None, "usage: " + STEREO_VALUES),
        (CPP, ["--stereo", "side-by-side", "--stereo-base", "nan"], None, "usage: " + STEREO_VALUES),
        (CPP, ["--stereo", "side-by-side", "--convergence", "-3"], None, "usage: " + STEREO_VALUES),
        (CPP, ["--stereo", "top-bottom", "--projection", "equirect", "--pole-merge", "70", "60"], None, "usage: " + STEREO_VALUES),
        (CPP, ["--stereo", "top-bottom", "--projection", "equirect", "--pole-merge", "60", "95"], None, "usage: " + STEREO_VALUES),
        (CPP, ["--stereo", "left-right"], None, "usage: --stereo top-bottom | side-by-side"),
        (CPP, ["--stereo", "top-bottom", "--stereo-base", "wide"], None, "usage: --stereo-base: a number"),
    ],
    "stereo-layout": [
        (PY, ["--stereo", "left-right"], None, ArgparseSays("--stereo")),
    ],
    "exposure": [
        (PY, ["--exposure-speed", "0.2", "1.0"], None, EXPOSURE_NEEDED),
        (PY, ["--exposure-range", "-4", "4"], None, EXPOSURE_NEEDED),
        (PY, ["--exposure-percentiles", "400", "20"], None, EXPOSURE_NEEDED),
        (PY, ["--auto-exposure", "0"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--auto-exposure", "-0.5"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--auto-exposure", "--exposure-speed", "-1", "1"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--auto-exposure", "--exposure-range", "2", "1"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--auto-exposure", "--exposure-percentiles", "600", "400"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--auto-exposure", "--exposure-percentiles", "-1", "20"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--exposure", "nan"], None, "--exposure EV finite, " + EXPOSURE_VALUES),
        (PY, ["--exposure"], None, ArgparseSays("--exposure")),
        (PY, ["--exposure", "bright"], None, ArgparseSays("--exposure")),
        (PY, ["--auto-exposure", "--exposure-percentiles", "1.5", "2"], None, ArgparseSays("--exposure-percentiles")),
        (PY, ["--exposure", "1"], TWO_RANKS, "--exposure / --auto-exposure: one GPU only (WORLD_SIZE > 1)"),
        (PY, ["--auto-exposure"], TWO_RANKS, "--exposure / --auto-exposure: one GPU only (WORLD_SIZE > 1)"),
        (PY, ["--auto-exposure", "0.18", "--glow", "0.25"], TWO_RANKS, "--glow: one GPU only (WORLD_SIZE > 1)"),
        (CPP, ["--exposure-speed", "0.2", "1.0"], None, "usage: " + EXPOSURE_NEEDED),
        (CPP, ["--exposure-range", "-4", "4"], None, "usage: " + EXPOSURE_NEEDED),
        (CPP, ["--exposure-percentiles", "400", "20"], None, "usage: " + EXPOSURE_NEEDED),
        (CPP, ["--auto-exposure", "0"], None, "usage: " + EXPOSURE_VALUES),
        (CPP, ["--auto-exposure", "-0.5"], None, "usage: " + EXPOSURE_VALUES),
        (CPP, ["--auto-exposure", "--exposure-speed", "-1", "1"], None, "usage: " + EXPOSURE_VALUES),
        (CPP, ["--auto-exposure", "--exposure-range", "2", "1"], None, "usage: " + EXPOSURE_VALUES),
        (CPP, ["--auto-exposure", "--exposure-percentiles", "600", "400"], None, "usage: " + EXPOSURE_VALUES),
        (CPP, ["--auto-exposure", "--exposure-percentiles", "-1", "20"], None, "usage: " + EXPOSURE_VALUES),
        (CPP, ["--exposure", "nan"], None, "usage: --exposure: a number"),
        (CPP, ["--exposure"], None, "usage: --exposure: a number"),
        (CPP, ["--exposure", "bright"], None, "usage: --exposure: a number"),
        (CPP, ["--auto-exposure", "--exposure-percentiles", "1.5", "2"], None, "usage: --exposure-percentiles LOW HIGH: whole numbers in per mille"),
        (CPP, ["--auto-exposure", "--exposure-speed", "1"], None, "usage: --exposure-speed: two numbers"),
        (CPP, ["--exposure", "1", "--gpus", "2"], None, "usage: --exposure / --auto-exposure: one GPU only (--gpus 1)"),
        (CPP, ["--auto-exposure", "--gpus", "2"], None, "usage: --exposure / --auto-exposure: one GPU only (--gpus 1)"),
        (CPP, ["--auto-exposure", "0.18", "--glow", "0.25", "--gpus", "2"], None, "rrt_headless: --glow renders on one GPU only (--gpus 1)"),
        (CPP, ["--exposure", "1", "--force-collective"], None, "usage: --exposure / --auto-exposure: one GPU only (--gpus 1)"),
    ],
    "glow": [
        (PY, ["--glow", "-1"], None, GLOW_VALUES),
        (PY, ["--glow", "0.5", "--glow-lobes", "5"], None, ArgparseSays("--glow")),
        (PY, ["--glow", "0.5", "--glow-radius", "0"], None, GLOW_VALUES),
        (PY, ["--glow", "0.5", "--glow-threshold", "-1"], None, GLOW_VALUES),
        (PY, ["--glow", "0.5", "--glow-radius", "0.5"], None, GLOW_VALUES),
        (PY, ["--glow", "nan"], None, GLOW_VALUES),
        (PY, ["--glow", "x"], None, ArgparseSays("--glow")),
        (PY, ["--glow", "0.5"], TWO_RANKS, "--glow: one GPU only (WORLD_SIZE > 1)"),
        (CPP, ["--glow", "-1"], None, GLOW_VALUES + ", --glow-lobes 1 | 2 | 3 | 4"),
        (CPP, ["--glow", "0.5", "--glow-lobes", "5"], None, GLOW_VALUES + ", --glow-lobes 1 | 2 | 3 | 4"),
        (CPP, ["--glow", "0.5", "--glow-lobes", "2.5"], None, "--glow-lobes 1 | 2 | 3 | 4"),
        (CPP, ["--glow", "0.5", "--glow-radius", "0"], None, GLOW_VALUES + ", --glow-lobes 1 | 2 | 3 | 4"),
        (CPP, ["--glow", "0.5", "--glow-radius", "0.5"], None, GLOW_VALUES + ", --glow-lobes 1 | 2 | 3 | 4"),
        (CPP, ["--glow", "0.5", "--glow-threshold", "-1"], None, GLOW_VALUES + ", --glow-lobes 1 | 2 | 3 | 4"),
        (CPP, ["--glow", "nan"], None, "--glow: a number"),
        (CPP, ["--glow"], None, "--glow: a number"),
        (CPP, ["--glow", "0.5", "--gpus", "2"], None, "rrt_headless: --glow renders on one GPU only (--gpus 1)"),
        (CPP, ["--glow", "0.5", "--force-collective"], None, "rrt_headless: --glow renders on one GPU only (--gpus 1)"),
    ],
    "adaptive": [
        (PY, ["--adaptive"], None, ADAPTIVE_NEEDS_SS),
        (PY, ["--adaptive", "8"], None, ADAPTIVE_NEEDS_SS),
        (PY, ["--adaptive", "--supersample", "1"], None, ADAPTIVE_NEEDS_SS),
        (PY, ["--supersample", "2", "--adaptive", "8", "--motion-blur", "2"], None, "--adaptive renders one instant per frame (--motion-blur 1)"),
        (PY, ["--supersample", "2", "--adaptive", "--stereo", "top-bottom"], None, "--adaptive: not with --stereo"),
        (PY, ["--supersample", "2", "--adaptive", "eight"], None, ArgparseSays("a threshold in 0 ... 255")),
        (PY, ["--supersample", "2", "--adaptive", "8.5"], None, ArgparseSays("a threshold in 0 ... 255")),
        (PY, ["--supersample", "2", "--adaptive", "256"], None, ArgparseSays("a threshold in 0 ... 255")),
        (PY, ["--supersample", "2", "--adaptive", "-1"], None, ArgparseSays("a threshold in 0 ... 255")),
        (PY, ["--supersample", "2", "--adaptive"], TWO_RANKS, "--adaptive: one GPU only (WORLD_SIZE > 1)"),
        (CPP, ["--adaptive"], None, "usage: " + ADAPTIVE_NEEDS_SS),
        (CPP, ["--adaptive", "8"], None, "usage: " + ADAPTIVE_NEEDS_SS),
        (CPP, ["--adaptive", "--supersample", "1"], None, "usage: " + ADAPTIVE_NEEDS_SS),
        (CPP, ["--supersample", "2", "--adaptive", "8", "--motion-blur", "2"], None, "usage: --adaptive renders one instant per frame (--motion-blur 1)"),
        (CPP, ["--supersample", "2", "--adaptive", "--stereo", "top-bottom"], None, "usage: --adaptive: not with --stereo"),
        (CPP, ["--supersample", "2", "--adaptive", "eight"], None, "usage: --adaptive [T]: a threshold in 0 ... 255 (default 8)"),
        (CPP, ["--supersample", "2", "--adaptive", "8.5"], None, "usage: --adaptive [T]: a threshold in 0 ... 255 (default 8)"),
        (CPP, ["--supersample", "2", "--adaptive", "256"], None, "usage: --adaptive [T]: a threshold in 0 ... 255 (default 8)"),
        (CPP, ["--supersample", "2", "--adaptive", "-1"], None, "usage: --adaptive [T]: a threshold in 0 ... 255 (default 8)"),
        (CPP, ["--supersample", "2", "--adaptive", "--gpus", "2"], None, "usage: --adaptive renders on one GPU only (--gpus 1)"),
    ],
    "projection": [
        (PY, ["--projection", "equirect", "--fov", "400"], None, FOV_RANGE),
        (PY, ["--projection", "equirect", "--vfov", "181"], None, FOV_RANGE),
        (PY, ["--projection", "equirect", "--fov", "nan"], None, FOV_RANGE),
        (PY, ["--projection", "fisheye", "--fov", "-5"], None, FOV_RANGE),
        (PY, ["--projection", "fisheye", "--fov", "0"], None, FOV_RANGE),
        (PY, ["--projection", "fisheye", "--vfov", "90"], None, "--vfov: equirect only (a fisheye's aperture is --fov)"),
        (PY, ["--fov", "90"], None, "--fov / --vfov need --projection equirect | fisheye"),
        (PY, ["--projection", "equirect", "--motion-blur", "4"], None, PANO_ONE_INSTANT),
        (PY, ["--projection", "fisheye", "--motion-blur", "2"], None, PANO_ONE_INSTANT),
        (PY, ["--projection", "equirect", "--glow", "0.25"], None, "--glow clamps at the frame's edge and an equirect frame wraps: not with --projection equirect"),
        (CPP, ["--projection", "equirect", "--fov", "400"], None, FOV_RANGE),
        (CPP, ["--projection", "equirect", "--vfov", "181"], None, FOV_RANGE),
        (CPP, ["--projection", "equirect", "--fov", "nan"], None, FOV_RANGE),
        (CPP, ["--projection", "fisheye", "--fov", "-5"], None, FOV_RANGE),
        (CPP, ["--projection", "fisheye", "--fov", "0"], None, FOV_RANGE),
        (CPP, ["--projection", "fisheye", "--vfov", "90"], None, "--vfov: equirect only (a fisheye's aperture is --fov)"),
        (CPP, ["--fov", "90"], None, "--fov / --vfov need --projection equirect | fisheye"),
        (CPP, ["--projection", "equirect", "--motion-blur", "4"], None, "rrt_headless: " + PANO_ONE_INSTANT),
        (CPP, ["--projection", "fisheye", "--motion-blur", "2"], None, "rrt_headless: " + PANO_ONE_INSTANT),
        (CPP, ["--projection", "equirect", "--glow", "0.25"], None, "rrt_headless: --glow clamps at the frame's edge and an equirect frame wraps: not with --projection equirect"),
        (CPP, ["--projection", "cubemap"], None, "--projection pinhole | equirect | fisheye"),
        (CPP, ["--projection", "fisheye", "--fov", "wide"], None, "--fov DEG: a number of degrees"),
    ],
    "projection-kind": [
        (PY, ["--projection", "cubemap"], None, ArgparseSays("--projection")),
    ],
    "motion-blur": [
        (PY, ["--motion-blur", "3"], None, ArgparseSays("--motion-blur")),
        (PY, ["--shutter", "1.5"], None, "--shutter: a fraction of the frame interval in [0, 1]"),
        (PY, ["--shutter", "-0.1"], None, "--shutter: a fraction of the frame interval in [0, 1]"),
        (CPP, ["--motion-blur", "3"], None, "--motion-blur 1 | 2 | 4 | 8 | 16 (sub-frames per frame)"),
        (CPP, ["--motion-blur"], None, "--motion-blur 1 | 2 | 4 | 8 | 16 (sub-frames per frame)"),
        (CPP, ["--shutter", "1.5"], None, "--shutter F: a fraction of the frame interval in [0, 1]"),
        (CPP, ["--shutter", "x"], None, "--shutter F: a fraction of the frame interval in [0, 1]"),
        (CPP, ["--shutter", "nan"], None, "--shutter F: a fraction of the frame interval in [0, 1]"),
    ],
    "supersample": [
        (PY, ["--supersample", "3"], None, ArgparseSays("--supersample")),
        (CPP, ["--supersample", "3"], None, "--supersample 1 | 2 | 4 | 8 (sub-samples per pixel along each axis)"),
        (CPP, ["--supersample", "two"], None, "--supersample 1 | 2 | 4 | 8 (sub-samples per pixel along each axis)"),
        (CPP, ["--supersample"], None, "--supersample 1 | 2 | 4 | 8 (sub-samples per pixel along each axis)"),
    ],
    "quirks": [
        (CPP, ["--spin"], None, "unknown argument --spin"),
        (CPP, ["--bogus"], None, "unknown argument --bogus"),
        (CPP, ["--width", "0"], None, "bad arguments"),
        (CPP, ["--fov", "0"], None, FOV_RANGE),
        (CPP, ["--path-policy", "x"], None, "--path-policy auto | single | three-pass"),
    ],
}
IDS = dict(ids=lambda a: " ".join(a) if isinstance(a, list) else "")      # a test's id: its command line


def rows(group, driver, env=None):
    """[(argv, expected)] of a group's rows for one driver, single-rank (env None) or TWO_RANKS, in the table's order"""
    return [(argv, expected) for d, argv, e, expected in ROWS[group] if d == driver and e == env]


def refused(driver, argv, expected, env=None):
    """runs the driver and asserts the refusal: exit status 2 and the whole message (ArgparseSays: a part of argparse's last line)"""
    if driver == CPP:
        from relativisticraytracer_amd import build
        cmd = [build.build_headless()]
    else:
        cmd = [sys.executable, "-m", "relativisticraytracer_amd.headless"]
    r = subprocess.run(cmd + argv, cwd=ROOT, env=dict(os.environ, **(env or {})), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2, (r.returncode, r.stderr[-800:])
    if driver == CPP:
        assert r.stderr == expected + "\n"
        return
    last = r.stderr.splitlines()[-1]
    assert "usage: relativisticraytracer_amd.headless" in r.stderr, r.stderr[-800:]
    if isinstance(expected, ArgparseSays):
        assert last.startswith("relativisticraytracer_amd.headless: error: argument ") and expected.part in last, last
    else:
        assert last == "relativisticraytracer_amd.headless: error: " + expected


@pytest.mark.parametrize("args,expected", rows("quirks", CPP), **IDS)
def test_cpp_parser_quirks(args, expected):
    """a plain option without its value is an unknown argument, the validated ones and the range checks say their own message"""
    refused(CPP, args, expected)


def test_every_row_has_a_test():
    """the groups the host modules and this one run, and nothing else: a row added under a new key would run nowhere"""
    assert set(ROWS) == {"lens", "stereo", "stereo-layout", "exposure", "glow", "adaptive", "projection", "projection-kind",
                         "motion-blur", "supersample", "quirks"}
    assert sum(len(v) for v in ROWS.values()) == 171
