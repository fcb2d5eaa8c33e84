"""--png-deflate's refusals, worded alike by both headless drivers and decided before any GPU work: neither driver needs a GPU to
refuse.  (tests/test_driver_refusals.py pins the refusals that were there before.)"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BASE = ["--width", "16", "--height", "12", "--frames", "1"]
REFUSALS = [
    (["--png-deflate", "device"], "--png-deflate needs --png PATTERN"),
    (["--png-deflate", "host"], "--png-deflate needs --png PATTERN"),
    (["--png", "f.%04d.png", "--png-deflate", "gpu"], "--png-deflate host | device"),
    (["--png", "f.%04d.png", "--png-deflate", ""], "--png-deflate host | device"),
    (["--png", "f.%04d.png", "--png-deflate", "device", "--png-level", "4"], "--png-level is the host zlib's level: not with --png-deflate device"),
    (["--png", "f.%04d.png", "--png-level", "9", "--png-deflate", "device"], "--png-level is the host zlib's level: not with --png-deflate device"),
    # the refusals that were there come first, worded as before
    (["--png-depth", "8", "--png-deflate", "device"], "--png-depth / --png-filter / --png-level need --png PATTERN"),
    (["--png", "f.%04d.png", "--png-level", "0", "--png-deflate", "device"], "--png-level 1 ... 9"),
]


def _run(driver, args, cwd):
    if driver == "cpp":
        from relativisticraytracer_amd import build
        cmd = [build.build_headless()]
    else:
        cmd = [sys.executable, "-m", "relativisticraytracer_amd.headless"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + BASE + args, cwd=cwd, capture_output=True, text=True, timeout=120, env=env)


@pytest.mark.parametrize("driver", ["py", "cpp"])
@pytest.mark.parametrize("args,message", REFUSALS)
def test_refusal(driver, args, message, tmp_path):
    r = _run(driver, args, str(tmp_path))
    assert r.returncode != 0 and r.stdout.strip() == ""
    assert message in r.stderr, r.stderr[-1000:]
    assert os.listdir(tmp_path) == []                   # nothing was written


def test_host_is_the_default_and_parses(tmp_path):
    """--png-deflate host is today's path: the option alone changes nothing that check_args leaves behind"""
    from relativisticraytracer_amd import headless
    ap = headless.build_parser()
    base = BASE + ["--png", "f.%04d.png"]
    plain, host, device = (ap.parse_args(base + extra) for extra in ([], ["--png-deflate", "host"], ["--png-deflate", "device"]))
    for a in (plain, host, device):
        headless.check_args(ap, a, 1)
    assert plain.png_format == host.png_format == device.png_format == (8, "adaptive", 4)
    assert (plain.png_on_device, host.png_on_device, device.png_on_device) == (False, False, True)
