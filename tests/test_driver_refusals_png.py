"""--png's refusals, by message, of both headless drivers: values off the lists, --png-* without --png, depth 16 with --glow or on two
ranks, patterns with no or two frame fields, and a name another output has.  A table of its own (tests/test_driver_refusals.py's is
closed), same conventions; neither driver touches a device before it refuses."""
import pytest

from test_driver_refusals import CPP, PY, TWO_RANKS, refused

NEEDED = "--png-depth / --png-filter / --png-level need --png PATTERN"
NO_GLOW = "--png-depth 16 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow"
NO_FIELD = "--png PATTERN needs a frame field (%04d) when --frames > 1: the frames would overwrite one another"
FILTERS = "--png-filter adaptive | none | sub | up | average | paeth"
PNG_ROWS = [
    (["--png-depth", "16"], None, NEEDED),
    (["--png-filter", "up"], None, NEEDED),
    (["--png-level", "6"], None, NEEDED),
    (["--png-depth", "12"], None, NEEDED),
    (["--png", "f.%04d.png", "--png-depth", "12"], None, "--png-depth 8 | 16"),
    (["--png", "f.%04d.png", "--png-depth", "eight"], None, "--png-depth 8 | 16"),
    (["--png", "f.%04d.png", "--png-filter", "best"], None, FILTERS),
    (["--png", "f.%04d.png", "--png-filter", "4"], None, FILTERS),
    (["--png", "f.%04d.png", "--png-level", "0"], None, "--png-level 1 ... 9"),
    (["--png", "f.%04d.png", "--png-level", "10"], None, "--png-level 1 ... 9"),
    (["--png", "f.%04d.png", "--png-level", "fast"], None, "--png-level 1 ... 9"),
    (["--png", "f.%04d.png", "--png-depth", "16", "--glow", "0.25"], None, NO_GLOW),
    (["--png", "f.%04d.png", "--png-depth", "16", "--exposure", "1", "--glow", "0.25"], None, NO_GLOW),
    (["--png", "f.png", "--frames", "2"], None, NO_FIELD),
    (["--png", "f.png"], None, NO_FIELD),                                   # --frames defaults to 24
    (["--png", "f.%d.%04d.png"], None, "--png PATTERN: one frame field (%d or %0Nd)"),
    (["--png", "f.%04d.png", "--frames", "3", "--out", "f.0003.png"], None, "--png and --out name the same file"),
    (["--png", "f.%04d.png", "--frames", "3", "--out", "./sub/../f.0001.png"], None, "--png and --out name the same file"),
    (["--png", "f.png", "--frames", "1", "--out", "f.png"], None, "--png and --out name the same file"),
    (["--png", "f.%d.y4m", "--frames", "12", "--y4m", "f.12.y4m"], None, "--png and --y4m name the same file"),
    (["--png", "f.%04d.img", "--frames", "2", "--exr", "f.%04d.img"], None, "--png and --exr name the same file"),
]
PY_ONLY = [(["--png", "f.%04d.png", "--png-depth", "16"], TWO_RANKS, "--png-depth 16: one GPU only (WORLD_SIZE > 1)")]
CPP_ONLY = [(["--png", "f.%04d.png", "--png-depth", "16", "--gpus", "2"], None, "--png-depth 16: one GPU only (--gpus 1)"),
            (["--png", "f.%04d.png", "--png-depth", "16", "--force-collective"], None, "--png-depth 16: one GPU only (--gpus 1)"),
            (["--png", "f.%04d.png", "--png-depth"], None, "--png-depth 8 | 16")]
ROW_IDS = dict(ids=lambda a: " ".join(a) if isinstance(a, list) else "")


@pytest.mark.parametrize("args,env,msg", PNG_ROWS + PY_ONLY, **ROW_IDS)
def test_python_driver_refuses(args, env, msg):
    refused(PY, args, msg, env)


@pytest.mark.parametrize("args,env,msg", PNG_ROWS + CPP_ONLY, **ROW_IDS)
def test_cpp_driver_refuses(args, env, msg):
    refused(CPP, args, "usage: " + msg, env)


def test_depth_8_is_not_refused_where_depth_16_is():
    """depth 8 converts the assembled RGBA8 frame: --glow and two ranks pass the options' checks (the parse, no device)"""
    from relativisticraytracer_amd import headless
    ap = headless.build_parser()
    for extra, world in ((["--glow", "0.25"], 1), ([], 2), (["--exposure", "1", "--supersample", "2"], 1)):
        args = ap.parse_args(["--png", "f.%04d.png"] + extra)
        headless.check_args(ap, args, world)
        assert args.png_format == (8, "adaptive", 4)
    args = ap.parse_args(["--png", "f.%04d.png", "--png-depth", "16", "--png-filter", "paeth", "--png-level", "9", "--auto-exposure"])
    headless.check_args(ap, args, 1)
    assert args.png_format == (16, "paeth", 9)
