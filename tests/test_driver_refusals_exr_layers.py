"""--exr-layers' refusals, both headless drivers, the same wording: a table of its own (tests/test_driver_refusals.py's is closed),
same conventions.  No GPU: every refusal comes before a device is touched."""
import pytest

from test_driver_refusals import CPP, PY, refused

EXR = ["--exr", "f.%04d.exr"]
NEEDED = "--exr-layers needs --exr PATTERN"
LIST = "--exr-layers LIST: a comma-separated subset of steps,horizon,transmittance,emission,direction,position, or all"
TWICE = "--exr-layers LIST names a layer twice"
ONE_RAY = "--exr-layers stores per-ray data of the 1x pinhole frame: not with "
ROWS = [
    (["--exr-layers", "all"], NEEDED),
    (["--exr-layers", "nothing"], NEEDED),
    (EXR + ["--exr-layers", "depth"], LIST),
    (EXR + ["--exr-layers", "steps,"], LIST),
    (EXR + ["--exr-layers", ""], LIST),
    (EXR + ["--exr-layers", "all,steps"], LIST),
    (EXR + ["--exr-layers", "Steps"], LIST),
    (EXR + ["--exr-layers", "steps,horizon,steps"], TWICE),
    (EXR + ["--exr-layers", "direction,direction"], TWICE),
    (EXR + ["--exr-layers", "all", "--supersample", "2"], ONE_RAY + "--supersample > 1"),
    (EXR + ["--exr-layers", "steps", "--motion-blur", "4"], ONE_RAY + "--motion-blur > 1"),
    (EXR + ["--exr-layers", "all", "--dof", "0.05"], ONE_RAY + "--dof"),
    (EXR + ["--exr-layers", "direction", "--stereo", "top-bottom"], ONE_RAY + "--stereo"),
    (EXR + ["--exr-layers", "all", "--projection", "equirect"], ONE_RAY + "--projection equirect | fisheye"),
    (EXR + ["--exr-layers", "all", "--projection", "fisheye"], ONE_RAY + "--projection equirect | fisheye"),
    (EXR + ["--exr-layers", "all", "--supersample", "2", "--adaptive"], ONE_RAY + "--adaptive"),
    # --exr's own refusals come first, as they are
    (EXR + ["--exr-layers", "all", "--glow", "0.25"],
     "--exr reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow"),
]
ROW_IDS = dict(ids=lambda a: " ".join(a) if isinstance(a, list) else "")


@pytest.mark.parametrize("args,msg", ROWS, **ROW_IDS)
def test_python_driver_refuses(args, msg):
    refused(PY, args, msg)


@pytest.mark.parametrize("args,msg", ROWS, **ROW_IDS)
def test_cpp_driver_refuses(args, msg):
    refused(CPP, args, "usage: " + msg)
