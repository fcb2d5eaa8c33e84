"""Helpers shared by the -m gpu tests: torch is only the device-memory plumbing."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def ctx(sky):
    """(rrt, a sky texture of the suite's sky): import it by name; module scope, so every module gets and destroys its own"""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    yield rrt, tex
    tex.destroy()


def _zeros(n, dtype):
    import torch
    return torch.zeros(n, dtype=dtype, device="cuda")


def _host(t, shape):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(shape)


def run_drivers(tmp_path, args, timeout=600):
    """rrt_headless and `python -m relativisticraytracer_amd.headless` with the same arguments, each writing its own file: both
    end with status 0 and the two files are byte-identical -> (the C++ driver's summary, headless.py's summary, the C++ file)"""
    from relativisticraytracer_amd import build
    metas, files = [], (tmp_path / "cpp.rgba", tmp_path / "py.rgba")
    for cmd, out in zip(([build.build_headless()], [sys.executable, "-m", "relativisticraytracer_amd.headless"]), files):
        r = subprocess.run(cmd + list(args) + ["--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, (out.name, r.stderr[-2000:])
        metas.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert files[0].read_bytes() == files[1].read_bytes()
    return metas[0], metas[1], files[0]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def unit(name, *args):
    """Call rrt_unit_<name> (include/rrt_test.h, librrt_hip_test.so) through the C ABI; tensors are passed as device pointers."""
    import torch
    from relativisticraytracer_amd import _lib
    lib = _lib.load_test()
    conv = []
    for a in args:
        if hasattr(a, "data_ptr"):
            conv.append(C.c_void_p(a.data_ptr()))
        elif a is None:
            conv.append(C.c_void_p(0))
        else:
            conv.append(a)
    conv.append(C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(getattr(lib, "rrt_unit_" + name)(*conv), "rrt_unit_" + name)


def render_gpu(w, h, spin, vol, cam, time, sky_tex, fx=None, debug=True, max_steps=2000, frac_bits=8, arith_mode=0,
               noise_table=0):
    """Full-frame render through rrt_launch_raymarch(_ex); returns numpy arrays."""
    import torch
    import relativisticraytracer_amd as rrt
    fx = fx or rrt.CameraEffects()
    prm = rrt.RenderParams(spin=spin, volumetrics=vol, max_steps=max_steps, sky_frac_bits=frac_bits,
                           arith_mode=arith_mode, noise_table=noise_table)
    out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    res = {}
    if debug:
        n = w * h
        bufs = dict(ldr=torch.zeros(n * 4, device="cuda"), hdr=torch.zeros(n * 4, device="cuda"),
                    steps=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    hit=torch.zeros(n, dtype=torch.int32, device="cuda"),
                    pos=torch.zeros(n * 3, device="cuda"), vel=torch.zeros(n * 3, device="cuda"),
                    rad=torch.zeros(n * 4, device="cuda"),
                    lut_oob=torch.zeros(1, dtype=torch.int32, device="cuda"))
        rrt.launch_raymarch_debug(out, w, h, time, cam, sky_tex, fx, prm, **bufs)
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in bufs.items()}
        res["ldr"] = res["ldr"].reshape(h, w, 4); res["hdr"] = res["hdr"].reshape(h, w, 4)
        res["pos"] = res["pos"].reshape(n, 3); res["vel"] = res["vel"].reshape(n, 3)
        res["rad"] = res["rad"].reshape(n, 4)
    else:
        rrt.launch_raymarch(out, w, h, time, cam, sky_tex, fx, prm)
        torch.cuda.synchronize()
    res["rgba8"] = out.cpu().numpy().reshape(h, w, 4)
    return res
