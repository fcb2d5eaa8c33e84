"""HDR glow (rrt_launch_glow, include/rrt.h) against its numpy restatement (tests/glow_ref.py): synthetic HDR fields and real
supersampled / motion-blurred frames, RGBA8 byte for byte through the portable exp; the identities (intensity 0, a threshold
above every luma); side streams and graph capture; both headless drivers.  torch is only the device-memory plumbing."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import glow_ref
from test_gpu_motion_blur import moving_cameras, render_mb
from test_gpu_supersample import _host, _zeros, render_ss, scene, tone_map

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    yield rrt, tex
    tex.destroy()


def _device_hdr(hdr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(hdr, np.float32).ravel()).cuda()


def glow(rrt, d_hdr, w, h, g, stream=None):
    """rrt_launch_glow of a device HDR frame: RGBA8 (h, w, 4)"""
    import torch
    out = _zeros(h * w * 4, torch.uint8)
    scratch = torch.empty(rrt.glow_scratch_bytes(w, h, g), dtype=torch.uint8, device="cuda")
    rrt.launch_glow(out, d_hdr, w, h, g, scratch, stream=stream)
    if stream is not None:
        stream.synchronize()
    return _host(out, (h, w, 4))


def expected(po, rrt, hdr, g):
    h = hdr.shape[0]
    return tone_map(po, glow_ref.glow_hdr(hdr, glow_ref.lobe_taps(rrt, g, h), g.threshold, g.intensity))


def synthetic_hdr(rng, w, h):
    """a dim field with sparse bright spikes (some of them far above any threshold) and a few exact zeros"""
    hdr = rng.uniform(0.0, 1.2, (h, w, 4)).astype(np.float32)
    spikes = rng.random((h, w)) < 0.03
    hdr[spikes, :3] *= rng.uniform(5.0, 400.0, (int(spikes.sum()), 1)).astype(np.float32)
    hdr[rng.random((h, w)) < 0.02, :3] = 0.0
    hdr[..., 3] = 1.0
    return hdr


CASES = [  # (w, h, lobes, radius, threshold, intensity)
    (1, 1, 1, 0.5, 0.0, 1.0),
    (1, 37, 2, 0.03, 0.5, 0.7),
    (53, 1, 4, 0.4, 1.0, 0.25),
    (97, 61, 1, 0.6, 0.8, 2.0),                 # R_0 = 110 > width
    (97, 61, 3, 0.05, 1.0, 0.25),
    (64, 48, 4, 0.004, 0.0, 0.5),
    (130, 33, 2, 0.2, 3.0, 1.5),
    (960, 540, 4, 0.004, 1.0, 0.25),            # the defaults at a quarter of 1080p... in pixels: R = 7, 13, 26, 52
    (1000, 541, 2, 0.02, 2.0, 0.8),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}_L{c[2]}" for c in CASES])
def test_synthetic_hdr_matches_the_restatement(ctx, po, case):
    rrt, _ = ctx
    w, h, lobes, radius, threshold, intensity = case
    rng = np.random.default_rng(w * 1000 + h)
    hdr = synthetic_hdr(rng, w, h)
    g = rrt.GlowSettings(lobes=lobes, radius=radius, threshold=threshold, intensity=intensity)
    got = glow(rrt, _device_hdr(hdr), w, h, g)
    want = expected(po, rrt, hdr, g)
    assert np.array_equal(got, want), (case, int((got != want).any(-1).sum()))
    plain = tone_map(po, hdr[..., :3])
    if w * h > 1:
        assert not np.array_equal(got, plain)                  # the glow is visible


def test_lobe_counts_and_radii(ctx, po):
    rrt, _ = ctx
    rng = np.random.default_rng(77)
    w, h = 150, 90
    hdr = synthetic_hdr(rng, w, h)
    d = _device_hdr(hdr)
    for lobes in (1, 2, 3, 4):
        for radius in (0.002, 0.011, 0.09):
            for threshold in (0.0, 1.0, 25.0):
                g = rrt.GlowSettings(lobes=lobes, radius=radius, threshold=threshold, intensity=0.6)
                assert np.array_equal(glow(rrt, d, w, h, g), expected(po, rrt, hdr, g)), (lobes, radius, threshold)


def _real_frames(rrt, tex):
    """(name, rgba8, hdr) of supersampled (s = 1, 2) and motion-blurred (K = 2) frames of random scenes"""
    rng = np.random.default_rng(4242)
    for case in range(3):
        sc, cam, fx = scene(rrt, rng, case)
        prm = rrt.RenderParams(spin=sc["spin"], volumetrics=sc["vol"], arith_mode=2 if case % 2 else 0)
        for s in (1, 2):
            yield (case, "ss", s), *render_ss(rrt, tex, sc["w"], sc["h"], s, sc["t"], cam, fx, prm)
        times = [sc["t"], sc["t"] + 0.05]
        yield (case, "mb", 2), *render_mb(rrt, tex, sc["w"], sc["h"], 1, times, moving_cameras(rrt, sc, 2), fx, prm)


def test_real_frames_match_the_restatement_and_the_identities(ctx, po):
    rrt, tex = ctx
    n_visible = 0
    for what, rgba8, hdr in _real_frames(rrt, tex):
        h, w = rgba8.shape[:2]
        d = _device_hdr(hdr)
        g = rrt.GlowSettings(lobes=3, radius=0.02, threshold=0.3, intensity=0.8)
        got = glow(rrt, d, w, h, g)
        assert np.array_equal(got, expected(po, rrt, hdr, g)), what
        n_visible += not np.array_equal(got, rgba8)
        for off in (rrt.GlowSettings(intensity=0.0), rrt.GlowSettings(threshold=3.0e38, intensity=2.0)):
            assert np.array_equal(glow(rrt, d, w, h, off), rgba8), (what, off.info())
    assert n_visible > 0


def test_side_stream_and_graph_capture(ctx):
    """_ss followed by the glow: on a side stream and captured into one graph (a chain), the bytes of eager launches"""
    import torch
    rrt, tex = ctx
    w, h = 120, 68
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=0.9)
    g = rrt.GlowSettings(lobes=4, radius=0.01, threshold=0.2, intensity=0.7)
    _, hdr = render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, prm)
    ref = glow(rrt, _device_hdr(hdr), w, h, g)
    side = torch.cuda.Stream()
    assert np.array_equal(glow(rrt, _device_hdr(hdr), w, h, g, stream=side), ref)
    out, lin = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    scratch = torch.empty(rrt.glow_scratch_bytes(w, h, g), dtype=torch.uint8, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch_ss(out, w, h, 2, 1.0, cam, tex, fx, prm, hdr=lin)
        rrt.launch_glow(out, lin, w, h, g, scratch)
    for _ in range(2):
        out.zero_(); lin.zero_(); scratch.zero_()
        graph.replay()
        assert np.array_equal(_host(out, (h, w, 4)), ref)


@pytest.mark.parametrize("mode", [["--supersample", "2"], ["--motion-blur", "2"]])
def test_drivers_write_the_glowed_frames(ctx, tmp_path, mode):
    """rrt_headless and headless.py --glow 0.5: the same file, the summary's glow settings, and every frame == the library's _ss /
    _mb launch at the driver's clock and CameraPath(0)'s cameras, then rrt_launch_glow"""
    import torch
    from relativisticraytracer_amd import build
    from relativisticraytracer_amd import camera_paths as cp
    rrt, tex = ctx
    exe = build.build_headless()
    w, h = 96, 54
    a, b = tmp_path / "cpp.rgba", tmp_path / "py.rgba"
    args = ["--width", str(w), "--height", str(h), "--frames", "3", "--path", "0", "--spin", "0.9", "--all-effects",
            "--glow", "0.5", "--glow-threshold", "0.2", "--glow-radius", "0.01", "--glow-lobes", "3"] + mode
    r = subprocess.run([exe] + args + ["--out", str(a)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["glow"] == {"radius": 0.01, "lobes": 3, "threshold": 0.2, "intensity": 0.5}, meta
    r = subprocess.run([sys.executable, "-m", "relativisticraytracer_amd.headless"] + args + ["--out", str(b)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["glow"]["lobes"] == 3 and abs(meta["glow"]["intensity"] - 0.5) < 1e-7 and meta["tile_order"] is None, meta
    assert open(a, "rb").read() == open(b, "rb").read()
    data = np.fromfile(a, np.uint8).reshape(3, h, w, 4)
    path = cp.CameraPath(0)
    fx = rrt.CameraEffects(useChromaticAberration=True)
    prm = rrt.RenderParams(spin=0.9)
    g = rrt.GlowSettings(lobes=3, radius=0.01, threshold=0.2, intensity=0.5)
    n_visible = 0
    for k in (1, 2, 3):
        if mode[0] == "--supersample":
            st, pt = cp.recording_clock(k, 24)
            plain, hdr = render_ss(rrt, tex, w, h, 2, st, path.camera_at(pt), fx, prm)
        else:
            st, pt = cp.motion_clock(k, 24, 0.5, 2)
            plain, hdr = render_mb(rrt, tex, w, h, 1, st, [path.camera_at(p) for p in pt], fx, prm)
        assert np.array_equal(glow(rrt, _device_hdr(hdr), w, h, g), data[k - 1]), k
        n_visible += not np.array_equal(plain, data[k - 1])
    assert n_visible > 0
    torch.cuda.synchronize()
