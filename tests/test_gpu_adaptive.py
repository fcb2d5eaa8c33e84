"""Adaptively supersampled frames (rrt_launch_raymarch_adaptive, include/rrt.h) against their definition: out = where(mask, ss, base),
byte for byte and bit for bit, with base the s = 1 frame and ss the s x s frame of rrt_launch_raymarch_ss (or _pano) -- launches that
tests/test_gpu_supersample.py and tests/test_gpu_projection.py pin -- and mask the numpy restatement of the rule on the stored base
bytes (tests/adaptive_ref.py).  The device's list is compared as a set with the mask, its count with the list's length.  Small frames:
96x64 and a ragged 67x45, the default view and a disk-grazing one.  torch is only the device-memory plumbing."""

import numpy as np
import pytest

import adaptive_ref
from conftest import same_bits
from gpu_util import _host, _zeros, run_drivers

pytestmark = pytest.mark.gpu

SIZES = ((96, 64), (67, 45))
T_TIME = 1.0


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    table = rrt.NoiseTable(4.0)
    yield rrt, tex, table
    table.destroy()
    tex.destroy()


def views(rrt):
    return {"default": rrt.CameraState.default(), "grazing": rrt.CameraState.from_angles((35.0, 0.8, 10.0), -106.0, -1.2)}


def all_effects(rrt):
    return rrt.CameraEffects(useBloom=True, useVignette=True, useChromaticAberration=True, useLensDistortion=True)


def render_ref(rrt, tex, w, h, s, cam, fx, prm, proj=None):
    """the reference launch of the definition: (rgba8, hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    if proj is None:
        rrt.launch_raymarch_ss(out, w, h, s, T_TIME, cam, tex, fx, prm, hdr=hdr)
    else:
        rrt.launch_raymarch_pano(out, w, h, s, proj, T_TIME, cam, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def render_adaptive(rrt, tex, w, h, s, T, cam, fx, prm, proj=None, with_hdr=True, stream=None):
    """the adaptive frame into fresh buffers (filled with a pattern no launch writes): (rgba8, hdr or None, count, list)"""
    import torch
    out = torch.full((h * w * 4,), 0x5a, dtype=torch.uint8, device="cuda")
    hdr = torch.full((h * w * 4,), -7.0, dtype=torch.float32, device="cuda") if with_hdr else None
    scratch = torch.full((rrt.adaptive_scratch_bytes(w, h),), 0xa5, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())          # the fills above
    rrt.launch_raymarch_adaptive(out, w, h, s, proj, rrt.AdaptiveSettings(T), T_TIME, cam, tex, fx, scratch, prm, hdr=hdr, stream=stream)
    torch.cuda.synchronize()
    words = scratch.cpu().numpy().view(np.uint32)
    count = int(words[0])
    assert count <= w * h, count
    return _host(out, (h, w, 4)), (_host(hdr, (h, w, 4)) if with_hdr else None), count, words[4:4 + count].copy()


def check_definition(rrt, tex, w, h, s, T, cam, fx, prm, what, proj=None, share=(0.02, 0.40)):
    """render base, ss and the adaptive frame and compare with where(mask, ss, base); returns (mask, out8).  share: the bounds
    the refined share must lie in, so that the expected frame is neither of its inputs (None: the caller's own condition)"""
    base8, baseH = render_ref(rrt, tex, w, h, 1, cam, fx, prm, proj)
    ss8, ssH = render_ref(rrt, tex, w, h, s, cam, fx, prm, proj)
    m = adaptive_ref.mask(base8, T)
    frac = float(m.mean())
    print(f"adaptive {what}: {w}x{h} s={s} T={T} refined {int(m.sum())} = {frac:.4f}, bytes ss != base on {int((ss8 != base8).any(-1).sum())} px")
    if share is not None:
        assert share[0] <= frac <= share[1], (what, frac)
    out8, outH, count, lst = render_adaptive(rrt, tex, w, h, s, T, cam, fx, prm, proj)
    assert count == int(m.sum()), (what, count, int(m.sum()))
    assert np.array_equal(np.sort(lst), np.flatnonzero(m.ravel()).astype(np.uint32)), what
    want8, wantH = adaptive_ref.expected(base8, ss8, m), adaptive_ref.expected(baseH, ssH, m)
    assert np.array_equal(out8, want8), (what, int((out8 != want8).any(-1).sum()))
    assert same_bits(outH, wantH), (what, int((outH != wantH).any(-1).sum()))
    if share is not None and s > 1:          # the expected frame is neither input
        assert not np.array_equal(want8, base8) and not np.array_equal(want8, ss8), what
    return m, out8


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("arith", [0, 2], ids=["strict", "fmad"])
@pytest.mark.parametrize("s", [2, 4, 8])
def test_definition(ctx, s, arith):
    """both sizes x both views x (noise table, nudge) on and off, default effects; all effects on and spin 0 once each"""
    rrt, tex, table = ctx
    fx = rrt.CameraEffects()
    for (w, h) in SIZES:
        for name, cam in views(rrt).items():
            for use_table, nudge in ((False, 0), (True, 0), (False, 3), (True, 3)):
                prm = rrt.RenderParams(spin=0.9, arith_mode=arith, noise_table=table.id if use_table else 0, nudge_ulps=nudge,
                                       nudge_seed=11)
                check_definition(rrt, tex, w, h, s, 8, cam, fx, prm, f"{name} table={use_table} nudge={nudge} arith={arith}")
    w, h = SIZES[1]
    check_definition(rrt, tex, w, h, s, 8, views(rrt)["grazing"], all_effects(rrt), rrt.RenderParams(spin=0.9, arith_mode=arith),
                     f"grazing all effects arith={arith}")
    check_definition(rrt, tex, w, h, s, 8, views(rrt)["default"], fx, rrt.RenderParams(spin=0.0, arith_mode=arith),
                     f"default spin 0 arith={arith}")


def test_without_an_hdr_plane(ctx):
    """d_hdr_rgba32f NULL: the same bytes"""
    rrt, tex, _ = ctx
    w, h = SIZES[1]
    cam, fx, prm = views(rrt)["grazing"], rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    _, want8 = check_definition(rrt, tex, w, h, 2, 8, cam, fx, prm, "with hdr")
    out8, _, _, _ = render_adaptive(rrt, tex, w, h, 2, 8, cam, fx, prm, with_hdr=False)
    assert np.array_equal(out8, want8)


# ---------------------------------------------------------------- the ends
def test_ends(ctx):
    rrt, tex, _ = ctx
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    for (w, h) in SIZES:
        for name, cam in views(rrt).items():
            base8, baseH = render_ref(rrt, tex, w, h, 1, cam, fx, prm)
            for s in (2, 8):                    # T = 255 refines nothing: the base frame, count 0
                out8, outH, count, _ = render_adaptive(rrt, tex, w, h, s, 255, cam, fx, prm)
                assert count == 0 and np.array_equal(out8, base8) and same_bits(outH, baseH), (name, s)
            for T in (0, 8, 255):               # s = 1: the base frame at any T (the refined pixels are rendered again, the same)
                out8, outH, count, _ = render_adaptive(rrt, tex, w, h, 1, T, cam, fx, prm)
                assert np.array_equal(out8, base8) and same_bits(outH, baseH), (name, T)
                assert count == int(adaptive_ref.mask(base8, T).sum())
    # T = 0 on the default view: nearly every pixel is refined, the waves run full, and the definition still holds
    for s in (2, 4):
        m, _ = check_definition(rrt, tex, 96, 64, s, 0, views(rrt)["default"], fx, prm, "T=0", share=(0.90, 1.0))
        assert m.mean() >= 0.90


# ---------------------------------------------------------------- panoramas
@pytest.mark.parametrize("s", [2, 4])
@pytest.mark.parametrize("kind,w,h", [("equirect", 128, 64), ("fisheye", 64, 64)])
def test_panoramas(ctx, kind, w, h, s):
    """the same check with rrt_launch_raymarch_pano as the reference; the fisheye's rim has refined pixels whose sub-samples lie
    partly outside the disc (HDR exactly 0, no march: they still enter the pixel's tree)"""
    rrt, tex, _ = ctx
    proj = rrt.Projection(kind)
    for arith in (0, 2):
        prm = rrt.RenderParams(spin=0.9, arith_mode=arith)
        m, _ = check_definition(rrt, tex, w, h, s, 8, views(rrt)["default"], rrt.CameraEffects(), prm, f"{kind} arith={arith}", proj=proj)
        if kind == "fisheye":
            W, H = s * w, s * h
            xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
            u = (np.float32(2.0) * (xs + np.float32(0.5)) - np.float32(W)) / np.float32(H)
            v = (np.float32(2.0) * (ys + np.float32(0.5)) - np.float32(H)) / np.float32(H)
            outside = (u * u + v * v > np.float32(1.0)).reshape(h, s, w, s)                   # top-down virtual rows
            n_out = outside.sum(axis=(1, 3))[::-1]                                            # per pixel, bottom-up like the frame
            rim = m & (n_out > 0) & (n_out < s * s)
            assert rim.sum() >= 8, int(rim.sum())


# ---------------------------------------------------------------- packing
def test_fewer_pixels_than_one_wave(ctx):
    """a handful of refined pixels: fewer than the 16 slots of an s = 2 wave, and not a multiple of the 4 slots of an s = 4 wave --
    the last wave is partly empty, and its empty slots leave before the march"""
    rrt, tex, _ = ctx
    fx, prm = rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    found = None
    for (w, h) in SIZES:
        for name, cam in views(rrt).items():
            base8, _ = render_ref(rrt, tex, w, h, 1, cam, fx, prm)
            for T in range(254, 0, -1):
                n = int(adaptive_ref.mask(base8, T).sum())
                if n >= 16:
                    break
                if n >= 1 and n % 4 != 0:
                    found = (w, h, name, cam, T, n)
                    break
            if found:
                break
        if found:
            break
    assert found, "no view / threshold with 1 <= count < 16, count % 4 != 0"
    w, h, name, cam, T, n = found
    for s in (2, 4, 8):
        m, _ = check_definition(rrt, tex, w, h, s, T, cam, fx, prm, f"few pixels ({name})", share=None)
        assert int(m.sum()) == n


def test_refined_pixels_in_every_corner(ctx):
    """a white-noise sky: nearly every pixel differs from its neighbours, the four corners of the frame included -- clamped
    neighbours, the first and the last pixel of the frame in the list, ragged edges.  At 96x64 all but three pixels are refined
    (0.9995), at 67x45 every one (the disk's glow in front of the shadow is noisy enough at that size): there the mask is all
    ones and the frame is the s x s frame itself, the other end of T = 255.  That the expected frame is neither of its inputs is
    test_definition's condition, not this test's."""
    rrt, _, _ = ctx
    noise = np.random.default_rng(7).integers(0, 256, (256, 512, 4), dtype=np.uint8)
    noise[..., 3] = 255
    tex = rrt.SkyTexture(noise)
    try:
        for (w, h) in SIZES:
            for s in (2, 4):
                m, _ = check_definition(rrt, tex, w, h, s, 8, views(rrt)["default"], rrt.CameraEffects(), rrt.RenderParams(spin=0.9),
                                        "noise sky", share=None)
                assert m[0, 0] and m[0, -1] and m[-1, 0] and m[-1, -1], (w, h)
                assert m.mean() > 0.5
    finally:
        tex.destroy()


# ---------------------------------------------------------------- repeatability and capture
def test_repeatable_on_a_side_stream_and_captured(ctx):
    """two launches into fresh buffers give the same bytes, also on a side stream; captured into a graph (a linear chain: base pass,
    zero, mask, refine) and replayed twice over overwritten buffers, the same bytes again"""
    import torch
    rrt, tex, _ = ctx
    w, h, s = 67, 45, 2
    cam, fx, prm = views(rrt)["grazing"], rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    ref8, refH, count, lst = render_adaptive(rrt, tex, w, h, s, 8, cam, fx, prm)
    assert 0 < count < w * h
    for stream in (None, torch.cuda.Stream()):
        got8, gotH, c2, l2 = render_adaptive(rrt, tex, w, h, s, 8, cam, fx, prm, stream=stream)
        assert np.array_equal(got8, ref8) and same_bits(gotH, refH) and c2 == count
        assert np.array_equal(np.sort(l2), np.sort(lst))
    out, lin = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    scratch = torch.zeros(rrt.adaptive_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
    ad = rrt.AdaptiveSettings(8)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch_adaptive(out, w, h, s, None, ad, T_TIME, cam, tex, fx, scratch, prm, hdr=lin)
    for fill in (0x00, 0xff):
        out.fill_(fill); lin.fill_(float(fill)); scratch.fill_(fill)
        graph.replay()
        assert np.array_equal(_host(out, (h, w, 4)), ref8), fill
        assert same_bits(_host(lin, (h, w, 4)), refH), fill
        assert int(scratch[:4].cpu().numpy().view(np.uint32)[0]) == count, fill


# ---------------------------------------------------------------- the drivers
def _driver_frames(rrt, tex, w, h, frames, T, glow=None):
    """what the drivers must write: the Python launch at the recording clock's times and the start-up camera (+ the glow)"""
    import torch
    from relativisticraytracer_amd import camera_paths as cp
    fx, prm, cam = rrt.CameraEffects(), rrt.RenderParams(spin=0.9), rrt.CameraState.default()
    want, fracs = [], []
    for k in range(1, frames + 1):
        st, _ = cp.recording_clock(k, 24)
        out, lin = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
        scratch = torch.zeros(rrt.adaptive_scratch_bytes(w, h), dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch_adaptive(out, w, h, 2, None, rrt.AdaptiveSettings(T), st, cam, tex, fx, scratch, prm, hdr=lin)
        if glow is not None:
            gs = torch.empty(rrt.glow_scratch_bytes(w, h, glow), dtype=torch.uint8, device="cuda")
            plain = _host(out, (h, w, 4)).copy()
            rrt.launch_glow(out, lin, w, h, glow, gs)
            assert not np.array_equal(plain, _host(out, (h, w, 4))), "the glow is invisible: the check would show nothing"
        want.append(_host(out, (h, w, 4)).copy())
        fracs.append(int(scratch[:4].cpu().numpy().view(np.uint32)[0]) / (w * h))
    return np.stack(want), float(np.mean(fracs))


@pytest.mark.parametrize("with_glow", [False, True], ids=["plain", "glow"])
def test_drivers_write_the_adaptive_frames(ctx, tmp_path, with_glow):
    """rrt_headless and headless.py --supersample 2 --adaptive 8: the frames of the Python launch, a refined_fraction in (0, 1) --
    the mean of the frames' counts --, and with --glow 0.25 rrt_launch_glow applied to the adaptive frame's HDR"""
    rrt, tex, _ = ctx
    w, h, frames = 96, 64, 2
    args = ["--width", str(w), "--height", str(h), "--frames", str(frames), "--spin", "0.9", "--supersample", "2", "--adaptive", "8"]
    glow = None
    if with_glow:
        args += ["--glow", "0.25", "--glow-threshold", "0.2", "--glow-radius", "0.02"]
        glow = rrt.GlowSettings(radius=0.02, threshold=0.2, intensity=0.25)
    want, frac = _driver_frames(rrt, tex, w, h, frames, 8, glow)
    assert 0.0 < frac < 1.0
    meta_c, meta_p, out = run_drivers(tmp_path, args)
    for name, meta in (("cpp", meta_c), ("py", meta_p)):           # one file: run_drivers found the two byte-identical
        assert meta["adaptive"]["threshold"] == 8 and meta["supersample"] == 2, (name, meta)
        assert 0.0 < meta["adaptive"]["refined_fraction"] < 1.0, (name, meta)
        assert abs(meta["adaptive"]["refined_fraction"] - frac) < 1e-6, (name, meta, frac)
        data = np.fromfile(out, np.uint8).reshape(frames, h, w, 4)
        assert np.array_equal(data, want), (name, int((data != want).any(-1).sum()))
