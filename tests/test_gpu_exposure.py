"""Exposure control (rrt_launch_exposure, include/rrt.h) against its numpy restatement (tests/exposure_ref.py): the histogram the
meter pass leaves, the state (ev, scale, the diagnostics), the scaled HDR bit for bit and the RGBA8 byte for byte through the portable
exp -- on synthetic frames of every ragged shape, frames of 2^20 pixels and more (the meter's strided rounds: one pixel over, a
ragged second round, 1080p), flat and black frames, sequences on one state without a host synchronisation, manual
mode, real supersampled / fisheye / stereo frames, a captured _ss -> exposure -> glow graph, and both headless drivers.  torch is only
the device-memory plumbing."""

import numpy as np
import pytest

import exposure_ref as er
import glow_ref
from conftest import same_bits
from gpu_util import _host, _zeros, run_drivers
from sampled_util import render_pano, render_ss, render_stereo

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    yield rrt, tex, er.library_table(rrt)
    tex.destroy()


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, F).ravel()).cuda()


def new_scratch(rrt, stream=None):
    """a scratch full of 0xff, then reset: whatever the reset does not write would show"""
    import torch
    scratch = torch.full((rrt.exposure_scratch_bytes(),), 255, dtype=torch.uint8, device="cuda")
    rrt.launch_exposure_reset(scratch, stream=stream)
    return scratch


def parse_state(raw):
    """the scratch's documented layout, from its bytes (a uint8 array)"""
    raw = np.ascontiguousarray(raw, np.uint8)
    s = raw[1024:1088]
    return {"hist": raw[0:1024].view(np.uint32).copy(), "ev": s[0:4].view(F)[0], "frames": int(s[4:8].view(np.uint32)[0]),
            "scale": s[8:12].view(F)[0], "target": s[12:16].view(F)[0], "n": int(s[16:24].view(np.uint64)[0]),
            "m": s[24:32].view(np.float64)[0], "reserved": s[32:64].copy(), "table": raw[1088:1088 + 2048].view(np.float64).copy()}


def read_state(scratch):
    import torch
    torch.cuda.synchronize()
    return parse_state(scratch.cpu().numpy())


def launch(rrt, d_in, w, h, s, scratch=None, bytes8=True, lin=True, in_place=False, stream=None):
    """rrt_launch_exposure of a device frame: (rgba8 or None, scaled hdr or None) on the host"""
    import torch
    out = _zeros(h * w * 4, torch.uint8) if bytes8 else None
    d_out = d_in if in_place else (_zeros(h * w * 4, torch.float32) if lin else None)
    rrt.launch_exposure(out, d_out, d_in, w, h, s, scratch, stream=stream)
    return (_host(out, (h, w, 4)) if bytes8 else None), (_host(d_out, (h, w, 4)) if d_out is not None else None)


def bits(x):
    return int(np.array([x], F).view(np.uint32)[0])


def check_state(po, got, st, n, m, target, what):
    assert got["n"] == n and got["frames"] == st.frames, what
    assert bits(got["ev"]) == bits(st.ev), (what, got["ev"], st.ev)
    assert bits(got["scale"]) == bits(er.scale_of(po, st.ev)), what
    assert bits(got["target"]) == bits(target if target is not None else 0.0), what
    assert got["m"] == (m if m is not None else 0.0), what
    assert not got["reserved"].any(), what


def synthetic_hdr(rng, w, h):
    """lumas log-uniform over 18 octaves, a few exact zeros and slightly negative pixels, an alpha that is not 1"""
    hdr = (2.0 ** rng.uniform(-12.0, 6.0, (h, w, 1)) * rng.uniform(0.3, 1.7, (h, w, 3))).astype(F)
    hdr = np.concatenate([hdr, rng.uniform(0.0, 1.0, (h, w, 1)).astype(F)], axis=-1)
    r = rng.random((h, w))
    hdr[r < 0.05, :3] = 0.0
    hdr[(r >= 0.05) & (r < 0.07), :3] = F(-1e-3)
    return hdr


AUTO = dict(mode="auto", key=0.18, ev=0.25, low_permille=100, high_permille=50)
SHAPES = [(1, 1), (7, 5), (65, 3), (257, 9), (300, 200)]     # below one wave, ragged against 64 and 256, several workgroups


# Frames of more than kMeterCUs * kMeterGroupsPerCU * kMeterThreads * kMeterRun = 2^20 pixels send exposure_meter's waves round their
# `base += stride` loop more than once (tests/test_post_pass_geometry.py asserts, without a GPU, what each of these shapes reaches)
STRIDED_SHAPES = [
    (1024, 1024),    # 2^20: the last frame of one round, 1024 workgroups, none ragged
    (61681, 17),     # 2^20 + 1: a second round taken by one wave with one lane inside the frame
    (1049, 1000),    # 2^20 + 424: the second round taken by two of workgroup 0's four waves, the second one ragged
    (1031, 1019),    # 2^20 + 2013: the second round taken by workgroups 0 and 1, the last wave's last run ragged
    (1920, 1080),    # 1080p: 1.98 rounds, the second taken by 1001 whole workgroups
]
RAGGED_SHAPES = [(61681, 17), (1049, 1000), (1031, 1019)]
VARIANT_SHAPE = (1031, 1019)
ALONE = 2.0 ** 10         # a luma no pixel of synthetic_hdr has (at most 2^6 * 1.7): the last pixel, which past-the-end lanes load


def check_auto_frame(ctx, po, hdr, variants=True):
    """one auto launch on a fresh state against the restatement: the histogram, the state, the scaled HDR's bits, the RGBA8 bytes"""
    rrt, _, table = ctx
    h, w = hdr.shape[:2]
    s = rrt.ExposureSettings(**AUTO)
    st = er.State()
    want_hist, want_scale, want_hdr, want8 = er.expose(po, rrt, hdr, s, st, table)
    n, m, target = er.resolve(want_hist, table, s)
    scratch = new_scratch(rrt)
    fresh = read_state(scratch)
    assert not fresh["hist"].any() and fresh["frames"] == 0 and bits(fresh["ev"]) == 0 and np.array_equal(fresh["table"], table)
    got8, got_hdr = launch(rrt, _device(hdr), w, h, s, scratch)
    got = read_state(scratch)
    assert np.array_equal(got["hist"], want_hist), int((got["hist"] != want_hist).sum())
    check_state(po, got, st, n, m, target, (w, h))
    assert np.array_equal(got["table"], table)
    assert same_bits(got_hdr, want_hdr) and np.array_equal(got8, want8), int((got8 != want8).any(-1).sum())
    if w * h > 1:
        assert bits(want_scale) != bits(1.0) and not np.array_equal(want8, er.tone_map(po, hdr[..., :3]))   # the exposure is visible
    # in place, bytes only, HDR only: the same frame from a fresh state
    for kw in (dict(in_place=True), dict(lin=False), dict(bytes8=False)) if variants else ():
        scratch = new_scratch(rrt)
        a8, ah = launch(rrt, _device(hdr), w, h, s, scratch, **kw)
        assert a8 is None or np.array_equal(a8, want8), kw
        assert ah is None or same_bits(ah, want_hdr), kw
        assert bits(read_state(scratch)["ev"]) == bits(st.ev), kw
    return want_hist


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_synthetic_frames_match_the_restatement(ctx, po, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    check_auto_frame(ctx, po, synthetic_hdr(rng, w, h))


@pytest.mark.parametrize("w,h", STRIDED_SHAPES, ids=[f"{w}x{h}" for w, h in STRIDED_SHAPES])
def test_strided_rounds_match_the_restatement(ctx, po, w, h):
    """frames of 2^20 pixels and more: the meter's second round, taken by one lane, by part of a workgroup, by a thousand workgroups.
    The last pixel, which every past-the-end lane loads, is alone in its bin: a meter that counted those lanes would count it again"""
    import torch
    rrt = ctx[0]
    rng = np.random.default_rng(w * 1000 + h)
    hdr = synthetic_hdr(rng, w, h)
    hdr[h - 1, w - 1, :3] = F(ALONE)
    alone = er.bin_of(er.luma(hdr[h - 1:, w - 1:]))[1].item()
    want_hist = check_auto_frame(ctx, po, hdr, variants=(w, h) == VARIANT_SHAPE)
    assert want_hist[alone] == 1 and int(want_hist.sum()) < w * h
    if (w, h) in RAGGED_SHAPES:
        assert np.array_equal(rrt.exposure_meter_host(hdr), want_hist)          # the library's host meter: a third count of the frame
    torch.cuda.empty_cache()


def test_flat_and_black_frames_in_strided_rounds(ctx, po):
    """1031 x 1019, two rounds: a frame in ONE bin takes the one-add path on every round and the bin holds w * h; a black frame
    meters nothing in either round and keeps ev -- on the first frame it takes the clamped setting"""
    import torch
    rrt, _, table = ctx
    w, h = VARIANT_SHAPE
    s = rrt.ExposureSettings(**dict(AUTO, adapt_up=0.5, adapt_down=0.25))
    flat = np.empty((h, w, 4), F)
    flat[...] = (0.3, 0.2, 0.1, 1.0)
    black = np.zeros((h, w, 4), F)
    black[..., 3] = 1.0
    scratch, st = new_scratch(rrt), er.State()
    for what, frame in (("flat", flat), ("black", black), ("flat again", flat)):
        want_hist, _, want_hdr, want8 = er.expose(po, rrt, frame, s, st, table)
        got8, got_hdr = launch(rrt, _device(frame), w, h, s, scratch)
        got = read_state(scratch)
        assert np.array_equal(got["hist"], want_hist), what
        check_state(po, got, st, *er.resolve(want_hist, table, s), what)
        assert same_bits(got_hdr, want_hdr) and np.array_equal(got8, want8), what
        if what.startswith("flat"):
            assert (want_hist > 0).sum() == 1 and int(want_hist.max()) == w * h and got["n"] == w * h
        else:
            assert got["n"] == 0 and bits(got["ev"]) == kept, what
        kept = bits(got["ev"])
    scratch = new_scratch(rrt)                                                   # black first: the setting, clamped
    launch(rrt, _device(black), w, h, rrt.ExposureSettings(mode="auto", ev=5.0, min_ev=-2.0, max_ev=2.0), scratch, lin=False)
    got = read_state(scratch)
    assert (got["n"], got["frames"]) == (0, 1) and got["ev"] == F(2.0) and not got["hist"].any()
    torch.cuda.empty_cache()


def test_flat_and_black_frames(ctx, po):
    """a frame in ONE bin (every wave takes the one-add path), two flat halves (uniform waves and mixed ones), and black frames:
    N == 0 keeps ev -- on the first frame it takes the clamped setting"""
    rrt, _, table = ctx
    w, h = 300, 200
    s = rrt.ExposureSettings(**dict(AUTO, adapt_up=0.5, adapt_down=0.25))
    flat = np.empty((h, w, 4), F)
    flat[...] = (0.3, 0.2, 0.1, 1.0)
    halves = flat.copy()
    halves[:, 137:, :3] = (5.0, 6.0, 7.0)
    black = np.zeros((h, w, 4), F)
    black[..., 3] = 1.0
    scratch, st = new_scratch(rrt), er.State()
    for what, frame in (("flat", flat), ("halves", halves), ("black", black), ("flat again", flat), ("black again", black)):
        want_hist, _, want_hdr, want8 = er.expose(po, rrt, frame, s, st, table)
        got8, got_hdr = launch(rrt, _device(frame), w, h, s, scratch)
        got = read_state(scratch)
        assert np.array_equal(got["hist"], want_hist), what
        check_state(po, got, st, *er.resolve(want_hist, table, s), what)
        assert same_bits(got_hdr, want_hdr) and np.array_equal(got8, want8), what
        if what == "flat":
            assert (want_hist > 0).sum() == 1 and int(want_hist.sum()) == w * h
        if what.startswith("black"):
            assert got["n"] == 0 and bits(got["ev"]) == kept, what
        kept = bits(got["ev"])
    # black first: the setting, clamped
    for ev, lo, hi in ((1.25, -8.0, 8.0), (5.0, -2.0, 2.0), (-5.0, -2.0, 2.0)):
        scratch = new_scratch(rrt)
        launch(rrt, _device(black), w, h, rrt.ExposureSettings(mode="auto", ev=ev, min_ev=lo, max_ev=hi), scratch, lin=False)
        got = read_state(scratch)
        assert (got["n"], got["frames"]) == (0, 1) and got["ev"] == F(min(max(ev, lo), hi)), (ev, lo, hi)


def test_sequence_on_one_state_without_a_host_synchronisation(ctx, po):
    """six launches on a side stream, each frame brighter or darker than the last, adapt_up != adapt_down: ev after every launch
    (copied aside on the stream, read once at the end) is the restatement's; the reset starts the sequence over"""
    import torch
    rrt, _, table = ctx
    w, h = 97, 61
    rng = np.random.default_rng(61)
    base = synthetic_hdr(rng, w, h)
    gains = (1.0, 40.0, 0.02, 3.0, 3.0, 0.5)
    frames = [base * np.array([g, g, g, 1.0], F) for g in gains]
    s = rrt.ExposureSettings(**dict(AUTO, adapt_up=0.5, adapt_down=0.125))
    d_frames = [_device(f) for f in frames]
    outs = [_zeros(h * w * 4, torch.uint8) for _ in frames]
    n_log = len(frames) + 2
    log = torch.zeros(n_log, rrt.exposure_scratch_bytes(), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        scratch = new_scratch(rrt, stream=side)
        for k, d in enumerate(d_frames):
            rrt.launch_exposure(outs[k], None, d, w, h, s, scratch, stream=side)
            log[k].copy_(scratch, non_blocking=True)
        rrt.launch_exposure_reset(scratch, stream=side)
        for k in (0, 1):
            rrt.launch_exposure(None, d_frames[k], d_frames[k], w, h, s, scratch, stream=side)
            log[len(frames) + k].copy_(scratch, non_blocking=True)
    side.synchronize()
    raw = log.cpu().numpy()
    st, evs = er.State(), []
    for k, f in enumerate(frames):
        hist, _, _, want8 = er.expose(po, rrt, f, s, st, table)
        got = parse_state(raw[k])
        assert np.array_equal(got["hist"], hist), k
        check_state(po, got, st, *er.resolve(hist, table, s), k)
        assert np.array_equal(_host(outs[k], (h, w, 4)), want8), k
        evs.append(bits(st.ev))
    assert len(set(evs)) == len(evs)                                  # the state moved every frame
    ups = [er.resolve(er.histogram(f), table, s)[2] for f in frames]
    assert any(t > F(0) for t in ups) and any(t < F(0) for t in ups)
    for k in (0, 1):
        got = parse_state(raw[len(frames) + k])
        assert got["frames"] == k + 1 and bits(got["ev"]) == evs[k], k


def test_manual_mode(ctx, po):
    """EV 0 is the identity -- the bytes _ss itself wrote and its HDR bits; EV +-1.5 is the restatement; no scratch is needed"""
    rrt, tex, _ = ctx
    w, h = 96, 64
    cam, fx, prm = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    rgba8, hdr = render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, prm)
    d = _device(hdr)
    got8, got_hdr = launch(rrt, d, w, h, rrt.ExposureSettings(ev=0.0))
    assert np.array_equal(got8, rgba8) and same_bits(got_hdr, hdr)
    for ev in (1.5, -1.5):
        s = rrt.ExposureSettings(ev=ev)
        _, scale, want_hdr, want8 = er.expose(po, rrt, hdr, s)
        assert scale == F(2.0 ** ev) or abs(float(scale) / 2.0 ** ev - 1.0) < 1e-6
        got8, got_hdr = launch(rrt, d, w, h, s)
        assert same_bits(got_hdr, want_hdr) and np.array_equal(got8, want8), ev
        assert not np.array_equal(got8, rgba8)
        a8, ah = launch(rrt, _device(hdr), w, h, s, in_place=True)
        assert same_bits(ah, want_hdr) and np.array_equal(a8, want8), ev
    rng = np.random.default_rng(9)
    syn = synthetic_hdr(rng, 257, 9)
    s = rrt.ExposureSettings(ev=-1.5)
    got8, got_hdr = launch(rrt, _device(syn), 257, 9, s)
    _, _, want_hdr, want8 = er.expose(po, rrt, syn, s)
    assert same_bits(got_hdr, want_hdr) and np.array_equal(got8, want8)


def test_real_frames(ctx, po):
    """a supersampled frame, a fisheye dome (the outside of the disc is not metered) and a top-bottom stereo composite"""
    rrt, tex, table = ctx
    w, h = 96, 64
    cam, fx, prm = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    stereo = rrt.Stereo("top-bottom", 1.0, 30.0, None)
    frames = [("ss", render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, prm)),
              ("fisheye", render_pano(rrt, tex, w, h, 1, rrt.Projection("fisheye"), 1.0, cam, fx, prm)),
              ("stereo", render_stereo(rrt, tex, w, h // 2, 1, rrt.Projection("pinhole"), stereo, 1.0, cam, fx, prm))]
    s = rrt.ExposureSettings(mode="auto")
    for what, (rgba8, hdr) in frames:
        assert hdr.shape == (h, w, 4), what
        st = er.State()
        hist, _, want_hdr, want8 = er.expose(po, rrt, hdr, s, st, table)
        scratch = new_scratch(rrt)
        got8, got_hdr = launch(rrt, _device(hdr), w, h, s, scratch)
        got = read_state(scratch)
        assert np.array_equal(got["hist"], hist), what
        check_state(po, got, st, *er.resolve(hist, table, s), what)
        assert same_bits(got_hdr, want_hdr) and np.array_equal(got8, want8), what
        assert not np.array_equal(got8, rgba8), what
        if what == "fisheye":
            lit = int((er.luma(hdr) > 0).sum())
            assert got["n"] == lit and 0.3 * w * h < lit < 0.6 * w * h          # the disc: pi/4 of the 64 x 64 square


def test_graph_capture_advances_the_state(ctx, po):
    """_ss -> exposure (in place) -> glow captured as one chain and replayed three times: each replay advances the state, and the
    three frames are the restatement's three-frame sequence"""
    import torch
    rrt, tex, table = ctx
    w, h = 96, 64
    cam, fx, prm = rrt.CameraState.default(), rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    s = rrt.ExposureSettings(mode="auto", key=0.3, adapt_up=0.5, adapt_down=0.25)
    g = rrt.GlowSettings(lobes=3, radius=0.02, threshold=0.3, intensity=0.6)
    _, hdr = render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, prm)
    out, lin = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    gs = torch.empty(rrt.glow_scratch_bytes(w, h, g), dtype=torch.uint8, device="cuda")
    scratch = new_scratch(rrt)
    # frame 0 eagerly: the first frame jumps to its target, so that the replays below show the adaptation
    dark = hdr * np.array([0.05, 0.05, 0.05, 1.0], F)
    st = er.State()
    er.expose(po, rrt, dark, s, st, table)
    launch(rrt, _device(dark), w, h, s, scratch, lin=False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch_ss(out, w, h, 2, 1.0, cam, tex, fx, prm, hdr=lin)
        rrt.launch_exposure(None, lin, lin, w, h, s, scratch)
        rrt.launch_glow(out, lin, w, h, g, gs)
    taps = glow_ref.lobe_taps(rrt, g, h)
    seen = []
    for k in range(3):
        out.zero_(); lin.zero_()
        graph.replay()
        got8 = _host(out, (h, w, 4)).copy()
        hist, _, scaled, _ = er.expose(po, rrt, hdr, s, st, table)
        want8 = er.tone_map(po, glow_ref.glow_hdr(scaled, taps, g.threshold, g.intensity))
        assert np.array_equal(got8, want8), (k, int((got8 != want8).any(-1).sum()))
        got = read_state(scratch)
        assert got["frames"] == k + 2 and bits(got["ev"]) == bits(st.ev), k
        seen.append(bits(st.ev))
    assert len(set(seen)) == 3


@pytest.mark.parametrize("with_glow", [False, True], ids=["plain", "glow"])
def test_drivers_write_the_exposed_frames(ctx, po, tmp_path, with_glow):
    """rrt_headless and headless.py --auto-exposure --exposure-speed 0.2 1.0 on four frames of path 0: the same file, every frame the
    restatement's exposure of the library's _ss frame at the driver's clock and camera (then glow_ref with --glow), the settings and
    the final ev in the summary"""
    from relativisticraytracer_amd import camera_paths as cp
    rrt, tex, table = ctx
    w, h, frames, fps = 64, 48, 4, 24
    args = ["--width", str(w), "--height", str(h), "--frames", str(frames), "--path", "0", "--spin", "0.9",
            "--auto-exposure", "--exposure-speed", "0.2", "1.0"]
    g = None
    if with_glow:
        args += ["--glow", "0.25", "--glow-threshold", "0.3", "--glow-radius", "0.02"]
        g = rrt.GlowSettings(radius=0.02, threshold=0.3, intensity=0.25)
    s = rrt.ExposureSettings(mode="auto", adapt_up=float(rrt.exposure_adapt(1.0 / fps, 0.2)), adapt_down=float(rrt.exposure_adapt(1.0 / fps, 1.0)))
    assert 0.0 < s.adapt_down < s.adapt_up < 1.0
    path, fx, prm = cp.CameraPath(0), rrt.CameraEffects(), rrt.RenderParams(spin=0.9)
    st, want, n_visible = er.State(), [], 0
    for k in range(1, frames + 1):
        t, pt = cp.recording_clock(k, fps)
        plain, hdr = render_ss(rrt, tex, w, h, 1, t, path.camera_at(pt), fx, prm)
        _, _, scaled, bytes8 = er.expose(po, rrt, hdr, s, st, table)
        if g is not None:
            bytes8 = er.tone_map(po, glow_ref.glow_hdr(scaled, glow_ref.lobe_taps(rrt, g, h), g.threshold, g.intensity))
        n_visible += not np.array_equal(plain, bytes8)
        want.append(bytes8)
    want = np.stack(want)
    assert n_visible == frames
    meta_c, meta_p, out = run_drivers(tmp_path, args)
    for name, meta in (("cpp", meta_c), ("py", meta_p)):           # one file: run_drivers found the two byte-identical
        e = meta["exposure"]
        assert e["mode"] == "auto" and (e["key"], e["low_permille"], e["high_permille"], e["min_ev"], e["max_ev"]) == (0.5, 400, 20, -8, 8), (name, e)
        assert bits(e["adapt_up"]) == bits(s.adapt_up) and bits(e["adapt_down"]) == bits(s.adapt_down), (name, e)
        assert bits(e["final_ev"]) == bits(st.ev), (name, e, st.ev)
        assert (meta["glow"] is not None) == with_glow, (name, meta)
        data = np.fromfile(out, np.uint8).reshape(frames, h, w, 4)
        assert np.array_equal(data, want), (name, [int((a != b).any(-1).sum()) for a, b in zip(data, want)])
