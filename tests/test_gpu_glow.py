"""HDR glow (rrt_launch_glow, include/rrt.h) against its numpy restatement (tests/glow_ref.py): synthetic HDR fields and real
supersampled / motion-blurred frames, RGBA8 byte for byte through the portable exp; the identities (intensity 0, a threshold
above every luma); the launch geometry of full-size frames (rows of several glow_hpass segments at both segment sizes, tap tables
of several glow_load_weights launches) on frames a few rows tall; side streams and graph capture; both headless drivers.  torch is
only the device-memory plumbing."""

import numpy as np
import pytest

import glow_ref
from gpu_util import _host, _zeros, ctx, run_drivers
from sampled_util import moving_cameras, render_mb, render_ss, scene, tone_map

pytestmark = pytest.mark.gpu


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


# Full-size launch geometry on the smallest frames that reach it (tests/test_post_pass_geometry.py asserts, without a GPU, that each
# still does): rows of more than one glow_hpass segment at both segment sizes, and tap tables of more than one glow_load_weights
# launch.  The restatement costs taps x pixels, so the frames are thousands of pixels wide and a few rows tall.
GEOMETRY_CASES = {  # name: (w, h, lobes, radius, threshold, intensity, (R per lobe))
    "last_segment_one_pixel": (2049, 2, 2, 2.0, 1.0, 1.0, (12, 24)),
    "three_segments_one_row": (4097, 1, 2, 4.0, 0.5, 0.7, (12, 24)),
    "the_4k_row": (3840, 24, 4, 0.36, 1.0, 0.25, (26, 52, 104, 208)),
    "widest_2048_segment_halo": (2049, 3, 1, 100.33323, 2.0, 0.5, (903,)),
    "first_1024_segment_radius": (2049, 3, 1, 100.44434, 2.0, 0.5, (904,)),
    "maximum_radius_four_lobes": (1100, 2, 4, 21.333311, 1.0, 0.5, (128, 256, 512, 1024)),
    "exactly_one_full_chunk": (70, 2, 2, 26.501, 0.5, 0.3, (160, 319)),
    "one_chunk_and_a_sliver": (70, 2, 3, 11.334, 0.5, 0.3, (69, 137, 273)),
}


def seam_spikes(hdr, cols):
    """bright pixels of two different colours on both sides of every segment boundary and in the last column: a halo staged from the
    wrong place moves bytes.  They are of moderate size and in the even rows only, and the odd rows' pixels there are dim: beside and
    under a spike the tone map is far from saturation, so that a segment of a single pixel shows a shifted halo too"""
    for i, x in enumerate(cols):
        hdr[0::2, x, :3] = (30.0, 2.0, 0.5) if i % 2 == 0 else (0.4, 15.0, 6.0)
        hdr[1::2, x, :3] = (0.25, 0.5, 0.125)
    return hdr


@pytest.mark.parametrize("name", list(GEOMETRY_CASES))
def test_full_size_launch_geometry_matches_the_restatement(ctx, po, name):
    """multi-segment rows (x0 > 0, halos out of the neighbouring segments, a last segment of one pixel, both segment sizes) and tap
    tables of one chunk exactly, one chunk and one tap, and five chunks: byte for byte the restatement, which knows no segments"""
    import post_geometry as pg
    rrt, _ = ctx
    w, h, lobes, radius, threshold, intensity, radii = GEOMETRY_CASES[name]
    g = rrt.GlowSettings(lobes=lobes, radius=radius, threshold=threshold, intensity=intensity)
    assert tuple((t.size - 1) // 2 for t in glow_ref.lobe_taps(rrt, g, h)) == radii, name     # the planner's R, from its taps
    seams = pg.glow_seams(w, radii[-1])
    rng = np.random.default_rng(w * 1000 + h)
    hdr = seam_spikes(synthetic_hdr(rng, w, h), seams)
    got = glow(rrt, _device_hdr(hdr), w, h, g)
    want = expected(po, rrt, hdr, g)
    assert np.array_equal(got, want), (name, int((got != want).any(-1).sum()), np.flatnonzero((got != want).any((0, 2)))[:8])
    plain = tone_map(po, hdr[..., :3])
    assert not np.array_equal(got, plain)
    for x in seams:                                             # the seams are lit: the glow moves bytes around every boundary
        lo, hi = max(x - 2, 0), min(x + 3, w)
        assert not np.array_equal(want[:, lo:hi], plain[:, lo:hi]), (name, x)


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


DRIVER_CASES = [  # (the mode's arguments, w, h, --glow, --glow-radius, --glow-lobes)
    (["--supersample", "2"], 96, 54, 0.5, 0.01, 3),
    (["--motion-blur", "2"], 96, 54, 0.5, 0.01, 3),
    (["--supersample", "1"], 2064, 16, 0.25, 0.1, 3),       # two glow_hpass segments (2048 + 16), R = 5, 10, 20: the drivers' own scratch
]


@pytest.mark.parametrize("mode", DRIVER_CASES)
def test_drivers_write_the_glowed_frames(ctx, tmp_path, mode):
    """rrt_headless and headless.py --glow: the same file, the summary's glow settings, and every frame == the library's _ss /
    _mb launch at the driver's clock and CameraPath(0)'s cameras, then rrt_launch_glow"""
    mode, w, h, intensity, radius, lobes = mode
    import torch
    from relativisticraytracer_amd import camera_paths as cp
    rrt, tex = ctx
    args = ["--width", str(w), "--height", str(h), "--frames", "3", "--path", "0", "--spin", "0.9", "--all-effects",
            "--glow", str(intensity), "--glow-threshold", "0.2", "--glow-radius", str(radius), "--glow-lobes", str(lobes)] + mode
    meta, meta_p, a = run_drivers(tmp_path, args)
    assert meta["glow"] == {"radius": radius, "lobes": lobes, "threshold": 0.2, "intensity": intensity}, meta
    meta = meta_p
    assert meta["glow"]["lobes"] == lobes and abs(meta["glow"]["intensity"] - intensity) < 1e-7 and meta["tile_order"] is None, meta
    data = np.fromfile(a, np.uint8).reshape(3, h, w, 4)
    path = cp.CameraPath(0)
    fx = rrt.CameraEffects(useChromaticAberration=True)
    prm = rrt.RenderParams(spin=0.9)
    g = rrt.GlowSettings(lobes=lobes, radius=radius, threshold=0.2, intensity=intensity)
    n_visible = 0
    for k in (1, 2, 3):
        if mode[0] == "--supersample":
            st, pt = cp.recording_clock(k, 24)
            plain, hdr = render_ss(rrt, tex, w, h, int(mode[1]), st, path.camera_at(pt), fx, prm)
        else:
            st, pt = cp.motion_clock(k, 24, 0.5, 2)
            plain, hdr = render_mb(rrt, tex, w, h, 1, st, [path.camera_at(p) for p in pt], fx, prm)
        assert np.array_equal(glow(rrt, _device_hdr(hdr), w, h, g), data[k - 1]), k
        n_visible += not np.array_equal(plain, data[k - 1])
    assert n_visible > 0
    torch.cuda.synchronize()
