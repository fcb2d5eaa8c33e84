"""s x s supersampled frames (rrt_launch_raymarch_ss*, include/rrt.h) against their definition: the 1x frame of (s w) x (s h),
rendered by the already-pinned debug launch, reduced per s x s block in float32 in the documented order (a pairwise tree over
the sub-samples of a sub-row, then over the row sums, times 1/s^2) and tone-mapped by the portable exp the 1x path is pinned to.
HDR bit for bit, RGBA8 byte for byte.  torch is only the device-memory plumbing."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import same_bits

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


def _zeros(n, dtype):
    import torch
    return torch.zeros(n, dtype=dtype, device="cuda")


def _host(t, shape):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().reshape(shape)


def render_ss(rrt, tex, w, h, s, t, cam, fx, prm):
    """the supersampled frame: (rgba8, hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    rrt.launch_raymarch_ss(out, w, h, s, t, cam, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def render_1x(rrt, tex, w, h, t, cam, fx, prm):
    """the 1x frame through the debug launch: (rgba8, post-FX hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    rrt.launch_raymarch_debug(out, w, h, t, cam, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def _tree(parts):
    """pairwise sum in natural order: ((p0 + p1) + (p2 + p3)) ..."""
    while len(parts) > 1:
        parts = [parts[k] + parts[k + 1] for k in range(0, len(parts), 2)]
    return parts[0]


def expected_mean(big_hdr, w, h, s):
    """the mean HDR of every s x s block of the (s h) x (s w) frame's HDR (bottom-up in, bottom-up out), in the order of the
    contract: within each sub-row j over i, then over the row sums, then * 1/s^2"""
    td = np.ascontiguousarray(big_hdr[::-1, :, :3], dtype=np.float32)      # top-down: row s y + j, column s x + i
    b = td.reshape(h, s, w, s, 3)
    rows = [_tree([b[:, j, :, i] for i in range(s)]) for j in range(s)]
    mean = _tree(rows) * np.float32(1.0 / (s * s))
    assert mean.dtype == np.float32
    return mean[::-1]


def tone_map(po, mean):
    """(uint8)(int)((1 - exp(-mean * 0.8f)) * 255) with the portable exp (raymarcher.cu:164-173, kExposure = 0.8f)"""
    x = (-mean).astype(np.float32) * np.float32(0.8)
    e = po.math_fn(0, po.MATH_PORTABLE, x.ravel()).reshape(x.shape)
    v = (np.float32(1.0) - e) * np.float32(255.0)
    rgb = (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)
    return np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def scene(rrt, rng, case, all_fx=False):
    """a tests/scene_gen.py scene made ragged for every s (odd w and h), volumetrics on and off by turns"""
    from scene_gen import random_scene
    sc = random_scene(rng, case)
    sc["w"] |= 1
    sc["h"] |= 1
    sc["vol"] = 0 if case % 3 == 2 else 1
    f = sc["fx"]
    on = lambda k: True if all_fx else bool(f[k])
    fx = rrt.CameraEffects(useBloom=on("use_bloom"), useVignette=on("use_vignette"), useChromaticAberration=on("use_ca"),
                           useLensDistortion=on("use_lens"), bloomThreshold=f["bloom_threshold"], bloomIntensity=f["bloom_intensity"],
                           vignetteIntensity=f["vignette_intensity"], caAmount=f["ca_amount"] if not all_fx else max(f["ca_amount"], 0.004),
                           distortionAmount=f["distortion_amount"])
    a = sc["cam"]
    return sc, rrt.CameraState(a[0], a[1], a[2], a[3]), fx


def check_parity(po, rrt, tex, w, h, s, t, cam, fx, prm, what):
    big8, big_hdr = render_1x(rrt, tex, s * w, s * h, t, cam, fx, prm)
    got8, got_hdr = render_ss(rrt, tex, w, h, s, t, cam, fx, prm)
    mean = expected_mean(big_hdr, w, h, s)
    assert np.isfinite(mean).all(), what
    assert same_bits(got_hdr[..., :3], mean), (what, int((got_hdr[..., :3] != mean).sum()))
    assert np.all(got_hdr[..., 3] == 1.0), what
    want8 = tone_map(po, mean)
    assert np.array_equal(got8, want8), (what, int((got8 != want8).any(-1).sum()))
    return got8, big8


def test_s1_is_the_1x_frame(ctx, po):
    """s = 1: the bytes of rrt_launch_raymarch and the d_hdr of the debug launch, strict and FMAD"""
    import torch
    rrt, tex = ctx
    rng = np.random.default_rng(20261015)
    for case in range(6):
        sc, cam, fx = scene(rrt, rng, case, all_fx=case == 0)
        w, h = sc["w"], sc["h"]
        for arith in (0, 2):
            prm = rrt.RenderParams(spin=sc["spin"], volumetrics=sc["vol"], arith_mode=arith)
            ref = _zeros(h * w * 4, torch.uint8)
            rrt.launch_raymarch(ref, w, h, sc["t"], cam, tex, fx, prm)
            ref8 = _host(ref, (h, w, 4))
            _, dbg_hdr = render_1x(rrt, tex, w, h, sc["t"], cam, fx, prm)
            got8, got_hdr = render_ss(rrt, tex, w, h, 1, sc["t"], cam, fx, prm)
            assert np.array_equal(got8, ref8), (case, arith)
            assert same_bits(got_hdr, dbg_hdr), (case, arith)


def test_virtual_frame_parity_on_random_scenes(ctx, po):
    """s = 2 and 4 on 8 ragged scenes (media on and off, every effect on in some, strict and FMAD), s = 8 on 2 of them"""
    rrt, tex = ctx
    rng = np.random.default_rng(355)
    covered = set()
    for case in range(8):
        sc, cam, fx = scene(rrt, rng, case, all_fx=case in (1, 4))
        arith = 2 if case % 2 else 0
        prm = rrt.RenderParams(spin=sc["spin"], volumetrics=sc["vol"], arith_mode=arith)
        for s in ((2, 4, 8) if case in (3, 6) else (2, 4)):
            got8, _ = check_parity(po, rrt, tex, sc["w"], sc["h"], s, sc["t"], cam, fx, prm, (case, s, arith))
            covered.add((s, arith, sc["vol"]))
    assert {(2, 0, 1), (2, 2, 1), (2, 0, 0), (2, 2, 0), (4, 0, 1), (4, 2, 1)} <= covered, covered
    assert any(k[0] == 8 for k in covered)


def test_virtual_frame_parity_480x270_with_noise_table(ctx, po):
    """the reference's default view at 480x270, s = 4 (the virtual frame is 1920x1080), media through the lattice-hash tables"""
    rrt, tex = ctx
    nt = rrt.NoiseTable(4.0)
    try:
        cam = rrt.CameraState.default()
        fx = rrt.CameraEffects(useChromaticAberration=True)
        prm = rrt.RenderParams(spin=0.9, noise_table=nt.id)
        got8, big8 = check_parity(po, rrt, tex, 480, 270, 4, 1.0, cam, fx, prm, "480x270 s4 table")
        assert got8[..., :3].std() > 5.0                                # a real picture, not a blank frame
    finally:
        nt.destroy()


def test_nudged_primary_rays_hash_the_virtual_pixel(ctx, po):
    """nudge_ulps = 3: the sub-samples are nudged as the big frame's pixels are"""
    rrt, tex = ctx
    rng = np.random.default_rng(7)
    for case in range(3):
        sc, cam, fx = scene(rrt, rng, case)
        for s in (2, 4):
            prm = rrt.RenderParams(spin=sc["spin"], volumetrics=sc["vol"], arith_mode=2 * (case % 2), nudge_ulps=3, nudge_seed=11 + case)
            check_parity(po, rrt, tex, sc["w"], sc["h"], s, sc["t"], cam, fx, prm, ("nudge", case, s))


def test_tile_shards_assemble_to_the_full_supersampled_frame(ctx):
    import torch
    rrt, tex = ctx
    w, h = 77, 45
    cam = rrt.CameraState.default()
    fx = rrt.CameraEffects(useChromaticAberration=True)
    prm = rrt.RenderParams(spin=0.9)
    for s in (2, 4):
        full, _ = render_ss(rrt, tex, w, h, s, 1.0, cam, fx, prm)
        for n in (1, 3, 8):
            for tr in (16, 5):
                if s == 4 and (n, tr) != (3, 5):
                    continue
                rows = [rrt.tile_shard_rows(h, tr, k, n) for k in range(n)]
                stride = ((max(rows) * w * 4) + 255) & ~255
                tiles = _zeros(stride * n, torch.uint8)
                for k in range(n):
                    rrt.launch_raymarch_ss_tiles(tiles.data_ptr() + k * stride, w, h, s, tr, k, n, 1.0, cam, tex, fx, prm)
                frame = _zeros(h * w * 4, torch.uint8)
                rrt.assemble_all_tiles(frame, tiles, stride, w, h, tr, n)
                assert np.array_equal(_host(frame, (h, w, 4)), full), (s, n, tr)


def test_path_and_order_params_are_ignored(ctx):
    """a workspace, a path policy, pool rounds, chains and a tile-order object change nothing and are not touched"""
    rrt, tex = ctx
    w, h = 101, 57
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
    ref, ref_hdr = render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, rrt.RenderParams(spin=0.9))
    ws, order = rrt.Workspace(64 << 20), rrt.TileOrder()
    try:
        prm = rrt.RenderParams(spin=0.9, workspace=ws.id, tile_order=order.id, path_policy=2, pool_rounds=3, pass_chains=2)
        for _ in range(2):
            got, got_hdr = render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, prm)
            assert np.array_equal(got, ref) and same_bits(got_hdr, ref_hdr)
        assert order.info()["launches"] == 0                            # nothing recorded through the order object
    finally:
        ws.destroy()
        order.destroy()


def test_graph_capture_and_side_stream(ctx):
    """no memset, no synchronisation: a launch runs on a side stream and can be captured into a graph and replayed"""
    import torch
    rrt, tex = ctx
    w, h = 64, 36
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=0.9)
    ref, _ = render_ss(rrt, tex, w, h, 2, 1.0, cam, fx, prm)
    side = torch.cuda.Stream()
    a = _zeros(h * w * 4, torch.uint8)
    rrt.launch_raymarch_ss(a, w, h, 2, 1.0, cam, tex, fx, prm, stream=side)
    side.synchronize()
    assert np.array_equal(a.cpu().numpy().reshape(h, w, 4), ref)
    b = _zeros(h * w * 4, torch.uint8)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch_ss(b, w, h, 2, 1.0, cam, tex, fx, prm)
    for _ in range(2):
        b.zero_()
        graph.replay()
        assert np.array_equal(_host(b, (h, w, 4)), ref)


def test_drivers_write_the_supersampled_frames(ctx, tmp_path):
    """rrt_headless --supersample 2 --path 0: three frames == launch_raymarch_ss with the driver's cameras and clock; headless.py
    writes the same file"""
    import torch
    from relativisticraytracer_amd import build
    from relativisticraytracer_amd import camera_paths as cp
    rrt, tex = ctx
    exe = build.build_headless()
    w, h = 96, 54
    a, b = tmp_path / "cpp.rgba", tmp_path / "py.rgba"
    args = ["--width", str(w), "--height", str(h), "--frames", "3", "--path", "0", "--spin", "0.9", "--all-effects", "--supersample", "2"]
    r = subprocess.run([exe] + args + ["--out", str(a)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["supersample"] == 2
    r = subprocess.run([sys.executable, "-m", "relativisticraytracer_amd.headless"] + args + ["--out", str(b)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = json.loads(r.stdout.strip().splitlines()[-1])
    assert meta["supersample"] == 2 and meta["tile_order"] is None
    data = np.fromfile(a, np.uint8).reshape(3, h, w, 4)
    assert open(a, "rb").read() == open(b, "rb").read()
    path = cp.CameraPath(0)
    fx = rrt.CameraEffects(useChromaticAberration=True)
    for k in (1, 2, 3):
        st, pt = cp.recording_clock(k)
        buf = _zeros(h * w * 4, torch.uint8)
        rrt.launch_raymarch_ss(buf, w, h, 2, st, path.camera_at(pt), tex, fx, rrt.RenderParams(spin=0.9))
        assert np.array_equal(_host(buf, (h, w, 4)), data[k - 1]), k
