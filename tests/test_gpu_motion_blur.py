"""Motion-blurred frames (rrt_launch_raymarch_mb*, include/rrt.h) against their definition: K sub-frames, each the 1x frame of
(s w) x (s h) rendered by the already-pinned debug launch at its own (time, camera), reduced per s x s block in the order of the
supersampled contract, then over k by the same pairwise tree, times 1/(s^2 K), tone-mapped by the portable exp.  HDR bit for bit,
RGBA8 byte for byte.  torch is only the device-memory plumbing."""

import numpy as np
import pytest

from conftest import same_bits
from gpu_util import _host, _zeros, ctx, run_drivers
from sampled_util import check_parity_mb as check_parity, moving_cameras, render_mb, render_ss, scene

pytestmark = pytest.mark.gpu


def test_random_scenes_k4_match_the_definition(ctx, po):
    """K = 4 distinct times and cameras, s = 1 and 2, on ragged scenes (media on and off, strict and FMAD)"""
    rrt, tex = ctx
    rng = np.random.default_rng(2410)
    for case in range(6):
        sc, cam, fx = scene(rrt, rng, case, all_fx=case == 1)
        prm = rrt.RenderParams(spin=sc["spin"], volumetrics=sc["vol"], arith_mode=2 if case % 2 else 0)
        times = [sc["t"] + 0.05 * k for k in range(4)]
        cams = moving_cameras(rrt, sc, 4)
        for s in (1, 2):
            got8 = check_parity(po, rrt, tex, sc["w"], sc["h"], s, times, cams, fx, prm, (case, s))
        if case == 0:
            one8, _ = render_ss(rrt, tex, sc["w"], sc["h"], 2, times[0], cams[0], fx, prm)
            assert not np.array_equal(got8, one8)                        # the blur is visible


def test_identities(ctx):
    """K = 1 is rrt_launch_raymarch_ss; K equal sub-frames are K = 1; s = 1, K = 1 is rrt_launch_raymarch"""
    import torch
    rrt, tex = ctx
    rng = np.random.default_rng(11)
    for case in range(4):
        sc, cam, fx = scene(rrt, rng, case)
        w, h = sc["w"], sc["h"]
        prm = rrt.RenderParams(spin=sc["spin"], volumetrics=sc["vol"], arith_mode=2 * (case % 2))
        for s in (1, 2):
            ref8, ref_hdr = render_ss(rrt, tex, w, h, s, sc["t"], cam, fx, prm)
            for n in (1, 4, 16 if case == 0 else 2):
                got8, got_hdr = render_mb(rrt, tex, w, h, s, [sc["t"]] * n, [cam] * n, fx, prm)
                assert np.array_equal(got8, ref8) and same_bits(got_hdr, ref_hdr), (case, s, n)
        one = _zeros(h * w * 4, torch.uint8)
        rrt.launch_raymarch(one, w, h, sc["t"], cam, tex, fx, prm)
        got8, _ = render_mb(rrt, tex, w, h, 1, [sc["t"]], [cam], fx, prm)
        assert np.array_equal(got8, _host(one, (h, w, 4))), case


def test_noise_table_window(ctx, po):
    """a table whose window holds only some of the sub-times gives the bytes of no table (every sub-frame hashes arithmetically);
    a table that holds all of them gives the same bytes too"""
    rrt, tex = ctx
    w, h = 96, 54
    cam = rrt.CameraState.default()
    fx = rrt.CameraEffects()
    times = [1.0, 1.5, 2.0, 2.5]
    cams = [cam] * 4
    ref8, ref_hdr = render_mb(rrt, tex, w, h, 2, times, cams, fx, rrt.RenderParams(spin=0.9))
    check_parity(po, rrt, tex, w, h, 2, times, cams, fx, rrt.RenderParams(spin=0.9), "no table")
    for t0, t1 in ((0.0, 1.7), (1.2, 3.0), (0.0, 4.0)):
        nt = rrt.NoiseTable.window(t0, t1, 0)
        try:
            got8, got_hdr = render_mb(rrt, tex, w, h, 2, times, cams, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
            assert np.array_equal(got8, ref8) and same_bits(got_hdr, ref_hdr), (t0, t1)
        finally:
            nt.destroy()


def test_tile_shards_assemble_to_the_full_frame(ctx):
    import torch
    rrt, tex = ctx
    w, h = 77, 45
    cams = [rrt.CameraState.from_angles((0.5 * k, 10.0, -60.0), 0.3 * k, -10.0) for k in range(4)]
    fx = rrt.CameraEffects(useChromaticAberration=True)
    prm = rrt.RenderParams(spin=0.9)
    times = [1.0, 1.02, 1.04, 1.06]
    for s in (1, 2):
        full, _ = render_mb(rrt, tex, w, h, s, times, cams, fx, prm)
        for n, tr in ((3, 16), (8, 5)):
            rows = [rrt.tile_shard_rows(h, tr, k, n) for k in range(n)]
            stride = ((max(rows) * w * 4) + 255) & ~255
            tiles = _zeros(stride * n, torch.uint8)
            for k in range(n):
                rrt.launch_raymarch_mb_tiles(tiles.data_ptr() + k * stride, w, h, s, tr, k, n, times, cams, tex, fx, prm)
            frame = _zeros(h * w * 4, torch.uint8)
            rrt.assemble_all_tiles(frame, tiles, stride, w, h, tr, n)
            assert np.array_equal(_host(frame, (h, w, 4)), full), (s, n, tr)


def test_ignored_params_and_graph_capture(ctx):
    """a workspace, a path policy, pool rounds, chains and a tile-order object change nothing; a launch on a side stream and a
    captured graph's replays give the same bytes"""
    import torch
    rrt, tex = ctx
    w, h = 64, 36
    cams = [rrt.CameraState.from_angles((0.0, 10.0 + 0.2 * k, -60.0), 0.0, -10.0) for k in range(4)]
    times = [1.0, 1.01, 1.02, 1.03]
    fx = rrt.CameraEffects()
    ref, ref_hdr = render_mb(rrt, tex, w, h, 2, times, cams, fx, rrt.RenderParams(spin=0.9))
    ws, order = rrt.Workspace(64 << 20), rrt.TileOrder()
    try:
        prm = rrt.RenderParams(spin=0.9, workspace=ws.id, tile_order=order.id, path_policy=2, pool_rounds=3, pass_chains=2)
        got, got_hdr = render_mb(rrt, tex, w, h, 2, times, cams, fx, prm)
        assert np.array_equal(got, ref) and same_bits(got_hdr, ref_hdr)
        assert order.info()["launches"] == 0
    finally:
        ws.destroy()
        order.destroy()
    prm = rrt.RenderParams(spin=0.9)
    side = torch.cuda.Stream()
    a = _zeros(h * w * 4, torch.uint8)
    rrt.launch_raymarch_mb(a, w, h, 2, times, cams, tex, fx, prm, stream=side)
    side.synchronize()
    assert np.array_equal(a.cpu().numpy().reshape(h, w, 4), ref)
    b = _zeros(h * w * 4, torch.uint8)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch_mb(b, w, h, 2, times, cams, tex, fx, prm)
    for _ in range(2):
        b.zero_()
        graph.replay()
        assert np.array_equal(_host(b, (h, w, 4)), ref)


@pytest.mark.parametrize("ss", [1, 2])
def test_drivers_write_the_blurred_frames(ctx, tmp_path, ss):
    """rrt_headless and headless.py --path 0 --motion-blur 4 --shutter 0.5: the same file, the summary keys, and every frame ==
    launch_raymarch_mb at motion_clock's times with CameraPath(0)'s cameras"""
    import torch
    from relativisticraytracer_amd import camera_paths as cp
    rrt, tex = ctx
    w, h = 96, 54
    args = ["--width", str(w), "--height", str(h), "--frames", "3", "--path", "0", "--spin", "0.9", "--all-effects",
            "--motion-blur", "4", "--shutter", "0.5"] + (["--supersample", str(ss)] if ss > 1 else [])
    meta, meta_p, a = run_drivers(tmp_path, args)
    assert meta["motion_blur"] == 4 and meta["shutter"] == 0.5 and meta["supersample"] == ss, meta
    meta = meta_p
    assert meta["motion_blur"] == 4 and meta["shutter"] == 0.5 and meta["supersample"] == ss and meta["tile_order"] is None, meta
    data = np.fromfile(a, np.uint8).reshape(3, h, w, 4)
    path = cp.CameraPath(0)
    fx = rrt.CameraEffects(useChromaticAberration=True)
    for k in (1, 2, 3):
        st, pt = cp.motion_clock(k, 24, 0.5, 4)
        buf = _zeros(h * w * 4, torch.uint8)
        rrt.launch_raymarch_mb(buf, w, h, ss, st, [path.camera_at(p) for p in pt], tex, fx, rrt.RenderParams(spin=0.9))
        assert np.array_equal(_host(buf, (h, w, 4)), data[k - 1]), k
