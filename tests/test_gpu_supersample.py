"""s x s supersampled frames (rrt_launch_raymarch_ss*, include/rrt.h) against their definition: the 1x frame of (s w) x (s h),
rendered by the already-pinned debug launch, reduced per s x s block in float32 in the documented order (a pairwise tree over
the sub-samples of a sub-row, then over the row sums, times 1/s^2) and tone-mapped by the portable exp the 1x path is pinned to.
HDR bit for bit, RGBA8 byte for byte.  torch is only the device-memory plumbing."""

import numpy as np
import pytest

from conftest import same_bits
from gpu_util import _host, _zeros, ctx, run_drivers
from sampled_util import check_parity_ss as check_parity, render_1x, render_ss, scene

pytestmark = pytest.mark.gpu


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
    from relativisticraytracer_amd import camera_paths as cp
    rrt, tex = ctx
    w, h = 96, 54
    args = ["--width", str(w), "--height", str(h), "--frames", "3", "--path", "0", "--spin", "0.9", "--all-effects", "--supersample", "2"]
    meta_c, meta, a = run_drivers(tmp_path, args)
    assert meta_c["supersample"] == 2
    assert meta["supersample"] == 2 and meta["tile_order"] is None
    data = np.fromfile(a, np.uint8).reshape(3, h, w, 4)
    path = cp.CameraPath(0)
    fx = rrt.CameraEffects(useChromaticAberration=True)
    for k in (1, 2, 3):
        st, pt = cp.recording_clock(k)
        buf = _zeros(h * w * 4, torch.uint8)
        rrt.launch_raymarch_ss(buf, w, h, 2, st, path.camera_at(pt), tex, fx, rrt.RenderParams(spin=0.9))
        assert np.array_equal(_host(buf, (h, w, 4)), data[k - 1]), k
