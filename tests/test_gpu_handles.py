"""The five kinds of handle (sky, workspace, noise table, tile map, tile order; csrc/rrt_handles.h) on the device: a launch through
each object gives the bytes of the plain single-kernel launch (which the project documents every path to be byte-identical to), and
after the object's destroy the same launch is RRT_ERR_BAD_HANDLE (4) and touches neither rrt_last_hip_error() nor the output.

The frame is 64 x 32: eight 8 x 8 wave tiles in x and four dispatch rows in y, so the tile order, the row maps and the tile map all have more
than one tile.  Nothing is destroyed while work that reads it is in flight (every destroy follows a synchronise): these tests check
the bookkeeping, not races.  The table itself is tested on the host (tests/test_handles_host.py)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, T, SPIN = 64, 32, 1.0, 0.9
SENTINEL = 0x5A
SINGLE, THREE_PASS = 1, 2          # rrt_params.path_policy
BAD_HANDLE = 4
# the three-pass path wants its bookkeeping plus 1024 sample blocks of 10 368 B (10.1 MiB) in the workspace: 11 MiB is the
# smallest whole number of MiB that takes it at this frame (rrt_workspace_rounds confirms below)
WS_BYTES = 11 << 20


@pytest.fixture(scope="module")
def scene():
    """(rrt, lib, camera, effects, sky texels, a sky, the reference bytes): the plain single-kernel frame, rendered once"""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    texels = np.array([[[255, 40, 10, 255], [20, 200, 60, 255]], [[30, 60, 250, 255], [240, 240, 90, 255]]], np.uint8)   # 2 x 2
    tex = rrt.SkyTexture(texels)
    cam, fx = rrt.CameraState.default(), rrt.CameraEffects()
    out = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(out, W, H, T, cam, tex, fx, rrt.RenderParams(spin=SPIN, path_policy=SINGLE))
    torch.cuda.synchronize()
    ref = out.cpu().numpy().copy()
    assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 16          # a picture, not a flat frame
    yield rrt, _lib.load(), cam, fx, texels, tex, ref
    tex.destroy()


def _launch(scene, prm, sky=None):
    """rrt_launch_raymarch into a buffer full of SENTINEL -> (status, bytes, rrt_last_hip_error before, after)"""
    import torch
    rrt, lib, cam, fx, _, tex, _ = scene
    out = torch.full((H * W * 4,), SENTINEL, dtype=torch.uint8, device="cuda")
    before = lib.rrt_last_hip_error()
    rc = lib.rrt_launch_raymarch(C.c_void_p(out.data_ptr()), W, H, T, C.byref(cam), tex.handle if sky is None else sky, C.byref(fx),
                                 C.byref(prm), None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), before, lib.rrt_last_hip_error()


def _refused(scene, prm, sky=None):
    rc, got, before, after = _launch(scene, prm, sky)
    assert rc == BAD_HANDLE and before == after and np.all(got == SENTINEL)


def _plain_frame_still_renders(scene):
    rrt, _, _, _, _, _, ref = scene
    rc, got, _, _ = _launch(scene, rrt.RenderParams(spin=SPIN, path_policy=SINGLE))
    assert rc == 0 and np.array_equal(got, ref)


def test_workspace(scene):
    import torch
    rrt, lib, _, _, _, _, ref = scene
    ws = rrt.Workspace(WS_BYTES)
    prm = rrt.RenderParams(spin=SPIN, workspace=ws.id, path_policy=THREE_PASS)
    rc, got, _, _ = _launch(scene, prm)
    assert rc == 0 and np.array_equal(got, ref)
    st = ws.stats()
    assert st["rounds_enqueued"] >= 1 and st["overflow_waves"] == 0          # the three-pass path, not its fall-back
    torch.cuda.synchronize()
    assert lib.rrt_workspace_destroy(ws.id) == 0 and lib.rrt_workspace_destroy(ws.id) == BAD_HANDLE
    _refused(scene, prm)
    assert lib.rrt_workspace_stats(ws.id, None, None) == BAD_HANDLE and lib.rrt_workspace_rounds(ws.id, None, None, None, None) == BAD_HANDLE
    assert lib.rrt_workspace_read(ws.id, 0, 8, None) == BAD_HANDLE
    ws.id = 0
    _plain_frame_still_renders(scene)


def test_noise_table(scene):
    import torch
    rrt, lib, _, _, _, _, ref = scene
    nt = rrt.NoiseTable.window(T - 0.5, T + 0.5)
    assert nt.covers(T) and nt.info()["device"] == torch.cuda.current_device()
    prm = rrt.RenderParams(spin=SPIN, noise_table=nt.id, path_policy=SINGLE)
    rc, got, _, _ = _launch(scene, prm)
    assert rc == 0 and np.array_equal(got, ref)
    torch.cuda.synchronize()
    assert lib.rrt_noise_table_destroy(nt.id) == 0 and lib.rrt_noise_table_destroy(nt.id) == BAD_HANDLE
    _refused(scene, prm)
    assert lib.rrt_noise_table_info(nt.id, None, None, None) == BAD_HANDLE
    assert lib.rrt_noise_table_window(nt.id, None, None, None, None) == BAD_HANDLE
    nt.id = 0
    _plain_frame_still_renders(scene)


def test_tile_order(scene):
    import torch
    rrt, lib, _, _, _, _, ref = scene
    order = rrt.TileOrder()
    prm = rrt.RenderParams(spin=SPIN, tile_order=order.id, path_policy=SINGLE)
    for _ in range(2):                                   # the probe's order, then the order the first launch recorded
        rc, got, _, _ = _launch(scene, prm)
        assert rc == 0 and np.array_equal(got, ref)
    info = order.info()
    assert info["launches"] == 2 and info["ordered_launches"] == 1 and info["n_tiles"] == (W // 8) * (H // 8) and order.seeded_launches() == 1
    torch.cuda.synchronize()
    assert lib.rrt_tile_order_destroy(order.id) == 0 and lib.rrt_tile_order_destroy(order.id) == BAD_HANDLE
    for policy in (SINGLE, THREE_PASS, 0):               # whatever path the launch would take
        prm.path_policy = policy
        _refused(scene, prm)
    assert lib.rrt_tile_order_info(order.id, None, None, None, None, None, 0) == BAD_HANDLE
    assert lib.rrt_tile_order_set_seeding(order.id, 0) == BAD_HANDLE and lib.rrt_tile_order_seeded(order.id, None) == BAD_HANDLE
    order.id = 0
    _plain_frame_still_renders(scene)


def test_tile_map(scene):
    import torch
    rrt, lib, cam, fx, _, tex, ref = scene
    tm = rrt.TileMap(H, 8, 2, np.array([0, 1, 1, 0], np.int32))          # two shards, four row tiles
    assert tm.shard_rows(0) == 16 and tm.shard_rows(1) == 16
    stride = tm.max_shard_rows() * W * 4
    tiles = torch.full((2 * stride,), SENTINEL, dtype=torch.uint8, device="cuda")
    frame = torch.zeros(H * W * 4, dtype=torch.uint8, device="cuda")
    prm = rrt.RenderParams(spin=SPIN, path_policy=SINGLE)
    for shard in range(2):
        rrt.launch_raymarch_tilemap(tiles[shard * stride:], W, H, tm, shard, T, cam, tex, fx, prm)
    rrt.assemble_all_tilemap(frame, tiles, stride, W, H, tm)
    torch.cuda.synchronize()
    assert np.array_equal(frame.cpu().numpy(), ref)
    assert lib.rrt_tile_map_destroy(tm.id) == 0 and lib.rrt_tile_map_destroy(tm.id) == BAD_HANDLE
    tiles.fill_(SENTINEL); frame.fill_(SENTINEL)
    before = lib.rrt_last_hip_error()
    args = (W, H, tm.id, 0, T, C.byref(cam), tex.handle, C.byref(fx), C.byref(prm), None)
    assert lib.rrt_launch_raymarch_tilemap(C.c_void_p(tiles.data_ptr()), *args) == BAD_HANDLE
    assert lib.rrt_assemble_all_tilemap(C.c_void_p(frame.data_ptr()), C.c_void_p(tiles.data_ptr()), stride, W, H, tm.id, None) == BAD_HANDLE
    assert lib.rrt_tile_map_shard_rows(tm.id, 0, None, None) == BAD_HANDLE
    torch.cuda.synchronize()
    assert lib.rrt_last_hip_error() == before and bool((tiles == SENTINEL).all()) and bool((frame == SENTINEL).all())
    tm.id = 0
    _plain_frame_still_renders(scene)


def test_sky(scene):
    """a second sky of the same texels renders the same bytes; destroyed, it is refused; its id is never issued again"""
    rrt, lib, _, _, texels, tex, ref = scene
    prm = rrt.RenderParams(spin=SPIN, path_policy=SINGLE)
    sky2 = rrt.SkyTexture(texels)
    assert sky2.handle > tex.handle and sky2.handle >> 48 == 0x5254
    rc, got, _, _ = _launch(scene, prm, sky2.handle)
    assert rc == 0 and np.array_equal(got, ref)
    gone = sky2.handle
    assert lib.rrt_sky_destroy(gone) == 0 and lib.rrt_sky_destroy(gone) == BAD_HANDLE
    sky2.handle = 0
    _refused(scene, prm, gone)
    sky3 = rrt.SkyTexture(texels)
    assert sky3.handle > gone
    rc, got, _, _ = _launch(scene, prm, sky3.handle)
    assert rc == 0 and np.array_equal(got, ref)
    sky3.destroy()
    _plain_frame_still_renders(scene)


def test_which_kinds_a_foreign_device_may_destroy(scene):
    """A tile map and a tile order are destroyed under their own device only (4, and the object is still there afterwards); a sky,
    a workspace and a noise table go from any device.  One GPU here, so the foreign device is rrt_debug_fake_device(), which only
    librrt_hip_test.so has: the whole test talks to that library."""
    import torch
    rrt = scene[0]
    from relativisticraytracer_amd import _lib
    texels = scene[4]
    with _lib.using_test_library() as lib:
        real = torch.cuda.current_device()
        tex, ws, nt = rrt.SkyTexture(texels), rrt.Workspace(WS_BYTES), rrt.NoiseTable.window(T - 0.5, T + 0.5)
        tm, order = rrt.TileMap(H, 8, 2, np.array([0, 1, 1, 0], np.int32)), rrt.TileOrder()
        torch.cuda.synchronize()
        try:
            assert lib.rrt_debug_fake_device(real + 1) == 0
            assert lib.rrt_tile_map_destroy(tm.id) == BAD_HANDLE and lib.rrt_tile_order_destroy(order.id) == BAD_HANDLE
            assert tm.shard_rows(1) == 16 and order.seeded_launches() == 0          # still registered (these two ask no device)
            assert lib.rrt_sky_destroy(tex.handle) == 0 and lib.rrt_workspace_destroy(ws.id) == 0 and lib.rrt_noise_table_destroy(nt.id) == 0
            tex.handle = ws.id = nt.id = 0
            assert lib.rrt_debug_fake_device(-1) == 0
            assert lib.rrt_tile_map_destroy(tm.id) == 0 and lib.rrt_tile_order_destroy(order.id) == 0
            assert lib.rrt_tile_map_destroy(tm.id) == BAD_HANDLE and lib.rrt_tile_order_destroy(order.id) == BAD_HANDLE
            tm.id = order.id = 0
        finally:
            lib.rrt_debug_fake_device(-1)
            for o in (tex, ws, nt, tm, order):
                o.destroy()


def test_an_object_of_the_test_library_is_destroyed_there_from_outside():
    """A handle object remembers the library that made it: a sky and a workspace created inside using_test_library() and destroyed
    after it are gone from the TEST library's registries (its raw destroy says 4), not sent to the product library's, where the
    ids mean nothing or something else.  No kernel is launched."""
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import _lib
    with _lib.using_test_library() as lib:
        tex, ws = rrt.SkyTexture(np.arange(8 * 4 * 4, dtype=np.uint8).reshape(4, 8, 4)), rrt.Workspace(1 << 20)
    handle, wid = tex.handle, ws.id
    assert handle and wid
    tex.destroy()
    ws.destroy()
    assert tex.handle == 0 and ws.id == 0
    assert lib.rrt_sky_destroy(handle) == BAD_HANDLE and lib.rrt_workspace_destroy(wid) == BAD_HANDLE
