"""Frame-level parity of the HIP path (through the C ABI) against the CPU oracle.

Bars (north_star: "within 1e-4 relative per channel"), round 3: set to the MEASURED class, not a loose envelope --
  * vs the oracle in PORTABLE math mode (same csrc/rrt_math.h on both sides): RGBA8 bytes identical, float RGB /
    per-ray state bit-identical -- for the debug instantiation (which exposes the per-ray state) AND for the
    production instantiation the bench times (bytes);
  * vs the oracle in LIBM mode and vs the REFERENCE's own kernel body (glibc transcendentals, the independent
    checks): step counts identical; RGBA8 within 1 LSB on <= 1e-4 of the bytes of a fixture (measured: 0 to 2 bytes
    per frame) and <= 2e-5 at 4K / 1080p; float RGB within 1e-4 relative (+1e-5 absolute floor for near-black
    pixels) on EVERY pixel whose hard-gate decisions (raymarcher.cu:71,76,91; densities.h:85; bloom threshold; the
    sky filter's quantised weights) agree between the two math libraries -- tests/test_gate_accounting.py::account
    recomputes the gate logs here -- and the flipped ones are counted (<= 2 per fixture frame).
"""
import os

import numpy as np
import pytest

from conftest import same_bits

pytestmark = pytest.mark.gpu

CASES = {   # name -> (w, h, spin, vol, (pos, yaw, pitch), time, effect overrides)  == tests/golden/make_golden.py
    "G1": (128, 128, 0.0, 1, ((0.0, 10.0, -60.0), 0.0, -10.0), 1.0, {}),
    "G2": (64, 36, 0.9, 0, ((0.0, 10.0, -60.0), 0.0, -10.0), 1.0, {}),
    "G3": (64, 36, 0.9, 1, ((0.0, 10.0, -60.0), 0.0, -10.0), 1.0, {}),
    "G4": (64, 36, 0.99, 1, ((0.0, 10.0, -60.0), 0.0, -10.0), 1.0, {}),
    "G5": (64, 36, 0.9, 1, ((35.0, 0.8, 10.0), -106.0, -1.2), 12.5, {"useChromaticAberration": True}),
}


@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import gpu_util
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    yield gpu_util, rrt, tex
    tex.destroy()


def _render(ctx, name, **kw):
    g, rrt, tex = ctx
    w, h, spin, vol, camspec, t, fxkw = CASES[name]
    cam = rrt.CameraState.from_angles(*camspec)
    return g.render_gpu(w, h, spin, vol, cam, t, tex, fx=rrt.CameraEffects(**fxkw), **kw), cam


def _gate_flips(po, sky, cam, ofx, prm_kw, t, w, h):
    """Per pixel (h, w), in the frame's bottom-up storage order: do the hard-gate decisions of the two math
    libraries differ for this ray?  (CPU: tests/test_gate_accounting.py::account)"""
    from test_gate_accounting import account
    a = cam.as_array()
    acc = account(po, sky, po.camera(a[0], a[1], a[2], a[3]), ofx, prm_kw, t, w, h)
    assert acc["forced_ok"].all()                                  # gates aligned: the libraries agree to 1e-4 everywhere
    return acc["flipped"].reshape(h, w)[::-1]                      # account() lists rays top-down


@pytest.mark.parametrize("name", list(CASES))
def test_golden_frames_byte_identical(ctx, frames_gold, name):
    r, cam = _render(ctx, name)
    assert np.array_equal(cam.as_array(), frames_gold[f"{name}_camera"])
    assert np.array_equal(r["rgba8"], frames_gold[f"{name}_portable_rgba8"])
    # the PRODUCTION instantiation (debug=False: the kernel the bench times), and the same through the noise tables
    g, rrt, tex = ctx
    prod, _ = _render(ctx, name, debug=False)
    assert np.array_equal(prod["rgba8"], frames_gold[f"{name}_portable_rgba8"])
    nt = rrt.NoiseTable(16.0)
    try:
        prod, _ = _render(ctx, name, debug=False, noise_table=nt.id)
        assert np.array_equal(prod["rgba8"], frames_gold[f"{name}_portable_rgba8"])
    finally:
        nt.destroy()
    assert np.array_equal(r["steps"], frames_gold[f"{name}_portable_steps"].astype(np.int32))
    assert np.array_equal(r["hit"], frames_gold[f"{name}_portable_hit"].astype(np.int32))
    if name != "G1":
        assert same_bits(r["ldr"], frames_gold[f"{name}_portable_ldr"])
        assert same_bits(r["pos"], frames_gold[f"{name}_portable_pos"])
        assert same_bits(r["vel"], frames_gold[f"{name}_portable_vel"])
        assert same_bits(r["rad"], frames_gold[f"{name}_portable_rad"])


@pytest.mark.parametrize("name", list(CASES))
def test_golden_frames_within_tolerance_of_libm_oracle(ctx, frames_gold, po, sky, name):
    g, rrt, tex = ctx
    r, cam = _render(ctx, name)
    # geodesic state involves only + - * / sqrt: identical in both oracle modes and on the GPU
    assert np.array_equal(r["steps"], frames_gold[f"{name}_libm_steps"].astype(np.int32))
    assert np.array_equal(r["hit"], frames_gold[f"{name}_libm_hit"].astype(np.int32))
    du8 = np.abs(r["rgba8"].astype(int) - frames_gold[f"{name}_libm_rgba8"].astype(int))
    assert du8.max() <= 1
    assert (du8 > 0).sum() <= 1e-4 * du8.size, int((du8 > 0).sum())     # measured: 2 bytes of G1's 65 536, 0 elsewhere
    if name != "G1":
        w, h, spin, vol, camspec, t, fxkw = CASES[name]
        ref = frames_gold[f"{name}_libm_ldr"][..., :3]
        got = r["ldr"][..., :3]
        ok = (np.abs(got - ref) <= 1e-4 * np.abs(ref) + 1e-5).all(axis=2)
        flips = _gate_flips(po, sky, cam, po.default_effects(use_ca=int(fxkw.get("useChromaticAberration", False))),
                            {"spin": spin, "volumetrics": vol}, t, w, h)
        assert (ok | flips).all(), "a pixel outside 1e-4 whose gate decisions agree in both math libraries"
        assert (~ok).sum() <= 2, int((~ok).sum())                           # measured: 0 on every fixture
        assert np.abs(got - ref)[ok].max() <= 5e-5                          # measured 1.2e-5


def test_live_oracle_random_view(ctx, po, sky):
    """A view that is in no fixture: oracle rendered live, both math modes."""
    g, rrt, tex = ctx
    w, h = 96, 54
    cam = rrt.CameraState.from_angles((15.0, 3.0, -30.0), -26.6, -5.1)       # a keyframe of path 1
    fx = rrt.CameraEffects(useChromaticAberration=True, caAmount=0.004)
    r = g.render_gpu(w, h, 0.9, 1, cam, 6.0, tex, fx=fx)
    a = cam.as_array()
    ofx = po.default_effects(use_ca=1, ca_amount=0.004)
    ocam = po.camera(a[0], a[1], a[2], a[3])
    o = po.render(ocam, ofx, po.default_params(spin=0.9, math_mode=po.MATH_PORTABLE), 6.0, w, h, sky,
                  want=("rgba8", "ldr", "hdr", "diag"))
    assert np.array_equal(r["rgba8"], o["rgba8"])
    assert same_bits(r["hdr"], o["hdr"]) and same_bits(r["ldr"], o["ldr"])
    assert np.array_equal(r["steps"], o["steps"])
    prod = g.render_gpu(w, h, 0.9, 1, cam, 6.0, tex, fx=fx, debug=False)            # the production instantiation
    assert np.array_equal(prod["rgba8"], o["rgba8"])
    # RRT_ARITH_FMAD against the oracle's FMAD mode (the fixed fused tree): the same equalities
    of = po.render(ocam, ofx, po.default_params(spin=0.9, math_mode=po.MATH_PORTABLE, arith_mode=po.ARITH_FMAD), 6.0, w, h, sky,
                   want=("rgba8", "ldr", "hdr", "diag"))
    assert not np.array_equal(of["pos"], o["pos"])                                   # another frame than the strict one
    rf = g.render_gpu(w, h, 0.9, 1, cam, 6.0, tex, fx=fx, arith_mode=2)
    assert np.array_equal(rf["rgba8"], of["rgba8"])
    assert same_bits(rf["hdr"], of["hdr"]) and same_bits(rf["ldr"], of["ldr"])
    assert np.array_equal(rf["steps"], of["steps"]) and same_bits(rf["pos"], of["pos"]) and same_bits(rf["vel"], of["vel"])
    prod = g.render_gpu(w, h, 0.9, 1, cam, 6.0, tex, fx=fx, debug=False, arith_mode=2)
    assert np.array_equal(prod["rgba8"], of["rgba8"])
    ol = po.render(ocam, ofx, po.default_params(spin=0.9, math_mode=po.MATH_LIBM), 6.0, w, h, sky,
                   want=("rgba8", "ldr"))
    ok = (np.abs(r["ldr"][..., :3] - ol["ldr"][..., :3]) <= 1e-4 * np.abs(ol["ldr"][..., :3]) + 1e-5).all(axis=2)
    flips = _gate_flips(po, sky, cam, ofx, {"spin": 0.9}, 6.0, w, h)
    assert (ok | flips).all() and (~ok).sum() <= 2                                   # measured: one flipped ray
    d = np.abs(r["rgba8"].astype(int) - ol["rgba8"].astype(int))
    assert d.max() <= 1 and (d > 0).sum() <= 2e-4 * d.size                           # measured: 1 byte of 20 736


def test_effect_toggles_and_edge_sizes(ctx, po, sky):
    """All effects off / ragged sizes (not multiples of the 16x16 block) / 1x1 / max_steps 0."""
    g, rrt, tex = ctx
    cam = rrt.CameraState.default()
    a = cam.as_array(); ocam = po.camera(a[0], a[1], a[2], a[3])
    fx = rrt.CameraEffects(useBloom=False, useVignette=False, useLensDistortion=False)
    ofx = po.default_effects(use_bloom=0, use_vignette=0, use_lens=0)
    for arith in (0, 2):                                    # strict, and RRT_ARITH_FMAD against the oracle's FMAD mode
        for (w, h) in ((37, 23), (1, 1), (17, 16)):
            r = g.render_gpu(w, h, 0.9, 1, cam, 1.0, tex, fx=fx, arith_mode=arith)
            o = po.render(ocam, ofx, po.default_params(spin=0.9, math_mode=po.MATH_PORTABLE, arith_mode=arith), 1.0, w, h, sky)
            assert np.array_equal(r["rgba8"], o["rgba8"]), (w, h, arith)
        r = g.render_gpu(33, 9, 0.0, 1, cam, 1.0, tex, max_steps=0, arith_mode=arith)
        o = po.render(ocam, po.default_effects(), po.default_params(max_steps=0, math_mode=po.MATH_PORTABLE, arith_mode=arith),
                      1.0, 33, 9, sky)
        assert np.array_equal(r["rgba8"], o["rgba8"]), arith
        r = g.render_gpu(33, 9, 0.9, 1, cam, 1.0, tex, frac_bits=0, arith_mode=arith)
        o = po.render(ocam, po.default_effects(), po.default_params(spin=0.9, sky_frac_bits=0, math_mode=po.MATH_PORTABLE, arith_mode=arith),
                      1.0, 33, 9, sky)
        assert np.array_equal(r["rgba8"], o["rgba8"]), arith


@pytest.mark.parametrize("pos,yaw,pitch,spin", [
    ((0.0, 0.5, 0.0), 0.0, 0.0, 0.9),          # camera inside r < 1: the geodesics.h:33 guard, instant horizon
    ((0.0, 1.5, -1.0), 10.0, -30.0, 0.9),      # inside the horizon radius 2.02: every ray ends at step 0
    ((0.0, 2.5, -2.0), 0.0, -40.0, 0.99),      # just outside the horizon, looking in and out
    ((3000.0, 40.0, 0.0), -90.0, 0.0, 0.9),    # far away: rays looking outward escape after one step
    ((14.0, 0.05, 3.0), 200.0, 2.0, 0.9),      # inside the disk, in both media zones from step 0
    ((0.0, 60.0, 0.0), 0.0, -89.9, 0.0),       # straight down the spin axis, a = 0 (exact symmetries, +-0)
])
def test_unusual_cameras_match_oracle(ctx, po, sky, pos, yaw, pitch, spin):
    g, rrt, tex = ctx
    w, h = 48, 28
    cam = rrt.CameraState.from_angles(pos, yaw, pitch)
    fx = rrt.CameraEffects(useChromaticAberration=True)
    a = cam.as_array()
    for arith in (0, 2):                                    # strict, and RRT_ARITH_FMAD against the oracle's FMAD mode
        r = g.render_gpu(w, h, spin, 1, cam, 2.5, tex, fx=fx, arith_mode=arith)
        o = po.render(po.camera(a[0], a[1], a[2], a[3]), po.default_effects(use_ca=1),
                      po.default_params(spin=spin, math_mode=po.MATH_PORTABLE, arith_mode=arith), 2.5, w, h, sky,
                      want=("rgba8", "ldr", "diag"))
        assert np.array_equal(r["steps"], o["steps"]), arith
        assert np.array_equal(r["hit"], o["hit"]), arith
        assert np.array_equal(r["rgba8"], o["rgba8"]), arith
        assert same_bits(r["ldr"], o["ldr"]), arith


def test_row_and_tile_shards_reassemble_to_the_full_frame(ctx):
    """Sharded renders must be byte-identical to the single launch."""
    import torch
    g, rrt, tex = ctx
    w, h = 160, 90
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=0.9)
    full = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(full, w, h, 1.0, cam, tex, fx, prm)
    # contiguous rows written in place into the full frame
    rows = torch.zeros_like(full)
    for (y0, y1) in ((0, 31), (31, 64), (64, 90)):
        off = (h - y1) * w * 4
        rrt.launch_raymarch_rows(rows[off:], w, h, y0, y1, 1.0, cam, tex, fx, prm)
    # interleaved tiles, 3 shards of 8-row tiles (ragged last tile: 90 = 11*8 + 2)
    tiles = torch.zeros_like(full)
    for n_shards, R in ((3, 8), (8, 16), (2, 7)):
        tiles.zero_()
        for s in range(n_shards):
            nrows = rrt.tile_shard_rows(h, R, s, n_shards)
            buf = torch.zeros(max(nrows, 1) * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch_tiles(buf, w, h, R, s, n_shards, 1.0, cam, tex, fx, prm)
            rrt.assemble_tiles(tiles, buf, w, h, R, s, n_shards)
        torch.cuda.synchronize()
        assert torch.equal(tiles, full), (n_shards, R)
        # all shards gathered into one allocation, assembled by one launch (what rank 0 does after the gather)
        pad = max(rrt.tile_shard_rows(h, R, s, n_shards) for s in range(n_shards)) * w * 4
        allbuf = torch.zeros(n_shards * pad, dtype=torch.uint8, device="cuda")
        for s in range(n_shards):
            rrt.launch_raymarch_tiles(allbuf[s * pad:], w, h, R, s, n_shards, 1.0, cam, tex, fx, prm)
        tiles.zero_()
        rrt.assemble_all_tiles(tiles, allbuf, pad, w, h, R, n_shards)
        torch.cuda.synchronize()
        assert torch.equal(tiles, full), ("all", n_shards, R)
    torch.cuda.synchronize()
    assert torch.equal(rows, full)
    assert sum(rrt.tile_shard_rows(h, 8, s, 3) for s in range(3)) == h


@pytest.mark.parametrize("mode", [2, 1], ids=["fmad", "fast"])
@pytest.mark.parametrize("name", list(CASES))
def test_tolerance_modes_against_the_libm_oracle(ctx, frames_gold, name, mode):
    """RRT_ARITH_FMAD / RRT_ARITH_FAST against the INDEPENDENT oracle (glibc math, strict IEEE) on the fixtures, at the
    bars of the strict path's own tolerance test above, set to the measured class (round 5; was >= 99.5 % of pixels): float
    RGB within 1e-4 relative (+1e-5 abs) on all but a handful of a fixture's pixels, step counts likewise.  The pixel-by-pixel
    account of what falls outside -- every such pixel is one the strict arithmetic itself does not pin -- is
    tests/test_gpu_tolerance.py, at 1080p and 4K."""
    r, _ = _render(ctx, name, arith_mode=mode)
    du8 = np.abs(r["rgba8"].astype(int) - frames_gold[f"{name}_libm_rgba8"].astype(int))
    n_px = du8.shape[0] * du8.shape[1]
    steps_off = int((r["steps"] != frames_gold[f"{name}_libm_steps"].astype(np.int32)).sum())
    msg = f"{name} mode {mode}: bytes differing {(du8 > 0).sum()} (> 1 LSB: {(du8 > 1).sum()}, max {du8.max()}), step counts differing {steps_off} of {n_px}"
    if name != "G1":
        ref = frames_gold[f"{name}_libm_ldr"][..., :3]
        got = r["ldr"][..., :3]
        bad = (np.abs(got - ref) > 1e-4 * np.abs(ref) + 1e-5).any(axis=2)
        msg += f", pixels outside 1e-4: {int(bad.sum())}, max abs {np.abs(got - ref).max():.2e}"
        print(msg)
        assert bad.sum() <= 2, msg                       # of 2 304 pixels; measured: 0 on every fixture, both modes
    else:
        print(msg)
    assert (du8 > 1).sum() <= 2 and (du8 > 0).sum() <= 12, msg      # measured: 0 / <= 4 bytes (G1, 65 536 bytes)
    assert steps_off <= 3, msg                                       # measured: <= 1 ray per fixture


def test_three_pass_workspace_path_is_byte_identical(ctx):
    """rrt_params.workspace: march-only pass + pooled sample evaluation + ordered composite must give
    the bytes of the single-kernel path -- full frames, shards, both arithmetic modes, a=0 and a!=0,
    and with a pool that is far too small (overflowing wavefronts fall back to the in-line code)."""
    import torch
    g, rrt, tex = ctx
    ws = rrt.Workspace(1 << 30)
    tiny = rrt.Workspace(16 << 20)
    try:
        for (w, h, pos, yaw, pitch, t) in ((320, 180, (0.0, 10.0, -60.0), 0.0, -10.0, 1.0),
                                           (257, 131, (35.0, 0.8, 10.0), -106.0, -1.2, 12.5),
                                           (200, 120, (4.2, 0.6, 4.2), -90.0, -5.7, 14.0)):
            cam = rrt.CameraState.from_angles(pos, yaw, pitch); fx = rrt.CameraEffects(useChromaticAberration=True)
            for spin in (0.9, 0.0):
                for mode in (0, 1):
                    ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
                    rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin, arith_mode=mode))
                    for pool in (ws, tiny):
                        out = torch.zeros_like(ref)
                        # pool_rounds = 1 for the small pool: ONE round, so that what does not fit takes the in-line route
                        # (the rounds themselves: test_three_pass_rounds_reuse_a_small_pool)
                        rrt.launch_raymarch(out, w, h, t, cam, tex, fx,
                                            rrt.RenderParams(spin=spin, arith_mode=mode, workspace=pool.id, path_policy=2,
                                                             pool_rounds=1 if pool is tiny else 0))
                        torch.cuda.synchronize()
                        assert torch.equal(out, ref), (w, h, spin, mode, pool.nbytes, pool.stats())
                    assert ws.stats()["overflow_waves"] == 0 and ws.stats()["rows_used"] > 0
        assert tiny.stats()["overflow_waves"] > 0           # the small pool really did overflow on the last view
        # shards through the workspace
        w, h = 160, 90
        cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
        full = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch(full, w, h, 1.0, cam, tex, fx, rrt.RenderParams(spin=0.9))
        frame = torch.zeros_like(full)
        prm = rrt.RenderParams(spin=0.9, workspace=ws.id, path_policy=2)
        for s in range(3):
            buf = torch.zeros(rrt.tile_shard_rows(h, 8, s, 3) * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch_tiles(buf, w, h, 8, s, 3, 1.0, cam, tex, fx, prm)
            rrt.assemble_tiles(frame, buf, w, h, 8, s, 3)
        torch.cuda.synchronize()
        assert torch.equal(frame, full)
        # a bad id is reported, volumetrics-off / debug launches ignore the pool
        with pytest.raises(rrt.RRTError):
            rrt.launch_raymarch(frame, w, h, 1.0, cam, tex, fx, rrt.RenderParams(workspace=999))
    finally:
        ws.destroy(); tiny.destroy()


@pytest.mark.parametrize("name", ("G1", "G2", "G3", "G4", "G5", "K1", "K2", "R1"))
def test_frames_against_the_reference_kernel(ctx, frames_ref, name):
    """frames_ref.npz = the reference's OWN raymarch_kernel body compiled by g++ (glibc math): the HIP path takes
    exactly the reference's number of RK4 steps for every ray (the geodesics contain no transcendentals) and its
    bytes are within 1 LSB on all but a few pixels (libdevice / glibc / rrt_math.h differ by an ulp)."""
    g, rrt, tex = ctx
    w, h, spin, vol, t = frames_ref[f"{name}_scene"]
    fl, fv = frames_ref[f"{name}_fx_flags"], frames_ref[f"{name}_fx_vals"]
    fx = rrt.CameraEffects(useBloom=bool(fl[0]), useVignette=bool(fl[1]), useChromaticAberration=bool(fl[2]),
                           useLensDistortion=bool(fl[3]), bloomThreshold=float(fv[0]), bloomIntensity=float(fv[1]),
                           vignetteIntensity=float(fv[2]), caAmount=float(fv[3]), distortionAmount=float(fv[4]))
    a = frames_ref[f"{name}_camera"]
    cam = rrt.CameraState(a[0], a[1], a[2], a[3])
    r = g.render_gpu(int(w), int(h), float(np.float32(spin)), int(vol), cam, float(np.float32(t)), tex, fx=fx)
    assert np.array_equal(r["steps"], frames_ref[f"{name}_steps"].astype(np.int32))
    d = np.abs(r["rgba8"].astype(int) - frames_ref[f"{name}_rgba8"].astype(int))
    assert d.max() <= 1 and (d > 0).sum() <= 1e-4 * d.size, int((d > 0).sum())     # measured: 2 bytes on G1, 0 on the others
    prod = g.render_gpu(int(w), int(h), float(np.float32(spin)), int(vol), cam, float(np.float32(t)), tex, fx=fx, debug=False)
    assert np.array_equal(prod["rgba8"], r["rgba8"])                                # production instantiation: same bytes


def test_frame_with_a_real_sky_against_the_reference_kernel(ctx, po):
    """a frame whose sky is REAL -- a 256x128 crop of the reference's own asset as the reference's own
    decoder (stb_image, main.cpp:240) decodes it -- against the frame the reference's kernel body rendered with it
    (tests/golden/sky_ref.npz), live as well where oracle/_ref travelled, and byte for byte against the oracle."""
    import os
    from conftest import GOLDEN
    g, rrt, _ = ctx
    ref = dict(np.load(os.path.join(GOLDEN, "sky_ref.npz")))
    crop = ref["skybox2_jpg_bigcrop"]
    tex = rrt.SkyTexture(crop)
    try:
        w, h, spin, vol, t = ref["frame_scene"]
        w, h, spin, t = int(w), int(h), float(np.float32(spin)), float(np.float32(t))
        a = ref["frame_camera"]
        cam = rrt.CameraState(a[0], a[1], a[2], a[3])
        fx = rrt.CameraEffects(useChromaticAberration=True)
        r = g.render_gpu(w, h, spin, int(vol), cam, t, tex, fx=fx)
        assert np.array_equal(r["steps"], ref["frame_steps"].astype(np.int32))
        d = np.abs(r["rgba8"].astype(int) - ref["frame_rgba8"].astype(int))
        assert d.max() <= 1 and (d > 0).sum() <= 1e-4 * d.size + 1, int((d > 0).sum())
        prod = g.render_gpu(w, h, spin, int(vol), cam, t, tex, fx=fx, debug=False)
        assert np.array_equal(prod["rgba8"], r["rgba8"])
        ocam = po.camera(a[0], a[1], a[2], a[3])
        exact = po.render(ocam, po.default_effects(use_ca=1), po.default_params(spin=spin, volumetrics=int(vol), math_mode=po.MATH_PORTABLE),
                          t, w, h, crop)["rgba8"]
        assert np.array_equal(r["rgba8"], exact)
        if po.ref_frames_available():
            live = po.ref_render(a, po.default_effects(use_ca=1), spin, int(vol), t, w, h, crop)
            assert np.array_equal(live["rgba8"], ref["frame_rgba8"])
        # a raw sky file shipped from the build container is what the package loads (same texels in, same frame out)
        import tempfile
        from relativisticraytracer_amd import sky as skymod
        with tempfile.TemporaryDirectory() as td:
            skymod.save_sky_raw(os.path.join(td, "s.rrtsky"), crop)
            tex2 = rrt.SkyTexture(skymod.load_sky(os.path.join(td, "s.rrtsky")))
            r2 = g.render_gpu(w, h, spin, int(vol), cam, t, tex2, fx=fx, debug=False)
            tex2.destroy()
        assert np.array_equal(r2["rgba8"], r["rgba8"])
    finally:
        tex.destroy()


def test_random_scenes_against_the_reference_kernel_live(ctx, po, sky):
    """HIP path vs the REFERENCE's kernel body rendered live on this host (oracle/_ref/libref_frames.so was compiled
    from /root/reference in the build container and travels with the tree; skipped where it is absent): on seeded
    random scenes no fixture holds, every ray takes the reference's number of RK4 steps, and the bytes differ by one
    LSB on a few pixels at most (glibc vs rrt_math.h, an ulp apart; larger jumps are hard-gate flips, counted)."""
    import os
    if not po.ref_frames_available():
        pytest.skip("oracle/_ref/libref_frames.so not in this tree")
    from scene_gen import random_scene
    g, rrt, tex = ctx
    rng = np.random.default_rng(int(os.environ.get("RRT_SWEEP_SEED", "1618")))
    n_bytes = n_diff = n_big = media = 0
    for case in range(int(os.environ.get("RRT_REF_SWEEP_CASES", "24"))):
        sc = random_scene(rng, case)
        ofx = po.default_effects(**sc["fx"])
        ref = po.ref_render(sc["cam"], ofx, sc["spin"], sc["vol"], sc["t"], sc["w"], sc["h"], sky)
        f = sc["fx"]
        fx = rrt.CameraEffects(useBloom=bool(f["use_bloom"]), useVignette=bool(f["use_vignette"]),
                               useChromaticAberration=bool(f["use_ca"]), useLensDistortion=bool(f["use_lens"]),
                               bloomThreshold=f["bloom_threshold"], bloomIntensity=f["bloom_intensity"],
                               vignetteIntensity=f["vignette_intensity"], caAmount=f["ca_amount"],
                               distortionAmount=f["distortion_amount"])
        a = sc["cam"]
        r = g.render_gpu(sc["w"], sc["h"], sc["spin"], sc["vol"], rrt.CameraState(a[0], a[1], a[2], a[3]), sc["t"], tex, fx=fx)
        assert np.array_equal(r["steps"], ref["steps"]), case
        d = np.abs(r["rgba8"].astype(int) - ref["rgba8"].astype(int))
        n_bytes += d.size; n_diff += int((d > 0).sum()); n_big += int((d > 1).sum())
        media += int(sc["vol"] and (r["rad"][:, 3] < 1.0).any())
    # measured on the default seed: 0 of 57 176 bytes differ; soaks with other seeds (RRT_SWEEP_SEED) stay inside this
    assert n_diff <= 1e-4 * n_bytes + 2 and n_big <= 2e-5 * n_bytes + 1, (n_diff, n_big, n_bytes)
    assert media >= 5


@pytest.mark.parametrize("w,h,stride", [(3840, 2160, 29), (1920, 1080, 17)])
def test_baseline_frames_against_the_reference_kernel_live(ctx, po, sky, w, h, stride):
    """BASELINE's metric frame (4K, a = 0.9, full volumetrics, default camera) and the 1080p one, through the noise
    tables, against the REFERENCE's kernel body run live on this host at every `stride`-th pixel (the whole 4K frame
    was compared once: profiles/r02_dense_parity_vs_reference.txt): identical step counts, bytes within one LSB."""
    import torch
    if not po.ref_frames_available():
        pytest.skip("oracle/_ref/libref_frames.so not in this tree")
    g, rrt, tex = ctx
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
    nt = rrt.NoiseTable(4.0)
    try:
        out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        steps = torch.zeros(h * w, dtype=torch.int32, device="cuda")
        rrt.launch_raymarch_debug(out, w, h, 1.0, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id), steps=steps)
        torch.cuda.synchronize()
    finally:
        nt.destroy()
    ref = po.ref_render(cam.as_array(), po.default_effects(), 0.9, 1, 1.0, w, h, sky, stride=(stride, stride))
    ys = np.arange(0, h, stride); xs = np.arange(0, w, stride); rows = h - 1 - ys
    assert np.array_equal(steps.cpu().numpy().reshape(h, w)[np.ix_(ys, xs)], ref["steps"].reshape(h, w)[np.ix_(ys, xs)])
    d = np.abs(out.cpu().numpy().reshape(h, w, 4)[np.ix_(rows, xs)].astype(int) - ref["rgba8"][np.ix_(rows, xs)].astype(int))
    # the whole 4K frame differs from the reference's in 165 of 33 177 600 bytes (5e-6: profiles/r02_dense_parity_vs_reference.txt);
    # on these strided samples (39 900 / 28 928 bytes) the oracle finds none
    assert d.max() <= 1 and (d > 0).sum() <= max(1, 2e-5 * d.size), int((d > 0).sum())


def test_noise_table_path_is_byte_identical(ctx):
    """rrt_params.noise_table: low-octave noise3D calls read their corner hashes from the lattice tables
    whenever a wavefront's rays share a few cells.  Same bytes as the arithmetic path -- on 4K views where the
    switches are on nearly everywhere (bench view, disk-grazing, from inside the disk), on small frames where
    they are mostly off, through the three-pass path and shards; no read ever leaves a table box."""
    import torch
    g, rrt, tex = ctx
    nt = rrt.NoiseTable(20.0)
    ws = rrt.Workspace(3 << 30)
    try:
        views = [(3840, 2160, (0.0, 10.0, -60.0), 0.0, -10.0, 1.0),
                 (3840, 2160, (4.2, 0.6, 4.2), -90.0, -5.7, 14.0),
                 (1920, 1080, (35.0, 0.8, 10.0), -106.0, -1.2, 12.5),
                 (1000, 700, (15.0, 3.0, -30.0), -26.6, -5.1, 6.0),
                 (96, 54, (14.0, 0.05, 3.0), 200.0, 2.0, 19.5)]
        for (w, h, pos, yaw, pitch, t) in views:
            cam = rrt.CameraState.from_angles(pos, yaw, pitch); fx = rrt.CameraEffects(useChromaticAberration=True)
            for spin, mode in ((0.9, 0), (0.0, 0), (0.9, 1)):
                ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
                rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin, arith_mode=mode))
                out = torch.zeros_like(ref)
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx,
                                    rrt.RenderParams(spin=spin, arith_mode=mode, noise_table=nt.id))
                torch.cuda.synchronize()
                assert torch.equal(out, ref), (w, h, pos, spin, mode)
                if w * h <= 1920 * 1080:
                    out.zero_()
                    rrt.launch_raymarch(out, w, h, t, cam, tex, fx,
                                        rrt.RenderParams(spin=spin, arith_mode=mode, noise_table=nt.id, workspace=ws.id,
                                                         path_policy=2))
                    torch.cuda.synchronize()
                    assert torch.equal(out, ref), ("three-pass", w, h, pos, spin, mode, ws.stats())
            # debug launch: counts table reads that had to be clamped
            oob = torch.zeros(1, dtype=torch.int32, device="cuda")
            out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch_debug(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id), lut_oob=oob)
            torch.cuda.synchronize()
            assert int(oob.item()) == 0, (w, h, pos)
        # a time outside the table's range silently takes the arithmetic kernels
        w, h = 160, 90
        cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
        ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda"); out = torch.zeros_like(ref)
        for t in (25.0, -1.0):
            rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
            torch.cuda.synchronize()
            assert torch.equal(out, ref), t
    finally:
        nt.destroy(); ws.destroy()


def test_three_pass_full_size_and_heavy_view(ctx):
    """The pool at scale: the whole 4K bench frame (2.6 M rows, runs of up to 32 blocks) and a disk-skimming
    1080p view where single wavefronts own ~2000 rows; then the same heavy view through a pool that is too
    small, so that a large part of the wavefronts take the overflow route."""
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects()
    big = rrt.Workspace(6 << 30)
    small = rrt.Workspace(192 << 20)
    try:
        for (w, h, cam, t, pool) in ((3840, 2160, rrt.CameraState.default(), 1.0, big),
                                     (1920, 1080, rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7), 14.0, big),
                                     (1920, 1080, rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7), 14.0, small)):
            ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
            out = torch.zeros_like(ref)
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, workspace=pool.id, path_policy=2,
                                                                             pool_rounds=1 if pool is small else 8))        # small: ONE round -> the in-line route; big: rounds to spare
            torch.cuda.synchronize()
            st = pool.stats()
            assert torch.equal(out, ref), (w, h, st)
            if pool is small:
                assert st["overflow_waves"] > 100
            else:
                assert st["overflow_waves"] == 0 and st["rows_used"] > 100000
        # auto policy: a full 4K frame stays on the single kernel (pool untouched), an eighth of it does not
        w, h = 3840, 2160
        prm = rrt.RenderParams(spin=0.9, workspace=big.id)
        buf = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch_tiles(buf, w, h, 16, 3, 8, 1.0, rrt.CameraState.default(), tex, fx, prm)
        torch.cuda.synchronize()
        assert 0 < big.stats()["rows_used"] < 600000
    finally:
        big.destroy(); small.destroy()


def test_three_pass_rounds_reuse_a_small_pool(ctx):
    """Round 4 (rrt_params.pool_rounds): a pool far too small for the view is used in ROUNDS -- march until it is full,
    evaluate + composite, resume the suspended wavefronts -- so that no ray takes the in-line route: bytes of the single
    kernel, overflow_waves == 0, several rounds with work.  With too few rounds the rest finishes in line (same bytes);
    the automatic round count learns from the previous launch through the same workspace."""
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects(useChromaticAberration=True)
    pool = rrt.Workspace(25 << 20)      # (30 MB through round 4, when a row had six planes)
    nt = rrt.NoiseTable(16.0)
    order = rrt.TileOrder()
    try:
        for (w, h, pos, yaw, pitch, t, spin) in ((320, 180, (4.2, 0.6, 4.2), -90.0, -5.7, 14.0, 0.9),
                                                 (257, 131, (35.0, 0.8, 10.0), -106.0, -1.2, 12.5, 0.0)):
            cam = rrt.CameraState.from_angles(pos, yaw, pitch)
            ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin))
            for mode in (0, 1):
                if mode:
                    rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin, arith_mode=1))
                seen = []
                for rounds, table, oid, chains in ((48, 0, 0, 1), (48, nt.id, 0, 1), (2, 0, 0, 1), (1, nt.id, 0, 1), (48, nt.id, order.id, 1),
                                                   (48, 0, order.id, 1), (48, nt.id, 0, 2), (48, 0, order.id, 2), (1, nt.id, order.id, 2)):
                    out = torch.zeros_like(ref)
                    rrt.launch_raymarch(out, w, h, t, cam, tex, fx,
                                        rrt.RenderParams(spin=spin, arith_mode=mode, workspace=pool.id, path_policy=2,
                                                         pool_rounds=rounds, noise_table=table, tile_order=oid, pass_chains=chains))
                    torch.cuda.synchronize()
                    st = pool.stats()
                    assert torch.equal(out, ref), (w, h, mode, rounds, st)
                    assert st["rounds_enqueued"] == rounds
                    seen.append(st)
                assert seen[0]["overflow_waves"] == 0 and seen[0]["rounds_with_work"] >= 2, seen[0]
                assert seen[0]["peak_rows"] <= seen[0]["pool_rows"] and seen[0]["rows_used"] > seen[0]["pool_rows"]
                assert seen[2]["overflow_waves"] > 0 and seen[3]["overflow_waves"] > 0        # too few rounds: in line
                assert seen[4]["overflow_waves"] == 0 and seen[5]["overflow_waves"] == 0
                # two chains (each half of the dispatch order in its own slice of the pool, on its own stream): same bytes,
                # nothing in line with enough rounds, the in-line route with one
                assert seen[6]["overflow_waves"] == 0 and seen[7]["overflow_waves"] == 0 and seen[8]["overflow_waves"] > 0
        # automatic: the first launch through a fresh workspace guesses 2 rounds, later ones take what the previous one needed
        fresh = rrt.Workspace(25 << 20)
        w, h, t = 320, 180, 14.0
        cam = rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7)
        ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
        hist = []
        for _ in range(5):
            out = torch.zeros_like(ref)
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, workspace=fresh.id, path_policy=2))
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
            hist.append(fresh.stats())
        assert hist[0]["rounds_enqueued"] == 2 and hist[0]["overflow_waves"] > 0
        assert hist[-1]["overflow_waves"] == 0 and hist[-1]["rounds_enqueued"] >= hist[-1]["rounds_with_work"], hist
        fresh.destroy()
    finally:
        pool.destroy(); nt.destroy(); order.destroy()


def test_three_pass_two_chains_by_default_on_larger_launches(ctx):
    """rrt_params.pass_chains = 0: a launch of >= 2048 wavefronts runs its two halves as two chains side by side -- bytes of
    the single kernel for full frames and shards, repeatedly through one workspace (the pool split and the round counts adapt
    to what the previous launch needed), also with a pool small enough to need rounds in the heavy half."""
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects()
    nt = rrt.NoiseTable(16.0)
    try:
        for (w, h, pos, yaw, pitch, t, pool_mib) in ((960, 540, (0.0, 10.0, -60.0), 0.0, -10.0, 1.0, 512),
                                                     (640, 360, (4.2, 0.6, 4.2), -90.0, -5.7, 14.0, 96)):
            cam = rrt.CameraState.from_angles(pos, yaw, pitch)
            ws = rrt.Workspace(pool_mib << 20)
            ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
            prm = rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2)
            hist = []
            for k in range(8):          # the round count doubles (+1) while rays are still suspended at the end: it converges
                out = torch.zeros_like(ref)
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx, prm)
                torch.cuda.synchronize()
                assert torch.equal(out, ref), (w, h, k, ws.stats())
                hist.append(ws.stats())
            assert hist[-1]["overflow_waves"] == 0 and hist[-2]["overflow_waves"] == 0, hist
            one = rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2, pass_chains=1)
            out = torch.zeros_like(ref)
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, one)
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
            # shards (interleaved tiles) through two chains, two launches back to back on one stream through one workspace
            frame = torch.zeros_like(ref)
            for sh in range(2):
                buf = torch.zeros(rrt.tile_shard_rows(h, 16, sh, 2) * w * 4, dtype=torch.uint8, device="cuda")
                rrt.launch_raymarch_tiles(buf, w, h, 16, sh, 2, t, cam, tex, fx, prm)
                rrt.assemble_tiles(frame, buf, w, h, 16, sh, 2)
            torch.cuda.synchronize()
            assert torch.equal(frame, ref)
            ws.destroy()
    finally:
        nt.destroy()


def test_tile_maps_probe_and_balance(ctx):
    """Cost-weighted tile -> shard assignment (rrt_tile_map): the coarse probe's row-tile costs, dealt longest-first, give
    shards whose estimated loads agree to a few per cent where t mod n is far off; rendering every shard of such a map --
    single kernel and three-pass -- and ONE rrt_assemble_all_tilemap reproduces the single launch byte for byte; a random
    map does too."""
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects()
    ws = rrt.Workspace(512 << 20)
    try:
        for (w, h, R, G, cam, t) in ((640, 360, 8, 8, rrt.CameraState.default(), 1.0),
                                     (500, 281, 16, 3, rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7), 14.0)):
            prm = rrt.RenderParams(spin=0.9)
            full = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch(full, w, h, t, cam, tex, fx, prm)
            cost = rrt.probe_tile_costs(w, h, R, t, cam, fx, prm)
            n_tiles = (h + R - 1) // R
            assert cost.shape == (n_tiles,) and (cost > 0).all()
            assert np.array_equal(cost, rrt.probe_tile_costs(w, h, R, t, cam, fx, prm))        # deterministic
            dealt = rrt.balance_tiles(cost, G)
            load = np.bincount(dealt, weights=cost, minlength=G)
            modulo = np.bincount(np.arange(n_tiles) % G, weights=cost, minlength=G)
            assert load.max() / load.mean() <= modulo.max() / modulo.mean() + 1e-6
            rng = np.random.default_rng(9)
            for assignment in (dealt, rng.integers(0, G, n_tiles).astype(np.int32), np.arange(n_tiles, dtype=np.int32) % G):
                tm = rrt.TileMap(h, R, G, assignment)
                stride = tm.max_shard_rows() * w * 4
                for policy, wsid in ((1, 0), (2, ws.id)):
                    allbuf = torch.zeros(G * stride, dtype=torch.uint8, device="cuda")
                    p2 = rrt.RenderParams(spin=0.9, workspace=wsid, path_policy=policy)
                    for sh in range(G):
                        assert tm.shard_rows(sh) == sum(min(R, h - tt * R) for tt in range(n_tiles) if assignment[tt] == sh)
                        rrt.launch_raymarch_tilemap(allbuf[sh * stride:], w, h, tm, sh, t, cam, tex, fx, p2)
                    frame = torch.zeros_like(full)
                    rrt.assemble_all_tilemap(frame, allbuf, stride, w, h, tm)
                    torch.cuda.synchronize()
                    assert torch.equal(frame, full), (w, h, policy)
                tm.destroy()
        with pytest.raises(rrt.RRTError):
            rrt.TileMap(360, 8, 4, np.full(45, 4, np.int32))          # shard index out of range
    finally:
        ws.destroy()


def test_first_frame_order_comes_from_the_probe(ctx):
    """rrt_tile_order without history: the first launch of a geometry is ordered by the coarse probe of the view (seeded
    launches are counted), later ones by measured costs; rrt_tile_order_set_seeding(0) renders the first frame in the
    static order.  Same bytes every way, shards included."""
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects()
    w, h, t = 640, 360, 14.0
    cam = rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7)
    ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
    order = rrt.TileOrder()
    plain = rrt.TileOrder()
    plain.set_seeding(False)
    try:
        for o, want_seeded in ((order, 1), (plain, 0)):
            for k in range(3):
                out = torch.zeros_like(ref)
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, tile_order=o.id))
                torch.cuda.synchronize()
                assert torch.equal(out, ref), k
            info = o.info(arrays=True)
            assert o.seeded_launches() == want_seeded and info["launches"] == 3 and info["ordered_launches"] == 2
            assert sorted(info["perm"].tolist()) == list(range(info["n_tiles"]))
        # a shard through the probe-seeded order (the probe runs over the shard's own rows)
        buf = torch.zeros(rrt.tile_shard_rows(h, 16, 1, 3) * w * 4, dtype=torch.uint8, device="cuda")
        want = torch.zeros_like(buf)
        rrt.launch_raymarch_tiles(want, w, h, 16, 1, 3, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
        rrt.launch_raymarch_tiles(buf, w, h, 16, 1, 3, t, cam, tex, fx, rrt.RenderParams(spin=0.9, tile_order=order.id))
        torch.cuda.synchronize()
        assert torch.equal(buf, want) and order.seeded_launches() == 2
    finally:
        order.destroy(); plain.destroy()


def test_two_host_threads_with_their_own_objects_render_concurrently(ctx):
    """launches through DIFFERENT tile-order objects (and workspaces) from different host threads no longer
    serialise on a registry lock -- and must not corrupt each other: two threads, each with its own stream, order object
    and pool, render different views through both paths at the same time (ctypes releases the GIL inside the library)."""
    import threading
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects()
    w, h = 320, 180
    views = [(rrt.CameraState.default(), 1.0), (rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7), 14.0)]
    refs = []
    for cam, t in views:
        r = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch(r, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
        refs.append(r)
    torch.cuda.synchronize()
    errors = []

    def worker(idx):
        try:
            cam, t = views[idx]
            st = torch.cuda.Stream()
            order, ws = rrt.TileOrder(), rrt.Workspace(48 << 20)
            out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            for k in range(12):
                prm = rrt.RenderParams(spin=0.9, tile_order=order.id, workspace=ws.id if k % 2 else 0, path_policy=2 if k % 2 else 1,
                                       pass_chains=2, pool_rounds=8)
                with torch.cuda.stream(st):
                    out.zero_()
                    rrt.launch_raymarch(out, w, h, t, cam, tex, fx, prm, stream=st)
                st.synchronize()
                if not torch.equal(out, refs[idx]):
                    errors.append((idx, k))
            order.destroy(); ws.destroy()
        except Exception as e:          # noqa: BLE001 -- reported through the list
            errors.append((idx, repr(e)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120)
        assert not th.is_alive()
    assert not errors, errors


def test_clock_probe_reports_a_plausible_shader_clock(ctx):
    g, rrt, tex = ctx
    ghz = rrt.clock_probe_ghz(5000)
    assert 0.5 < ghz < 2.6, ghz


def test_streams_graph_capture_and_borrowed_sky(ctx, sky):
    """The launch allocates nothing and keeps no state: it runs on a side stream, can be captured into a
    HIP graph and replayed, and accepts a sky that lives in caller-owned device memory."""
    import ctypes as C
    import torch
    g, rrt, tex = ctx
    from relativisticraytracer_amd import _lib
    w, h = 128, 72
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=0.9)
    ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(ref, w, h, 1.0, cam, tex, fx, prm)
    torch.cuda.synchronize()
    # side stream
    side = torch.cuda.Stream()
    a = torch.zeros_like(ref)
    rrt.launch_raymarch(a, w, h, 1.0, cam, tex, fx, prm, stream=side)
    side.synchronize()
    assert torch.equal(a, ref)
    # graph capture + two replays
    b = torch.zeros_like(ref)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_raymarch(b, w, h, 1.0, cam, tex, fx, prm)
    for _ in range(2):
        b.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(b, ref)
    # a tile-order object under capture: the captured launch renders in the static order and leaves the
    # object alone, so that live launches through it can rewrite its permutation while the graph is replayed
    order = rrt.TileOrder()
    oprm = rrt.RenderParams(spin=0.9, tile_order=order.id)
    live = torch.zeros_like(ref)
    rrt.launch_raymarch(live, w, h, 1.0, cam, tex, fx, oprm)          # sizes the object's buffers outside the capture
    torch.cuda.synchronize()
    before = order.info()
    c2 = torch.zeros_like(ref)
    graph2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph2):
        rrt.launch_raymarch(c2, w, h, 1.0, cam, tex, fx, oprm)
    assert order.info() == before                                      # nothing recorded, nothing sorted
    for _ in range(3):
        c2.zero_()
        graph2.replay()
        rrt.launch_raymarch(live, w, h, 1.0, cam, tex, fx, oprm, stream=side)      # a live launch re-sorts meanwhile
        torch.cuda.synchronize()
        assert torch.equal(c2, ref) and torch.equal(live, ref)
    assert order.info()["launches"] == before["launches"] + 3
    order.destroy()
    # the three-pass path under capture: one chain (the workspace's side stream stays out of a capture), rounds as enqueued
    wsg = rrt.Workspace(64 << 20)
    d3 = torch.zeros_like(ref)
    p3 = rrt.RenderParams(spin=0.9, workspace=wsg.id, path_policy=2, pool_rounds=3)
    rrt.launch_raymarch(d3, w, h, 1.0, cam, tex, fx, p3)
    torch.cuda.synchronize()
    assert torch.equal(d3, ref)
    graph3 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph3):
        rrt.launch_raymarch(d3, w, h, 1.0, cam, tex, fx, p3)
    for _ in range(2):
        d3.zero_()
        graph3.replay()
        torch.cuda.synchronize()
        assert torch.equal(d3, ref)
    assert wsg.stats()["rounds_enqueued"] == 3 and wsg.stats()["overflow_waves"] == 0
    del graph3
    wsg.destroy()
    # borrowed device sky
    dsky = torch.from_numpy(sky).cuda()
    hnd = C.c_ulonglong(0)
    _lib.check(_lib.load().rrt_sky_create_from_device(C.c_void_p(dsky.data_ptr()), sky.shape[1], sky.shape[0],
                                                      C.byref(hnd)), "sky_from_device")
    c = torch.zeros_like(ref)
    rrt.launch_raymarch(c, w, h, 1.0, cam, hnd.value, fx, prm)
    torch.cuda.synchronize()
    assert torch.equal(c, ref)
    assert _lib.load().rrt_sky_destroy(hnd.value) == 0
    assert _lib.load().rrt_sky_destroy(hnd.value) in (4,)        # double destroy is reported, not fatal


def test_launch_argument_errors(ctx):
    import ctypes as C
    import torch
    g, rrt, tex = ctx
    from relativisticraytracer_amd import _lib
    lib = _lib.load()
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    p = C.c_void_p(out.data_ptr())
    assert lib.rrt_launch_raymarch(None, 4, 4, 0.0, C.byref(cam), tex.handle, C.byref(fx), None, None) == 1
    assert lib.rrt_launch_raymarch(p, 0, 4, 0.0, C.byref(cam), tex.handle, C.byref(fx), None, None) == 1
    assert lib.rrt_launch_raymarch(p, 4, 4, 0.0, C.byref(cam), 0, C.byref(fx), None, None) == 4      # bad handle
    bad = rrt.RenderParams(); bad.noise_table = -1
    bad3 = rrt.RenderParams(); bad3.noise_table = 77
    assert lib.rrt_launch_raymarch(p, 4, 4, 0.0, C.byref(cam), tex.handle, C.byref(fx), C.byref(bad3), None) == 4   # no such table
    bad2 = rrt.RenderParams(); bad2.arith_mode = 5
    assert lib.rrt_launch_raymarch(p, 4, 4, 0.0, C.byref(cam), tex.handle, C.byref(fx), C.byref(bad2), None) == 1
    assert lib.rrt_launch_raymarch(p, 4, 4, 0.0, C.byref(cam), tex.handle, C.byref(fx), C.byref(bad), None) == 1
    assert lib.rrt_launch_raymarch_rows(p, 4, 4, 3, 2, 0.0, C.byref(cam), tex.handle, C.byref(fx), None, None) == 1
    with pytest.raises(rrt.RRTError):
        rrt.launch_raymarch(out, -1, 4, 0.0, cam, tex, fx)


def test_non_finite_inputs_terminate_and_stay_in_bounds(ctx):
    """Garbage in must not hang or fault: NaN / Inf / huge camera vectors and times.  Every loop of the path is
    bounded by max_steps and every table / sky index is clamped or wrapped, so each launch completes, writes alpha
    255 to every pixel, and a clean frame afterwards is unchanged -- single kernel, noise tables, three-pass pool."""
    import torch
    g, rrt, tex = ctx
    w, h = 64, 40
    fx = rrt.CameraEffects(useChromaticAberration=True)
    good = rrt.CameraState.default()
    want = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(want, w, h, 1.0, good, tex, fx, rrt.RenderParams(spin=0.9))
    nan, inf = float("nan"), float("inf")
    cams = [rrt.CameraState(pos=(nan, 10, -60)), rrt.CameraState(pos=(0, 10, -60), forward=(nan, nan, nan)),
            rrt.CameraState(pos=(inf, 0, 0)), rrt.CameraState(pos=(1e30, -1e30, 1e30), forward=(0, 0, 1e30)),
            rrt.CameraState(pos=(12, 0.1, 0), forward=(0, 0, 0), right=(0, 0, 0), up=(0, 0, 0)),
            rrt.CameraState(pos=(12, 0.1, 0), forward=(inf, 0, 0), right=(0, -inf, 0), up=(0, 0, nan))]
    ws = rrt.Workspace(64 << 20)
    nt = rrt.NoiseTable(4.0)
    try:
        out = torch.zeros_like(want)
        for cam in cams + [good]:
            for t in (1.0, nan, inf, -inf, 3.0e38):
                for prm in (rrt.RenderParams(spin=0.9), rrt.RenderParams(spin=0.9, noise_table=nt.id),
                            rrt.RenderParams(spin=0.9, workspace=ws.id, path_policy=2, noise_table=nt.id)):
                    out.zero_()
                    rrt.launch_raymarch(out, w, h, t, cam, tex, fx, prm)
                    torch.cuda.synchronize()
                    assert bool((out.view(-1, 4)[:, 3] == 255).all())
        rrt.launch_raymarch(out, w, h, 1.0, good, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
        torch.cuda.synchronize()
        assert torch.equal(out, want)
    finally:
        nt.destroy(); ws.destroy()


def test_extreme_aspect_ratios_and_the_height_limit(ctx, po, sky):
    """Frames far outside the usual shapes: 8 x 70 001 (more rows than a HIP grid has y-blocks: the assemble kernels
    stride over rows) and 70 001 x 3.  Shards reassemble to the full frame and sampled pixels equal the oracle's;
    a frame taller than one launch can cover (65 535 row-blocks of 8 rows) is refused loudly."""
    import torch
    g, rrt, tex = ctx
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=0.9)
    a = cam.as_array(); ocam = po.camera(a[0], a[1], a[2], a[3])
    oprm = po.default_params(spin=0.9, math_mode=po.MATH_PORTABLE)
    for (w, h, sx, sy) in ((8, 70001, 3, 4999), (70001, 3, 4999, 1)):
        full = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch(full, w, h, 1.0, cam, tex, fx, prm)
        n_shards, R = 2, 16
        pad = max(rrt.tile_shard_rows(h, R, s, n_shards) for s in range(n_shards)) * w * 4
        allbuf = torch.zeros(n_shards * pad, dtype=torch.uint8, device="cuda")
        one = torch.zeros_like(full)
        for s in range(n_shards):
            rrt.launch_raymarch_tiles(allbuf[s * pad:], w, h, R, s, n_shards, 1.0, cam, tex, fx, prm)
            rrt.assemble_tiles(one, allbuf[s * pad:], w, h, R, s, n_shards)
        together = torch.zeros_like(full)
        rrt.assemble_all_tiles(together, allbuf, pad, w, h, R, n_shards)
        torch.cuda.synchronize()
        assert torch.equal(one, full) and torch.equal(together, full), (w, h)
        got = full.cpu().numpy().reshape(h, w, 4)
        o = po.render(ocam, po.default_effects(), oprm, 1.0, w, h, sky, stride=(sx, sy))["rgba8"]
        ys = np.arange(0, h, sy); xs = np.arange(0, w, sx)
        rows = h - 1 - ys
        assert np.array_equal(got[np.ix_(rows, xs)], o[np.ix_(rows, xs)]), (w, h)
        assert (got[..., 3] == 255).all()
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    with pytest.raises(rrt.RRTError):
        rrt.launch_raymarch(small, 1, 65535 * 8 + 1, 1.0, cam, tex, fx, prm)      # validated before anything is launched


@pytest.mark.parametrize("w,h,spin,t,stride", [
    (1920, 1080, 0.9, 1.0, 53),       # BASELINE configs[1]/[2] size
    (3840, 2160, 0.9, 1.0, 97),       # the bench frame (BASELINE metric config)
    (3840, 2160, 0.99, 1.0, 101),     # configs[3]
    (7680, 4320, 0.9, 3.0, 211),      # configs[4] size
])
def test_full_size_frames_sampled_against_oracle(ctx, po, sky, w, h, spin, t, stride):
    """Full-size frames: the oracle renders every `stride`-th pixel in x and y of the SAME frame
    (hundreds to thousands of rays) and those pixels must carry identical bytes in the GPU frame."""
    import torch
    g, rrt, tex = ctx
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=spin)
    out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(out, w, h, t, cam, tex, fx, prm)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(h, w, 4)
    a = cam.as_array()
    o = po.render(po.camera(a[0], a[1], a[2], a[3]), po.default_effects(),
                  po.default_params(spin=spin, math_mode=po.MATH_PORTABLE), t, w, h, sky, stride=(stride, stride))["rgba8"]
    ys = np.arange(0, h, stride); xs = np.arange(0, w, stride)
    rows = (h - 1 - ys)                                   # bottom-up storage
    assert np.array_equal(got[np.ix_(rows, xs)], o[np.ix_(rows, xs)])
    assert got[np.ix_(rows, xs)][..., :3].any()


@pytest.mark.parametrize("name,w,h,vol,frame_k,stride", [
    ("configs[1]: 1080p, skybox only", 1920, 1080, 0, 0, 41),
    ("configs[4]: 8K, path 0 frame 150, all effects", 7680, 4320, 1, 150, 193),
    ("configs[4]: 8K, path 0 frame 288 (inside the disk plane), all effects", 7680, 4320, 1, 288, 257),
])
def test_baseline_configs_at_full_size_sampled_against_oracle(ctx, po, sky, name, w, h, vol, frame_k, stride):
    """The BASELINE.json configurations round 1 only ran small or with the default camera: configs[1] (volumetrics off)
    at its real 1920x1080, and configs[4] (7680x4320, "Gargantua Fly-By" camera path with the recording clock, chromatic
    aberration on) -- with the noise tables, as the drivers render it.  Every `stride`-th pixel against the oracle."""
    import torch
    from relativisticraytracer_amd import camera_paths as cp
    g, rrt, tex = ctx
    if frame_k:
        t, pt = cp.recording_clock(frame_k)
        cam = cp.CameraPath(0).camera_at(pt)
        fx = rrt.CameraEffects(useChromaticAberration=True); ofx = po.default_effects(use_ca=1)
    else:
        t, cam, fx, ofx = 1.0, rrt.CameraState.default(), rrt.CameraEffects(), po.default_effects()
    nt = rrt.NoiseTable(14.0) if vol else None
    try:
        out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, volumetrics=vol, noise_table=nt.id if nt else 0))
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(h, w, 4)
    finally:
        if nt:
            nt.destroy()
    a = cam.as_array()
    o = po.render(po.camera(a[0], a[1], a[2], a[3]), ofx, po.default_params(spin=0.9, volumetrics=vol, math_mode=po.MATH_PORTABLE),
                  t, w, h, sky, stride=(stride, stride))["rgba8"]
    ys = np.arange(0, h, stride); xs = np.arange(0, w, stride)
    rows = (h - 1 - ys)
    assert np.array_equal(got[np.ix_(rows, xs)], o[np.ix_(rows, xs)]), name
    assert got[np.ix_(rows, xs)][..., :3].any()


def test_config3_all_eight_shards_at_4k_assemble_to_the_single_launch(ctx, po, sky):
    """BASELINE configs[3] as an 8-GPU workload, rehearsed on one GPU at FULL size: the 3840x2160 a = 0.99 frame
    rendered as its eight interleaved 16-row-tile shards -- through the path a rank's launch actually takes (three-pass
    pool for a share of 1.04 M rays, noise tables) -- into one gathered allocation, scattered by the single
    rrt_assemble_all_tiles launch rank 0 runs after the gather: equal to the single launch of the same frame, byte
    for byte, and to the oracle on every 101st pixel."""
    import torch
    g, rrt, tex = ctx
    w, h, R, n = 3840, 2160, 16, 8
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
    nt = rrt.NoiseTable(4.0); ws = rrt.Workspace(2 << 30)
    try:
        full = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        rrt.launch_raymarch(full, w, h, 1.0, cam, tex, fx, rrt.RenderParams(spin=0.99, noise_table=nt.id))
        pad = max(rrt.tile_shard_rows(h, R, s, n) for s in range(n)) * w * 4
        assert sum(rrt.tile_shard_rows(h, R, s, n) for s in range(n)) == h
        gathered = torch.zeros(n * pad, dtype=torch.uint8, device="cuda")
        prm = rrt.RenderParams(spin=0.99, noise_table=nt.id, workspace=ws.id)          # RRT_PATH_AUTO: three-pass for <= 1.5 M rays
        overflow = 0
        for sh in range(n):
            rrt.launch_raymarch_tiles(gathered[sh * pad:], w, h, R, sh, n, 1.0, cam, tex, fx, prm)
            torch.cuda.synchronize()
            st = ws.stats()
            assert st["rows_used"] > 0, "the shard did not take the three-pass path"
            overflow += st["overflow_waves"]
        frame = torch.zeros_like(full)
        rrt.assemble_all_tiles(frame, gathered, pad, w, h, R, n)
        torch.cuda.synchronize()
        assert torch.equal(frame, full), f"{int((frame != full).sum())} bytes differ"
        # and without the pool (single kernel per shard), per-shard assembly
        frame.zero_()
        for sh in range(n):
            buf = gathered[sh * pad:(sh + 1) * pad]; buf.zero_()
            rrt.launch_raymarch_tiles(buf, w, h, R, sh, n, 1.0, cam, tex, fx, rrt.RenderParams(spin=0.99))
            rrt.assemble_tiles(frame, buf, w, h, R, sh, n)
        torch.cuda.synchronize()
        assert torch.equal(frame, full)
    finally:
        nt.destroy(); ws.destroy()
    stride = 101
    a = cam.as_array()
    o = po.render(po.camera(a[0], a[1], a[2], a[3]), po.default_effects(), po.default_params(spin=0.99, math_mode=po.MATH_PORTABLE),
                  1.0, w, h, sky, stride=(stride, stride))["rgba8"]
    ys = np.arange(0, h, stride); xs = np.arange(0, w, stride); rows = h - 1 - ys
    assert np.array_equal(frame.cpu().numpy().reshape(h, w, 4)[np.ix_(rows, xs)], o[np.ix_(rows, xs)])


def test_noise_table_windows_far_along_the_clock(ctx):
    """the reference's simTime runs without bound (main.cpp:515).  A frame at t = 500 s through
    a [495, 505] window equals the arithmetic frame, no table read is ever clamped, a time outside the window falls back to
    the arithmetic kernels, every coverage and both LAYOUTS give the same bytes -- dense (one box per table: unaddressable
    at full coverage that far along the clock, the differential rotation of the dust coordinates, see rrt.h) and, round 5,
    banded (the fine dust families in a box per omega band, the accretion table in a box per octave: full coverage at
    t = 500 s in under 2 GiB) -- and the drivers' policy object walks a clock across several windows inside its budget."""
    import torch
    g, rrt, tex = ctx
    views = [(960, 540, (4.2, 0.6, 4.2), -90.0, -5.7), (640, 360, (35.0, 0.8, 10.0), -106.0, -1.2), (480, 270, (0.0, 10.0, -60.0), 0.0, -10.0)]
    fx = rrt.CameraEffects()
    with pytest.raises(rrt.RRTError):
        rrt.NoiseTable.window(495.0, 505.0, rrt.TABLE_FULL | rrt.TABLE_DENSE)
    B, D = rrt.TABLE_BANDED, rrt.TABLE_DENSE
    for t0, t1, cov, t in ((495.0, 505.0, rrt.TABLE_FULL, 500.0), (495.0, 505.0, rrt.TABLE_FULL, 495.0), (495.0, 505.0, rrt.TABLE_FULL, 505.0),
                           (495.0, 505.0, rrt.TABLE_COARSE | D, 500.0), (495.0, 505.0, rrt.TABLE_COARSE | B, 500.0),
                           (495.0, 505.0, rrt.TABLE_COARSEST, 503.25),
                           (10.0, 20.0, rrt.TABLE_FULL, 14.0), (10.0, 20.0, rrt.TABLE_FULL | B, 14.0), (10.0, 20.0, rrt.TABLE_COARSE, 14.0),
                           (-8.0, -2.0, rrt.TABLE_FULL, -5.5), (-8.0, -2.0, rrt.TABLE_FULL | B, -5.5)):
        nt = rrt.NoiseTable.window(t0, t1, cov)
        try:
            info = nt.info()
            want_banded = bool(cov & B) or (t0 > 400.0 and (cov & 0xf) == rrt.TABLE_FULL)
            assert (info["t0"], info["t1"], info["coverage"] & 0xf) == (t0, t1, cov & 0xf) and info["bytes"] == rrt.NoiseTable.plan(t1, t0, cov)["bytes"]
            assert bool(info["coverage"] & B) == want_banded, (t0, t1, cov, info["coverage"])
            if t0 > 400.0 and (cov & 0xf) == rrt.TABLE_FULL:
                assert info["bytes"] <= 2 << 30
            for (w, h, pos, yaw, pitch) in views:
                cam = rrt.CameraState.from_angles(pos, yaw, pitch)
                ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda"); out = torch.zeros_like(ref)
                rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
                torch.cuda.synchronize()
                assert torch.equal(out, ref), (t0, t1, cov, t, pos)
                oob = torch.zeros(1, dtype=torch.int32, device="cuda")
                rrt.launch_raymarch_debug(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id), lut_oob=oob)
                torch.cuda.synchronize()
                assert torch.equal(out, ref) and int(oob.item()) == 0, (t0, t1, cov, t, pos)
                if want_banded and w == 640:             # ... and through the three-pass path (its own instantiations of the banded code)
                    ws = rrt.Workspace(96 << 20)
                    out.zero_()
                    rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2, pool_rounds=8))
                    torch.cuda.synchronize()
                    ws.destroy()
                    assert torch.equal(out, ref), ("three-pass", t0, t1, cov, t)
            # just outside the window: the arithmetic kernels, same bytes
            w, h, pos, yaw, pitch = views[1]
            cam = rrt.CameraState.from_angles(pos, yaw, pitch)
            for tt in (t0 - 0.5, t1 + 0.5):
                ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda"); out = torch.zeros_like(ref)
                rrt.launch_raymarch(ref, w, h, tt, cam, tex, fx, rrt.RenderParams(spin=0.9))
                rrt.launch_raymarch(out, w, h, tt, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
                torch.cuda.synchronize()
                assert torch.equal(out, ref), tt
        finally:
            nt.destroy()
    # the policy object of the frame drivers: 40 s of clock with a 0.3 GiB budget needs several windows
    nw = rrt.NoiseWindows(40.0, int(0.3 * (1 << 30)), sync=torch.cuda.synchronize)
    w, h, pos, yaw, pitch = views[1]
    cam = rrt.CameraState.from_angles(pos, yaw, pitch)
    ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda"); out = torch.zeros_like(ref)
    try:
        for k in range(0, 40 * 24, 37):
            t = k / 24.0
            rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nw.table_id(t)))
            torch.cuda.synchronize()
            assert torch.equal(out, ref), t
        sm = nw.summary()
        assert sm["builds"] >= 2 and sm["arith_frames"] == 0 and sm["peak_bytes"] <= sm["budget_bytes"], sm
    finally:
        nw.close()


def test_handles_are_tied_to_their_device(ctx, sky):
    """VERDICT r02 item 7 / ADVICE: a sky, workspace or noise table used while another device is current is
    RRT_ERR_BAD_HANDLE, not a wild device pointer in a kernel.  One GPU here, so "another device" is the test hook
    rrt_debug_fake_device() -- which only librrt_hip_test.so has (round 5), so the whole test talks to that library
    (_lib.using_test_library: the package's wrappers and the hook then share one set of registries); on the real device
    everything launches."""
    import ctypes as C
    import torch
    from relativisticraytracer_amd import _lib
    g, rrt, _ = ctx
    with _lib.using_test_library() as lib:
        tex = rrt.SkyTexture(sky)
        w, h = 64, 36
        cam = rrt.CameraState.default(); fx = rrt.CameraEffects()
        out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        nt = rrt.NoiseTable(2.0); ws = rrt.Workspace(64 << 20); order = rrt.TileOrder()
        real = torch.cuda.current_device()
        try:
            assert nt.info()["device"] == real
            rrt.launch_raymarch(out, w, h, 1.0, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2))
            torch.cuda.synchronize()
            ref = out.clone()
            lib.rrt_debug_fake_device(real + 1)
            for prm in (rrt.RenderParams(spin=0.9), rrt.RenderParams(spin=0.9, noise_table=nt.id)):
                with pytest.raises(rrt.RRTError) as e:
                    rrt.launch_raymarch(out, w, h, 1.0, cam, tex, fx, prm)
                assert e.value.status == 4
            # a sky of the "other" device with a table / pool of this one: each is checked on its own
            sky2 = C.c_ulonglong(0)
            assert lib.rrt_sky_create_from_device(C.c_void_p(out.data_ptr()), 8, 4, C.byref(sky2)) == 0      # registered under the fake device
            a = cam
            for prm in (rrt.RenderParams(spin=0.9, noise_table=nt.id), rrt.RenderParams(spin=0.9, workspace=ws.id, path_policy=2)):
                assert lib.rrt_launch_raymarch(C.c_void_p(out.data_ptr()), w, h, 1.0, C.byref(a), sky2, C.byref(fx), C.byref(prm), None) == 4
            assert lib.rrt_workspace_stats(ws.id, None, None) == 4
            assert lib.rrt_tile_order_info(order.id, None, None, None, None, None, 0) == 4
            prm = rrt.RenderParams(spin=0.9, tile_order=order.id)
            assert lib.rrt_launch_raymarch(C.c_void_p(out.data_ptr()), w, h, 1.0, C.byref(a), sky2, C.byref(fx), C.byref(prm), None) == 4
            # destroying a tile order (or tile map) from the wrong device is REFUSED and frees nothing (include/rrt.h): the raw call
            # says RRT_ERR_BAD_HANDLE, the Python wrapper raises and keeps its id, and the object still works afterwards
            assert lib.rrt_tile_order_destroy(order.id) == 4
            with pytest.raises(rrt.RRTError) as e:
                order.destroy()
            assert e.value.status == 4 and order.id != 0
            lib.rrt_sky_destroy(sky2)
            lib.rrt_debug_fake_device(-1)
            assert lib.rrt_tile_order_info(order.id, None, None, None, None, None, 0) == 0
            out.zero_()
            rrt.launch_raymarch(out, w, h, 1.0, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2))
            torch.cuda.synchronize()
            assert torch.equal(out, ref)
        finally:
            lib.rrt_debug_fake_device(-1)
            nt.destroy(); ws.destroy(); order.destroy(); tex.destroy()


# the frame sizes (w, h; wave tiles of 8 x 8 pixels) the test below sends through a tile-order object
ORDERED_FRAME_SIZES = ((640, 360), (333, 130), (8200, 8208), (1000, 700), (8, 8))


def test_cost_ordered_dispatch_renders_the_same_frames(ctx):
    """rrt_tile_order (round 3): launches through the object record per-wave-tile costs and the next launch of the same
    geometry dispatches longest-first.  Any order renders the same pixels: full frames, tile shards, fast mode, a
    geometry change in between, two streams sharing one object; the order handed out is a permutation sorted by cost."""
    import torch
    g, rrt, tex = ctx
    fx = rrt.CameraEffects(useChromaticAberration=True)
    nt = rrt.NoiseTable(16.0)
    views = [(rrt.CameraState.from_angles((4.2, 0.6, 4.2), -90.0, -5.7), 14.0), (rrt.CameraState.default(), 1.0)]
    order = rrt.TileOrder()
    try:
        w, h = ORDERED_FRAME_SIZES[0]
        n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
        ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda"); out = torch.zeros_like(ref)
        launches = ordered = 0
        for cam, t in views:
            for mode in (0, 1):
                plain = rrt.RenderParams(spin=0.9, noise_table=nt.id, arith_mode=mode)
                withorder = rrt.RenderParams(spin=0.9, noise_table=nt.id, arith_mode=mode, tile_order=order.id)
                rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, plain)
                for k in range(3):
                    out.zero_()
                    rrt.launch_raymarch(out, w, h, t, cam, tex, fx, withorder)
                    torch.cuda.synchronize()
                    assert torch.equal(out, ref), (mode, k)
                    launches += 1; ordered += 1 if launches > 1 else 0
                info = order.info(arrays=True)
                assert (info["launches"], info["ordered_launches"], info["n_tiles"]) == (launches, ordered, n_tiles)
                perm, cost = info["perm"], info["cost"]
                assert np.array_equal(np.sort(perm), np.arange(n_tiles, dtype=np.uint32))            # a permutation ...
                assert np.all(np.diff((cost[perm] >> 6).astype(np.int64)) <= 0) and cost.max() > 0     # ... longest first (in 0.5 us steps)
                # ... and exactly what a stable sort of the 16 key bits over the STATIC dispatch order gives (round 5, csrc/rrt_tile_sort.h:
                # tiles of equal cost keep the centre-out order of the static launch)
                gx, gy = (w + 7) // 8, (h + 7) // 8
                j = np.arange(gy); mid = (gy - 1) >> 1
                rb = np.where(j & 1, mid + ((j + 1) >> 1), mid - (j >> 1))
                static = (rb[:, None] * gx + np.arange(gx)[None, :]).reshape(-1)
                keys = (cost[static] >> 6) & 0xffff
                assert np.array_equal(perm, static[np.argsort(-keys.astype(np.int64), kind="stable")])
        # another geometry: ordered by the coarse probe (round 4; no history to go by), and the object starts over
        w2, h2 = ORDERED_FRAME_SIZES[1]
        ref2 =torch.zeros(h2 * w2 * 4, dtype=torch.uint8, device="cuda"); out2 = torch.zeros_like(ref2)
        cam, t = views[0]
        rrt.launch_raymarch(ref2, w2, h2, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
        for k in range(2):
            rrt.launch_raymarch(out2, w2, h2, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id, tile_order=order.id))
            torch.cuda.synchronize()
            assert torch.equal(out2, ref2)
        info = order.info()
        assert info["launches"] == launches + 2 and info["ordered_launches"] == ordered + 1
        assert info["n_tiles"] == ((w2 + 7) // 8) * ((h2 + 7) // 8)
        # tile shards (their own row map), and two streams sharing the object: the library chains them
        rows = rrt.tile_shard_rows(h, 16, 1, 3)
        sref = torch.zeros(rows * w * 4, dtype=torch.uint8, device="cuda"); sout = [torch.zeros_like(sref) for _ in range(2)]
        rrt.launch_raymarch_tiles(sref, w, h, 16, 1, 3, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for k in range(6):
            with torch.cuda.stream(streams[k % 2]):
                rrt.launch_raymarch_tiles(sout[k % 2], w, h, 16, 1, 3, t, cam, tex, fx,
                                          rrt.RenderParams(spin=0.9, noise_table=nt.id, tile_order=order.id), stream=streams[k % 2])
        torch.cuda.synchronize()
        assert torch.equal(sout[0], sref) and torch.equal(sout[1], sref)
        # the three-pass path takes the object too (round 4), debug launches ignore it; a wrong id is a bad handle
        ws = rrt.Workspace(256 << 20)
        rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id, workspace=ws.id, path_policy=2, tile_order=order.id))
        rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, noise_table=nt.id))
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
        ws.destroy()
        with pytest.raises(rrt.RRTError) as e:
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9, tile_order=order.id + 1000))
        assert e.value.status == 4
        # the sort on a large geometry (1 051 650 tiles: 514 blocks) and on ragged ones: a few march steps per ray are enough to give the
        # tiles costs; the order must be the stable sort.  All of them run at ONE batch per block (csrc/rrt_tile_sort.h: reps_for
        # exceeds 1 past 2 097 152 tiles; tests/test_tile_sort_geometry.py asserts it of ORDERED_FRAME_SIZES): the chunkings with
        # 2 and 4 batches, and keys the test chooses, are tests/test_gpu_tile_sort.py
        for wb, hb in ORDERED_FRAME_SIZES[2:]:
            big = torch.zeros(hb * wb * 4, dtype=torch.uint8, device="cuda")
            for _ in range(2):
                rrt.launch_raymarch(big, wb, hb, 1.0, views[1][0], tex, fx, rrt.RenderParams(spin=0.9, max_steps=6, tile_order=order.id))
            torch.cuda.synchronize()
            info = order.info(arrays=True)
            gx, gy = (wb + 7) // 8, (hb + 7) // 8
            assert info["n_tiles"] == gx * gy
            j = np.arange(gy); mid = (gy - 1) >> 1
            rb = np.where(j & 1, mid + ((j + 1) >> 1), mid - (j >> 1))
            static = (rb[:, None] * gx + np.arange(gx)[None, :]).reshape(-1)
            keys = (info["cost"][static] >> 6) & 0xffff
            assert np.array_equal(info["perm"], static[np.argsort(-keys.astype(np.int64), kind="stable")]), (wb, hb)
            del big
    finally:
        order.destroy(); nt.destroy()


def test_full_size_properties_4k(ctx):
    """BASELINE config at full size: properties that need no oracle.
    Two launches give identical bytes (no races); every alpha is 255; the image is left-right
    symmetric for a = 0 only in the geodesic sense, so we check determinism + shard identity on
    a 4K strip instead."""
    import torch
    g, rrt, tex = ctx
    w, h = 3840, 2160
    cam = rrt.CameraState.default(); fx = rrt.CameraEffects(); prm = rrt.RenderParams(spin=0.9)
    a = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(a, w, h, 1.0, cam, tex, fx, prm)
    torch.cuda.synchronize()
    img = a.view(h, w, 4)
    assert bool((img[..., 3] == 255).all())
    # a 4K strip rendered as a shard equals the same rows of the full frame
    y0, y1 = 1000, 1064
    strip = torch.zeros((y1 - y0) * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch_rows(strip, w, h, y0, y1, 1.0, cam, tex, fx, prm)
    torch.cuda.synchronize()
    assert torch.equal(strip, a[(h - y1) * w * 4:(h - y0) * w * 4])
    # the shadow exists and the disk is bright: coarse sanity of the physical picture
    lum = img[..., :3].float().mean(dim=2)
    assert float(lum.max()) > 200 and float((lum < 2).float().mean()) > 0.001


def test_pipelined_sharder_over_one_rank_rccl(ctx):
    """FrameSharder with two frames in flight through a one-rank RCCL group (async gather, wait, assemble on
    alternating streams): every frame equals the single launch of the same time."""
    import socket
    import torch
    import torch.distributed as dist
    from relativisticraytracer_amd import sharding
    _, rrt, tex = ctx
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    pools = [rrt.Workspace(256 << 20), rrt.Workspace(256 << 20)]
    try:
        w, h, R = 320, 180, 16
        cam, fx = rrt.CameraState.default(), rrt.CameraEffects()
        prms = [rrt.RenderParams(spin=0.9, workspace=p.id) for p in pools]
        times = [1.0, 2.5, 4.0, 5.5, 7.0]
        n = {"i": 0}

        def render(buf, slot):
            rrt.launch_raymarch_tiles(buf, w, h, R, 0, 1, times[n["i"]], cam, tex, fx, prms[slot]); n["i"] += 1

        fs = sharding.FrameSharder(w, h, R, 0, 1, "cuda", render, None, pipeline=True, collective_at_world1=True,
                                   assemble_all=lambda f, b, st: rrt.assemble_all_tiles(f, b, st, w, h, R, 1))
        got = []
        for _ in times:
            f = fs.step()
            if f is not None:
                got.append(f.clone())
        got.append(fs.flush().clone())
        assert len(got) == len(times)
        ref = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
        for k, t in enumerate(times):
            rrt.launch_raymarch(ref, w, h, t, cam, tex, fx, rrt.RenderParams(spin=0.9))
            torch.cuda.synchronize()
            assert torch.equal(ref, got[k]), k
    finally:
        for p in pools:
            p.destroy()
        dist.destroy_process_group()


def test_randomized_sweep_every_launch_variant_matches_oracle(ctx, po, sky):
    """Seeded random scenes (camera anywhere from inside the disk to far out, any orientation, spin of either
    sign, random time / effects / ragged size): the single kernel, the three-pass path with an ample and with
    a starved pool, cost-ordered dispatch, and interleaved tile shards must all give the oracle's bytes (portable math mode).
    On even scenes the FMAD single kernel equals the oracle's FMAD mode, and every FMAD path the single kernel."""
    import torch
    g, rrt, tex = ctx
    rng = np.random.default_rng(int(os.environ.get("RRT_SWEEP_SEED", "20261004")))     # soaks vary the seed
    ample, starved = rrt.Workspace(512 << 20), rrt.Workspace(13 << 20)     # 13 MiB: the smallest useful pool
    mid = rrt.Workspace(64 << 20)                                          # two chains need >= 4096 blocks: rounds AND chains
    nt = rrt.NoiseTable(30.0)
    nt_banded = rrt.NoiseTable.window(0.0, 30.0, rrt.TABLE_FULL | rrt.TABLE_BANDED)
    order = rrt.TileOrder()
    order3 = rrt.TileOrder()
    try:
        overflowed = 0
        for case in range(int(os.environ.get("RRT_SWEEP_CASES", "60"))):      # soak: RRT_SWEEP_CASES=600 (run on the round's final build)
            if case % 100 == 99:
                print(f"sweep: {case + 1} scenes", flush=True)            # visible with -s: long soaks show progress
            w, h = int(rng.integers(9, 80)), int(rng.integers(5, 48))
            rad = float(np.exp(rng.uniform(np.log(3.0), np.log(120.0))))
            ang = float(rng.uniform(0, 2 * np.pi))
            height = float(rng.normal(0, 0.15) * rad if case % 2 else rng.normal(0, 0.6))
            pos = (rad * np.cos(ang), height, rad * np.sin(ang))
            # mostly looking towards the hole (so that the media are in view), jittered; sometimes anywhere
            yaw_in = np.degrees(np.arctan2(-pos[0], -pos[2]))
            yaw = float(yaw_in + rng.normal(0, 25)) if case % 5 else float(rng.uniform(-180, 180))
            pitch = float(np.clip(-np.degrees(np.arctan2(height, rad)) + rng.normal(0, 12), -89, 89))
            spin = float(rng.choice([0.0, 0.3, 0.9, 0.99, -0.7]))
            t = float(rng.uniform(0, 30))
            fxkw = dict(useBloom=bool(rng.integers(2)), useVignette=bool(rng.integers(2)),
                        useLensDistortion=bool(rng.integers(2)), useChromaticAberration=bool(rng.integers(2)),
                        bloomThreshold=float(rng.uniform(0.3, 1.2)), bloomIntensity=float(rng.uniform(0, 1)),
                        vignetteIntensity=float(rng.uniform(0, 0.8)), caAmount=float(rng.uniform(0, 0.02)),
                        distortionAmount=float(rng.uniform(-0.2, 0.3)))
            cam = rrt.CameraState.from_angles(pos, yaw, pitch)
            fx = rrt.CameraEffects(**fxkw)
            a = cam.as_array()
            ofx = po.default_effects(use_bloom=int(fxkw["useBloom"]), use_vignette=int(fxkw["useVignette"]),
                                     use_lens=int(fxkw["useLensDistortion"]), use_ca=int(fxkw["useChromaticAberration"]),
                                     bloom_threshold=fxkw["bloomThreshold"], bloom_intensity=fxkw["bloomIntensity"],
                                     vignette_intensity=fxkw["vignetteIntensity"], ca_amount=fxkw["caAmount"],
                                     distortion_amount=fxkw["distortionAmount"])
            o = po.render(po.camera(a[0], a[1], a[2], a[3]), ofx,
                          po.default_params(spin=spin, math_mode=po.MATH_PORTABLE), t, w, h, sky,
                          want=("rgba8", "ldr", "diag"))
            tag = (case, w, h, pos, yaw, pitch, spin, t, fxkw)
            r = g.render_gpu(w, h, spin, 1, cam, t, tex, fx=fx)
            assert np.array_equal(r["steps"], o["steps"]) and np.array_equal(r["hit"], o["hit"]), tag
            assert np.array_equal(r["rgba8"], o["rgba8"]) and same_bits(r["ldr"], o["ldr"]), tag
            r = g.render_gpu(w, h, spin, 1, cam, t, tex, fx=fx, noise_table=nt.id)       # same through the noise tables
            assert np.array_equal(r["rgba8"], o["rgba8"]) and same_bits(r["ldr"], o["ldr"]), tag
            assert int(r["lut_oob"][0]) == 0, tag
            for table in (0, nt.id):                                                     # the production instantiations (debug off)
                r = g.render_gpu(w, h, spin, 1, cam, t, tex, fx=fx, debug=False, noise_table=table)
                assert np.array_equal(r["rgba8"], o["rgba8"]), (tag, "production kernel", table)
            want = torch.from_numpy(o["rgba8"].reshape(-1)).cuda()
            for rep in range(2):            # cost-ordered dispatch: the first launch of a geometry in the static order, the second longest-first
                out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin, noise_table=nt.id if case % 2 else 0, tile_order=order.id))
                torch.cuda.synchronize()
                assert torch.equal(out, want), (tag, "tile order", rep)
            for pool in (ample, starved):
                out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx,
                                    rrt.RenderParams(spin=spin, workspace=pool.id, path_policy=2,
                                                     noise_table=nt.id if case % 2 else 0))
                torch.cuda.synchronize()
                assert torch.equal(out, want), (tag, pool.nbytes, pool.stats())
            overflowed += starved.stats()["overflow_waves"]
            # round 4: rounds over a small pool (nothing may take the in-line route), two chains forced on these small
            # launches, the three-pass path under cost-ordered dispatch (probe-seeded on a scene's first launch)
            for pool, rounds, chains, oid in ((starved, 64, 1, 0), (mid, 48, 2, 0), (ample, 0, 2, order3.id), (mid, 48, 2, order3.id)):
                out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx,
                                    rrt.RenderParams(spin=spin, workspace=pool.id, path_policy=2, pool_rounds=rounds, pass_chains=chains,
                                                     tile_order=oid, noise_table=nt.id if case % 2 else 0))
                torch.cuda.synchronize()
                assert torch.equal(out, want), (tag, "rounds / chains", pool.nbytes, rounds, chains, oid, pool.stats())
                if rounds:
                    assert pool.stats()["overflow_waves"] == 0, (tag, pool.nbytes, pool.stats())
            n, R = int(rng.integers(2, 6)), int(rng.integers(1, 9))
            frame = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            for s in range(n):
                rows = rrt.tile_shard_rows(h, R, s, n)
                buf = torch.zeros(max(rows, 1) * w * 4, dtype=torch.uint8, device="cuda")
                if rows:
                    rrt.launch_raymarch_tiles(buf, w, h, R, s, n, t, cam, tex, fx,
                                              rrt.RenderParams(spin=spin, workspace=ample.id, path_policy=2 * (s % 2)))
                    rrt.assemble_tiles(frame, buf, w, h, R, s, n)
            torch.cuda.synchronize()
            assert torch.equal(frame, want), (tag, n, R)
            # the same shards under an arbitrary tile -> shard map, gathered layout, one assemble
            n_tiles = (h + R - 1) // R
            tm = rrt.TileMap(h, R, n, rng.integers(0, n, n_tiles).astype(np.int32))
            stride = max(tm.max_shard_rows(), 1) * w * 4
            allbuf = torch.zeros(n * stride, dtype=torch.uint8, device="cuda")
            for s in range(n):
                if tm.shard_rows(s):
                    rrt.launch_raymarch_tilemap(allbuf[s * stride:], w, h, tm, s, t, cam, tex, fx,
                                                rrt.RenderParams(spin=spin, workspace=ample.id, path_policy=2 * (s % 2), noise_table=nt.id if case % 2 else 0))
            frame.zero_()
            rrt.assemble_all_tilemap(frame, allbuf, stride, w, h, tm)
            torch.cuda.synchronize()
            assert torch.equal(frame, want), (tag, "tile map", n, R)
            tm.destroy()
            # round 5: the BANDED table layout (forced: near the origin of the clock the automatic choice is dense) -- the oracle's bytes,
            # single kernel and three-pass, no clamped read; and the within-tolerance modes are one function on every path
            r = g.render_gpu(w, h, spin, 1, cam, t, tex, fx=fx, noise_table=nt_banded.id)
            assert np.array_equal(r["rgba8"], o["rgba8"]) and same_bits(r["ldr"], o["ldr"]) and int(r["lut_oob"][0]) == 0, (tag, "banded table")
            out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
            rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin, workspace=mid.id, path_policy=2, pool_rounds=48,
                                                                              pass_chains=1 + case % 2, noise_table=nt_banded.id))
            torch.cuda.synchronize()
            assert torch.equal(out, want), (tag, "banded table, three-pass")
            mode = 2 - case % 2                       # RRT_ARITH_FMAD on even scenes, RRT_ARITH_FAST on odd ones
            rmd = g.render_gpu(w, h, spin, 1, cam, t, tex, fx=fx, arith_mode=mode)
            rm = rmd["rgba8"]
            if mode == 2:                             # FMAD has a restatement: the oracle's FMAD mode, same equalities as strict
                of = po.render(po.camera(a[0], a[1], a[2], a[3]), ofx,
                               po.default_params(spin=spin, math_mode=po.MATH_PORTABLE, arith_mode=po.ARITH_FMAD), t, w, h, sky,
                               want=("rgba8", "ldr", "diag"))
                assert np.array_equal(rmd["steps"], of["steps"]) and np.array_equal(rmd["hit"], of["hit"]), (tag, "FMAD oracle")
                assert np.array_equal(rm, of["rgba8"]) and same_bits(rmd["ldr"], of["ldr"]), (tag, "FMAD oracle")
            wantm = torch.from_numpy(rm.reshape(-1)).cuda()
            for kw in (dict(noise_table=nt.id), dict(noise_table=nt_banded.id, workspace=starved.id, path_policy=2, pool_rounds=64),
                       dict(workspace=mid.id, path_policy=2, pool_rounds=48, pass_chains=2, tile_order=order3.id)):
                out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
                rrt.launch_raymarch(out, w, h, t, cam, tex, fx, rrt.RenderParams(spin=spin, arith_mode=mode, **kw))
                torch.cuda.synchronize()
                assert torch.equal(out, wantm), (tag, "mode", mode, kw)
        assert overflowed > 0          # the starved pool did exercise the overflow route somewhere in the sweep
        info = order.info()
        assert info["ordered_launches"] >= info["launches"] // 2       # every scene's second launch (at least) was cost-ordered
    finally:
        ample.destroy(); starved.destroy(); mid.destroy(); nt.destroy(); nt_banded.destroy(); order.destroy(); order3.destroy()
