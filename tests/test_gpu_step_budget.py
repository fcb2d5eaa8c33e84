"""The step budget (rrt_params.max_steps) on frames: every launch path at budgets from 1 to 1999, against the oracle rendered live
at the same budget.

"Out of steps" is the march loop's least-travelled exit: at the default 2000 only a few dozen rays of a small frame reach it, and
whether one of them does so inside the wave-uniform vacuum loop (rrt_kernels.h: vacuum_run, `return 2` at either position of its
doubled body), at the re-test after a wave-mate escaped, in the middle of a media run, in a three-pass round or right after a
pool-overflow resume depends on its 63 wave-mates.  A budgeted frame puts whole frames there: at 1..5 every wave runs out in its
first vacuum steps (both positions of the doubled body, the steps before the seed extrapolation starts); at a few hundred the
budget ends among the media samples; around 1000 a frame holds escaped, fallen-in and out-of-steps rays side by side.

COVERAGE IS A CONDITION: test_budget_set_meets_the_coverage_conditions computes, from the oracle's own per-ray diagnostics and
without a GPU, that the (view, spin, budget) set really holds such frames.

Strict and FMAD arithmetic: everything equals the oracle in the same arithmetic mode (FMAD: the oracle's fixed fused tree,
DESIGN.md section 2) and its portable math mode -- equality, no tolerance.  Every other path must give the single kernel's bytes
exactly.  FAST has no restatement (a hardware reciprocal root): its single kernel, and FMAD's beside it, is also held to the
suite's bars against the libm oracle at the same budget (test_gpu_frames.py::test_tolerance_modes_against_the_libm_oracle)."""
import numpy as np
import pytest

import march_ref as mr
from conftest import same_bits

gpu = pytest.mark.gpu

W, H = 61, 37                       # ragged: partial waves on both edges
T = 2.5
VIEWS = ("default", "skimmer", "in_disk", "far")
SPINS = (0.9, 0.0)
FIXED = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 100, 150, 200, 300, 600, 1000, 1999)
DRAWN = tuple(int(x) for x in np.random.default_rng(20261016).choice(np.arange(6, 1999), 5, replace=False))
BUDGETS = tuple(sorted(set(FIXED + DRAWN)))
CASES = [(view, spin, n) for view in VIEWS for spin in SPINS for n in BUDGETS]
# rrt_hip.hip: kThreePassMaxSteps = (kMaxRunsWalked - 8) * kMaxRun * kBlockRows -- launches with more steps take the single kernel
THREE_PASS_MAX_STEPS = (4096 - 8) * 8 * 8

_ORACLE = {}


def camera(view):
    import relativisticraytracer_amd as rrt
    return rrt.CameraState.from_angles(*mr.VIEWS[view])


def oracle(po, sky, view, spin, n, vol=1, libm=False, arith=0):
    """the oracle's frame and per-ray diagnostics of a case (chromatic aberration on, like the GPU launches below) in arithmetic
    `arith` (0 strict, 2 FMAD); kept for the other tests of the process"""
    key = (view, spin, n, vol, libm) + ((arith,) if arith else ())
    if key not in _ORACLE:
        a = camera(view).as_array()
        prm = po.default_params(spin=spin, volumetrics=vol, max_steps=n, math_mode=po.MATH_LIBM if libm else po.MATH_PORTABLE,
                                arith_mode=arith)
        _ORACLE[key] = po.render(po.camera(a[0], a[1], a[2], a[3]), po.default_effects(use_ca=1), prm, T, W, H, sky,
                                 want=("rgba8", "ldr", "hdr", "diag"))
    return _ORACLE[key]


def coverage(po, sky):
    """which cases hold: whole frames out of steps in the far vacuum (odd / even budget), rays out of steps near the hole, rays
    out of steps in the middle of the medium, frames that mix escaped, hit and out-of-steps rays"""
    cov = {"vacuum_odd": [], "vacuum_even": [], "near_hole": [], "mid_medium": [], "mixed": []}
    for view, spin, n in CASES:
        o = oracle(po, sky, view, spin, n)
        out = (o["steps"] == n) & (o["hit"] == 0)
        r = np.linalg.norm(o["pos"].astype(np.float64), axis=1)
        r0 = float(np.linalg.norm(camera(view).as_array()[0].astype(np.float64)))
        # every ray out of steps at r >= 30 and too few steps of 0.3 to have been any closer: the whole frame inside vacuum_run
        if out.all() and (r >= 30.0).all() and r0 - 0.3 * n >= 30.0 and not o["n_samples"].any():
            cov["vacuum_odd" if n % 2 else "vacuum_even"].append((view, spin, n))
        if (out & (r < 18.0)).any():
            cov["near_hole"].append((view, spin, n, int((out & (r < 18.0)).sum())))
        if (out & (o["rad"][:, 3] < 1.0)).any():
            cov["mid_medium"].append((view, spin, n, int((out & (o["rad"][:, 3] < 1.0)).sum())))
        if out.any() and (o["hit"] == 1).any() and ((o["hit"] == 0) & ~out).any():
            cov["mixed"].append((view, spin, n))
    return cov


def test_budget_set_meets_the_coverage_conditions(po, sky):
    cov = coverage(po, sky)
    print({k: len(v) for k, v in cov.items()})
    assert len(cov["vacuum_odd"]) >= 4 and len(cov["vacuum_even"]) >= 4, cov
    assert {c[0] for c in cov["vacuum_odd"]} >= {"default", "far"} and {c[0] for c in cov["vacuum_even"]} >= {"default", "far"}
    assert len(cov["near_hole"]) >= 4 and len(cov["mid_medium"]) >= 4 and len(cov["mixed"]) >= 4, cov
    assert {c[1] for c in cov["mid_medium"]} == set(SPINS) and {c[1] for c in cov["mixed"]} == set(SPINS)
    assert len(BUDGETS) == len(FIXED) + len(DRAWN) and min(BUDGETS) == 1 and max(BUDGETS) == 1999


# ------------------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def ctx(sky):
    import torch
    assert torch.cuda.is_available(), "the -m gpu tests need a GPU"
    import gpu_util
    import relativisticraytracer_amd as rrt
    tex = rrt.SkyTexture(sky)
    yield gpu_util, rrt, tex
    tex.destroy()


def fx_of(rrt):
    return rrt.CameraEffects(useChromaticAberration=True)


def launch(rrt, tex, cam, prm, w=W, h=H):
    """the production launch's bytes, (h, w, 4)"""
    import torch
    out = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(out, w, h, T, cam, tex, fx_of(rrt), prm)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(h, w, 4)


@gpu
@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("view", VIEWS)
def test_strict_frames_equal_the_oracle_at_every_budget(ctx, po, sky, view, spin):
    """the debug launch (per-ray state, HDR, LDR, bytes) and the production launch (bytes), volumetrics on and off, and the
    production launch through a noise table: everything equals the oracle at the same budget"""
    g, rrt, tex = ctx
    cam = camera(view)
    nt = rrt.NoiseTable(4.0)
    try:
        for n in BUDGETS:
            for vol in (1, 0):
                o = oracle(po, sky, view, spin, n, vol)
                r = g.render_gpu(W, H, spin, vol, cam, T, tex, fx=fx_of(rrt), max_steps=n)
                what = (view, spin, n, vol)
                assert np.array_equal(r["steps"], o["steps"]), (what, int((r["steps"] != o["steps"]).sum()))
                assert np.array_equal(r["hit"], o["hit"]), what
                assert np.array_equal(r["rgba8"], o["rgba8"]), what
                for k in ("pos", "vel", "rad", "hdr", "ldr"):
                    assert same_bits(r[k], o[k]), (what, k)
                prod = g.render_gpu(W, H, spin, vol, cam, T, tex, fx=fx_of(rrt), max_steps=n, debug=False)
                assert np.array_equal(prod["rgba8"], o["rgba8"]), what
            tab = g.render_gpu(W, H, spin, 1, cam, T, tex, fx=fx_of(rrt), max_steps=n, debug=False, noise_table=nt.id)
            assert np.array_equal(tab["rgba8"], oracle(po, sky, view, spin, n)["rgba8"]), (view, spin, n, "noise table")
    finally:
        nt.destroy()


FMAD_VOL_OFF = (1, 200, 1999)      # volumetrics off costs the oracle a second frame per budget: the ends and the middle only


def test_fmad_oracle_frames_are_not_the_strict_ones(po, sky):
    """a condition of the test below: at the budgets that leave room for it the FMAD oracle's per-ray state differs from the
    strict oracle's, so a kernel that ran strict arithmetic under the FMAD switch could not pass"""
    for view in VIEWS:
        for spin in SPINS:
            a, b = oracle(po, sky, view, spin, 150), oracle(po, sky, view, spin, 150, arith=2)
            assert (a["pos"].view(np.uint32) != b["pos"].view(np.uint32)).any(axis=1).mean() > 0.3, (view, spin)


@gpu
@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("view", VIEWS)
def test_fmad_frames_equal_the_fmad_oracle_at_every_budget(ctx, po, sky, view, spin):
    """the twin of the strict test above in RRT_ARITH_FMAD: the debug launch's per-ray state, HDR, LDR and bytes equal the
    oracle's FMAD mode at the same budget, the production launch and the noise-table launch give the same bytes; volumetrics
    off at the first, a middle and the last budget"""
    g, rrt, tex = ctx
    cam = camera(view)
    nt = rrt.NoiseTable(4.0)
    try:
        for n in BUDGETS:
            for vol in ((1, 0) if n in FMAD_VOL_OFF else (1,)):
                o = oracle(po, sky, view, spin, n, vol, arith=2)
                r = g.render_gpu(W, H, spin, vol, cam, T, tex, fx=fx_of(rrt), max_steps=n, arith_mode=2)
                what = (view, spin, n, vol)
                assert np.array_equal(r["steps"], o["steps"]), (what, int((r["steps"] != o["steps"]).sum()))
                assert np.array_equal(r["hit"], o["hit"]), what
                for k in ("pos", "vel", "rad", "hdr", "ldr"):
                    assert same_bits(r[k], o[k]), (what, k, int((~((r[k].view(np.uint32) == o[k].view(np.uint32)) | ((r[k] == 0) & (o[k] == 0)))).sum()))
                assert np.array_equal(r["rgba8"], o["rgba8"]), what
                prod = g.render_gpu(W, H, spin, vol, cam, T, tex, fx=fx_of(rrt), max_steps=n, debug=False, arith_mode=2)
                assert np.array_equal(prod["rgba8"], o["rgba8"]), what
            tab = g.render_gpu(W, H, spin, 1, cam, T, tex, fx=fx_of(rrt), max_steps=n, debug=False, noise_table=nt.id, arith_mode=2)
            assert np.array_equal(tab["rgba8"], oracle(po, sky, view, spin, n, arith=2)["rgba8"]), (view, spin, n, "noise table")
    finally:
        nt.destroy()


@gpu
@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("view", VIEWS)
def test_three_pass_paths_give_the_single_kernel_bytes_at_every_budget(ctx, view, spin):
    """workspace + path_policy = 2: a roomy pool, a pool small enough to overflow with pool_rounds = 1 (what does not fit is
    resumed in line: the resumed march meets the budget) and the same pool with pool_rounds = 3 (resume rounds meet it) -- the
    bytes of the single kernel (which the test above pins to the oracle), in all three arithmetic modes"""
    g, rrt, tex = ctx
    cam = camera(view)
    roomy, small = rrt.Workspace(256 << 20), rrt.Workspace(11 << 20)      # 11 MiB: just above the smallest pool the path takes (1024 blocks)
    overflowed, resumed_rounds, pooled = [], [], []
    try:
        for arith in (0, 2, 1):
            for n in BUDGETS:
                ref = launch(rrt, tex, cam, rrt.RenderParams(spin=spin, arith_mode=arith, max_steps=n))
                for ws, rounds in ((roomy, 0), (small, 1), (small, 3)):
                    got = launch(rrt, tex, cam, rrt.RenderParams(spin=spin, arith_mode=arith, max_steps=n, workspace=ws.id,
                                                                 path_policy=2, pool_rounds=rounds))
                    st = ws.stats()
                    assert np.array_equal(got, ref), (view, spin, arith, n, ws.nbytes, rounds, st, int((got != ref).any(-1).sum()))
                    if ws is roomy:
                        assert st["overflow_waves"] == 0, st
                        pooled.append(st["rows_used"])
                    elif rounds == 1 and st["overflow_waves"] > 0:
                        overflowed.append(n)
                    elif rounds == 3 and st["rounds_with_work"] > 1:
                        resumed_rounds.append(n)
        print(view, spin, "most rows pooled", max(pooled), "overflowed at", sorted(set(overflowed)), "resume rounds at", sorted(set(resumed_rounds)))
        if view in ("skimmer", "in_disk"):        # the medium is reached: rows are pooled
            assert max(pooled) > 0
        if view == "in_disk":                     # every wave pools a row per step: the small pool really overflows
            assert len(set(overflowed)) >= 3 and len(set(resumed_rounds)) >= 3, (overflowed, resumed_rounds)
    finally:
        roomy.destroy(); small.destroy()


@gpu
@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("view", VIEWS)
def test_row_and_tile_shards_reassemble_at_every_budget(ctx, view, spin):
    """row shards with odd first rows (they shift the wave tiles: other wave-mates for every ray) and interleaved tile shards
    reassemble to the single launch's bytes, in all three arithmetic modes"""
    import torch
    g, rrt, tex = ctx
    cam = camera(view); fx = fx_of(rrt)
    for arith in (0, 2, 1):
        for n in BUDGETS:
            prm = rrt.RenderParams(spin=spin, arith_mode=arith, max_steps=n)
            full = torch.from_numpy(launch(rrt, tex, cam, prm).reshape(-1)).cuda()
            rows = torch.zeros_like(full)
            for (y0, y1) in ((0, 7), (7, 21), (21, 37)):
                rrt.launch_raymarch_rows(rows[(H - y1) * W * 4:], W, H, y0, y1, T, cam, tex, fx, prm)
            torch.cuda.synchronize()
            assert torch.equal(rows, full), (view, spin, arith, n, "rows")
            for n_shards, R in ((3, 8), (2, 7)):
                tiles = torch.zeros_like(full)
                for s in range(n_shards):
                    buf = torch.zeros(max(rrt.tile_shard_rows(H, R, s, n_shards), 1) * W * 4, dtype=torch.uint8, device="cuda")
                    rrt.launch_raymarch_tiles(buf, W, H, R, s, n_shards, T, cam, tex, fx, prm)
                    rrt.assemble_tiles(tiles, buf, W, H, R, s, n_shards)
                torch.cuda.synchronize()
                assert torch.equal(tiles, full), (view, spin, arith, n, n_shards, R)


@gpu
def test_a_budget_above_the_three_pass_limit_takes_the_single_kernel(ctx):
    """max_steps just above what the three-pass bookkeeping can represent: a launch with a workspace and path_policy = 2 gives the
    single kernel's bytes and pools nothing; at the limit itself the same launch does pool rows"""
    g, rrt, tex = ctx
    w, h = 32, 20
    cam = camera("skimmer")
    for arith in (0, 2):
        for n, three_pass in ((THREE_PASS_MAX_STEPS, True), (THREE_PASS_MAX_STEPS + 1, False)):
            ws = rrt.Workspace(64 << 20)
            try:
                ref = launch(rrt, tex, cam, rrt.RenderParams(spin=0.9, arith_mode=arith, max_steps=n), w, h)
                got = launch(rrt, tex, cam, rrt.RenderParams(spin=0.9, arith_mode=arith, max_steps=n, workspace=ws.id, path_policy=2), w, h)
                assert np.array_equal(got, ref), (arith, n)
                assert (ws.stats()["rows_used"] > 0) == three_pass, (arith, n, ws.stats())
                assert ref[..., :3].std() > 5.0
            finally:
                ws.destroy()


# (view, budget): the budget ends in the far vacuum for every ray / among the media samples for some (coverage() says so)
SAMPLED = (("default", 33), ("skimmer", 200))


def test_sampled_cases_end_where_they_are_meant_to(po, sky):
    cov = coverage(po, sky)
    assert ("default", 0.9, 33) in cov["vacuum_odd"]
    assert any(c[:3] == ("skimmer", 0.9, 200) for c in cov["mid_medium"])


@gpu
@pytest.mark.parametrize("view,n", SAMPLED)
def test_supersampled_frames_honour_the_budget(ctx, po, view, n):
    """launch_raymarch_ss, s = 1, 2, 4: the tree over the budgeted 1x frame of (s w) x (s h) (test_gpu_supersample.check_parity);
    s = 1 gives the single kernel's bytes in every arithmetic mode"""
    from sampled_util import check_parity_ss as check_parity, render_ss
    g, rrt, tex = ctx
    cam = camera(view)
    for arith in (0, 2):
        prm = rrt.RenderParams(spin=0.9, arith_mode=arith, max_steps=n)
        for s in (1, 2, 4):
            check_parity(po, rrt, tex, W, H, s, T, cam, fx_of(rrt), prm, (view, n, arith, s))
    for arith in (0, 2, 1):
        prm = rrt.RenderParams(spin=0.9, arith_mode=arith, max_steps=n)
        got8, _ = render_ss(rrt, tex, W, H, 1, T, cam, fx_of(rrt), prm)
        assert np.array_equal(got8, launch(rrt, tex, cam, prm)), (view, n, arith)


def _sub_frames(rrt, cam, k):
    from sampled_util import moving_cameras
    return [T + 0.05 * j for j in range(k)], moving_cameras(rrt, {"cam": cam.as_array()}, k, step=0.35)


@gpu
@pytest.mark.parametrize("view,n", SAMPLED + (("default", 2000),))
def test_motion_blur_honours_the_budget_in_every_sub_frame(ctx, po, view, n):
    """launch_raymarch_mb with K = 2, 8 and 16 DISTINCT times and cameras (test_gpu_motion_blur.check_parity): every sub-frame is
    the budgeted 1x frame, and the tree over k closes levels 1, 2 and 3 with data that can tell an ordering error (equal sub-frames
    cannot).  At the default budget too, on a small frame."""
    from sampled_util import check_parity_mb as check_parity
    g, rrt, tex = ctx
    cam = camera(view)
    w, h = (W, H) if n != 2000 else (29, 17)
    for arith in (0, 2):
        prm = rrt.RenderParams(spin=0.9, arith_mode=arith, max_steps=n)
        for k in (2, 8, 16):
            times, cams = _sub_frames(rrt, cam, k)
            for s in ((1, 2) if k == 8 else (1,)):
                check_parity(po, rrt, tex, w, h, s, times, cams, fx_of(rrt), prm, (view, n, arith, k, s))


def _probe_matches(got, want):
    return ((got.view(np.uint32) == want.view(np.uint32)) | ((got == 0) & (want == 0))).all(-1)


@gpu
@pytest.mark.parametrize("view,n", SAMPLED)
def test_panoramas_honour_the_budget(ctx, po, view, n):
    """launch_raymarch_pano at the budget: 128 random inside pixels per configuration march the pinned pinhole path at the same
    budget (the check of test_gpu_projection.py::test_every_pixel_marches_the_pinned_pinhole_path, with max_steps in both)"""
    import projection_ref as pr
    from sampled_util import all_fx_pano as all_fx, probe_hdr_pano as _probe_hdr, render_pano
    g, rrt, tex = ctx
    rng = np.random.default_rng(n)
    cam = camera(view)
    for proj, PW, PH in ((rrt.Projection("equirect"), 96, 48), (rrt.Projection("fisheye", 220.0), 64, 64)):
        for spin, arith in ((0.9, 0), (0.0, 0), (0.9, 2)):
            prm = rrt.RenderParams(spin=spin, arith_mode=arith, max_steps=n)
            _, hdr = render_pano(rrt, tex, PW, PH, 1, proj, T, cam, all_fx(rrt), prm)
            D, inside = pr.d_vector(po, proj.kind, proj.fov_deg, proj.vfov_deg, PW, PH, *np.meshgrid(np.arange(PW), np.arange(PH)),
                                    cam.as_array())
            cand = np.argwhere(inside & np.all(D != 0, axis=-1))
            pick = cand[rng.choice(len(cand), 128, replace=False)]
            want = _probe_hdr(rrt, tex, T, cam.as_array()[0], cam, [D[y, x] for y, x in pick], all_fx(rrt, False), prm)
            got = np.stack([hdr[PH - 1 - y, x, :3] for y, x in pick])
            bad = ~_probe_matches(got, want)
            assert not bad.any(), (proj.info(), view, n, spin, arith, int(bad.sum()), pick[bad][:4].tolist())


@gpu
@pytest.mark.parametrize("view,n", SAMPLED)
def test_stereo_frames_honour_the_budget(ctx, po, view, n):
    """launch_raymarch_stereo at the budget: 128 random pixels per eye march the pinned pinhole path at the same budget (the check
    of test_gpu_stereo.py::test_every_pixel_marches_the_pinned_pinhole_path), and base 0 gives the mono frame in each half"""
    import projection_ref as pr
    import stereo_ref as sr
    from sampled_util import all_fx_stereo as all_fx, probe_hdr_stereo as _probe_hdr, render_mono, render_stereo, stereo_layout as _layout
    g, rrt, tex = ctx
    rng = np.random.default_rng(n)
    cam = camera(view)
    views = [(rrt.Projection("equirect"), rrt.Stereo("top-bottom", 1.5, 0.0, (45.0, 80.0)), 96, 48),
             (rrt.Projection("pinhole"), rrt.Stereo("side-by-side", 0.8, 12.0), 64, 36)]
    for proj, st, SW, SH in views:
        for spin, arith in ((0.9, 0), (0.9, 2)):
            prm = rrt.RenderParams(spin=spin, arith_mode=arith, max_steps=n)
            fx = all_fx(rrt, proj.kind == pr.EQUIRECT)
            _, hdr = render_stereo(rrt, tex, SW, SH, 1, proj, st, T, cam, fx, prm)
            for eye in (sr.LEFT, sr.RIGHT):
                o, D = sr.ray(po, proj.kind, proj.fov_deg, proj.vfov_deg, st.base, st.convergence,
                              (st.pole_merge_from_deg, st.pole_merge_to_deg), SW, SH, eye, cam.as_array())
                cand = np.argwhere(np.all(D != 0, axis=-1))
                pick = cand[rng.choice(len(cand), 128, replace=False)]
                want = _probe_hdr(rrt, tex, T, cam, [(o[y, x], D[y, x]) for y, x in pick], all_fx(rrt, False), prm)
                half = sr.eye_half(_layout(st), hdr, eye, SW, SH)
                got = np.stack([half[SH - 1 - y, x, :3] for y, x in pick])
                bad = ~_probe_matches(got, want)
                assert not bad.any(), (proj.info(), st.info(), eye, view, n, arith, int(bad.sum()), pick[bad][:4].tolist())
            # base 0: each half is the mono frame at the same budget
            st0 = rrt.Stereo(st.name, 0.0, 9.0, (30.0, 60.0))
            for s in (1, 2):
                ref8, ref = render_mono(rrt, tex, SW, SH, s, proj, T, cam, all_fx(rrt), prm)
                got8, got = render_stereo(rrt, tex, SW, SH, s, proj, st0, T, cam, all_fx(rrt), prm)
                for eye in (sr.LEFT, sr.RIGHT):
                    g8, gh = sr.eye_half(_layout(st0), got8, eye, SW, SH), sr.eye_half(_layout(st0), got, eye, SW, SH)
                    assert np.array_equal(g8, ref8) and same_bits(gh, ref), (proj.info(), view, n, arith, s, eye)


def _libm_account(r, o):
    """the figures of test_gpu_frames.py::test_tolerance_modes_against_the_libm_oracle for a debug render against a libm frame"""
    du8 = np.abs(r["rgba8"].astype(int) - o["rgba8"].astype(int))
    ref, got = o["ldr"][..., :3], r["ldr"][..., :3]
    with np.errstate(invalid="ignore"):
        bad = (np.abs(got - ref) > 1e-4 * np.abs(ref) + 1e-5).any(axis=2)
    return {"pixels_outside_1e-4": int(bad.sum()), "bytes_off_by_more_than_1": int((du8 > 1).sum()), "bytes_differing": int((du8 > 0).sum()),
            "steps_off": int((r["steps"] != o["steps"]).sum())}


def _within_bars(f):
    return f["pixels_outside_1e-4"] <= 2 and f["bytes_off_by_more_than_1"] <= 2 and f["bytes_differing"] <= 12 and f["steps_off"] <= 3


@gpu
@pytest.mark.parametrize("mode", [2, 1], ids=["fmad", "fast"])
def test_tolerance_modes_at_every_budget(ctx, po, sky, mode):
    """FMAD / FAST debug launches at every (view, spin, budget): no ray takes more than the budget's steps, a ray that fell in
    carries transmittance 0, the production launch gives the debug launch's bytes; and against the libm oracle AT THE SAME BUDGET
    the frame is inside the bars of test_tolerance_modes_against_the_libm_oracle (RGB within 1e-4 relative + 1e-5 absolute on all
    but 2 pixels, at most 2 bytes off by more than 1 LSB, at most 12 bytes differing, at most 3 step counts off).  A case where the
    STRICT path, run against the same libm frame, is outside the bars too measures the oracle's math-library sensitivity, not the
    mode: it leaves this comparison (and only this one) and is printed; at most one case in ten may."""
    g, rrt, tex = ctx
    dropped = []
    for view, spin, n in CASES:
        cam = camera(view)
        r = g.render_gpu(W, H, spin, 1, cam, T, tex, fx=fx_of(rrt), max_steps=n, arith_mode=mode)
        assert (r["steps"] >= 0).all() and (r["steps"] <= n).all(), (view, spin, n, int(r["steps"].max()))
        assert (r["rad"][r["hit"] == 1, 3] == 0.0).all(), (view, spin, n)
        prod = g.render_gpu(W, H, spin, 1, cam, T, tex, fx=fx_of(rrt), max_steps=n, arith_mode=mode, debug=False)
        assert np.array_equal(prod["rgba8"], r["rgba8"]), (view, spin, n)
        o = oracle(po, sky, view, spin, n, libm=True)
        f = _libm_account(r, o)
        if not _within_bars(f):
            fs = _libm_account(g.render_gpu(W, H, spin, 1, cam, T, tex, fx=fx_of(rrt), max_steps=n), o)
            print("outside the bars:", (view, spin, n), "mode", f, "strict", fs)
            assert not _within_bars(fs), ((view, spin, n), mode, f, "strict is inside", fs)
            dropped.append((view, spin, n))
    print("left to the oracle's math-library sensitivity:", dropped)
    assert len(dropped) <= len(CASES) // 10, dropped
