"""tests/march_ref.py::march_ref, the array form of the march loop that rrt_unit_march is compared with on the GPU, proven
against the oracle's own frames on the CPU: start from the primary rays of a frame (the oracle at max_steps = 0), march N steps,
and require the bits of the oracle's render at budget N with volumetrics off -- position, velocity, step count and hit flag of
every ray.  Both arithmetics: the strict march against the strict oracle, the FMAD march (march_ref.FMAD) against the oracle's
FMAD mode (Params.arith_mode), on the same views, spins and budgets."""
import numpy as np
import pytest

import march_ref as mr

W, H = 61, 37


def _camera(pos, yaw, pitch):
    from relativisticraytracer_amd import CameraState
    return CameraState.from_angles(pos, yaw, pitch).as_array()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_every_budget(po, sky, view, spin, arith):
    cam = _camera(*mr.VIEWS[view])
    p0, v0 = mr.primary_rays(po, cam, W, H, sky, spin=spin)
    assert np.array_equal(p0, np.broadcast_to(cam[0], p0.shape))
    ocam = po.camera(cam[0], cam[1], cam[2], cam[3])
    seen = set()
    for n in mr.BUDGETS:
        o = po.render(ocam, po.default_effects(), po.default_params(spin=spin, volumetrics=0, max_steps=n, arith_mode=arith), 0.0, W, H, sky,
                      want=("diag",))
        p, v, steps, hit = mr.march_ref(p0, v0, spin, n, po=po, arith=arith)
        assert np.array_equal(steps, o["steps"]), (view, spin, n, int((steps != o["steps"]).sum()))
        assert np.array_equal(hit, o["hit"]), (view, spin, n)
        assert np.array_equal(_bits(p), _bits(o["pos"])), (view, spin, n)
        assert np.array_equal(_bits(v), _bits(o["vel"])), (view, spin, n)
        out_of_steps = (steps == n) & (hit == 0)
        seen |= {k for k, m in (("hit", hit == 1), ("out", out_of_steps), ("escaped", (hit == 0) & ~out_of_steps)) if m.any()}
    # the budgets meet every exit of the loop this view has (inside the horizon: one; from far away no ray falls in)
    assert seen == {"inside_horizon": {"hit"}, "far": {"out", "escaped"}}.get(view, {"hit", "out", "escaped"}), (view, seen)


@pytest.mark.parametrize("spin", mr.SPINS)
@pytest.mark.parametrize("view", list(mr.VIEWS))
def test_march_ref_reproduces_the_oracle_at_every_budget(po, sky, view, spin):
    _check_every_budget(po, sky, view, spin, mr.STRICT)


@pytest.mark.parametrize("spin", mr.SPINS)
@pytest.mark.parametrize("view", list(mr.VIEWS))
def test_fmad_march_ref_reproduces_the_fmad_oracle_at_every_budget(po, sky, view, spin):
    _check_every_budget(po, sky, view, spin, mr.FMAD)


def test_fmad_march_ref_is_not_the_strict_one(po, sky):
    """the FMAD half above cannot pass by running strict twice: after 150 steps most rays of the default view differ"""
    cam = _camera(*mr.VIEWS["default"])
    p0, v0 = mr.primary_rays(po, cam, W, H, sky, spin=0.9)
    ps = mr.march_ref(p0, v0, 0.9, 150, po=po)[0]
    pf = mr.march_ref(p0, v0, 0.9, 150, po=po, arith=mr.FMAD)[0]
    assert (_bits(ps) != _bits(pf)).any(axis=1).mean() > 0.3
    with pytest.raises(ValueError):
        mr.march_ref(p0[:4], v0[:4], 0.9, 2, po=po, arith=1)          # FAST has no restatement
    with pytest.raises(ValueError):
        po.render(po.camera(cam[0], cam[1], cam[2], cam[3]), po.default_effects(), po.default_params(arith_mode=1), 0.0, 4, 4, sky)


def test_march_ref_first_step_and_empty_input(po):
    """a ray started at step k takes the steps a ray started at 0 takes from k on, and counts from k; no rays is no work"""
    rng = np.random.default_rng(5)
    p0 = rng.normal(size=(32, 3)).astype(np.float32) * np.float32(40.0)
    v0 = rng.normal(size=(32, 3)).astype(np.float32)
    v0 /= np.linalg.norm(v0, axis=1, keepdims=True).astype(np.float32)
    k0 = (np.arange(32) % 8).astype(np.int32)
    p, v, steps, hit = mr.march_ref(p0, v0, 0.9, 40, first_step=k0, po=po)
    for k in range(8):
        sel = k0 == k
        pk, vk, sk, hk = mr.march_ref(p0[sel], v0[sel], 0.9, 40 - k, po=po)
        assert np.array_equal(_bits(p[sel]), _bits(pk)) and np.array_equal(_bits(v[sel]), _bits(vk))
        assert np.array_equal(steps[sel], sk + k) and np.array_equal(hit[sel], hk)
    late = mr.march_ref(p0, v0, 0.9, 3, first_step=np.full(32, 5, np.int32), po=po)
    assert np.array_equal(late[2], np.full(32, 5)) and np.array_equal(_bits(late[0]), _bits(p0))
    e = mr.march_ref(np.zeros((0, 3)), np.zeros((0, 3)), 0.0, 10, po=po)
    assert e[0].shape == (0, 3) and e[2].shape == (0,)
