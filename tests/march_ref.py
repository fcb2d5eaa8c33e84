"""The march loop on arrays of rays, restated in numpy from the reference's loop (raymarcher.cu:41-121, no media): what
rrt_unit_march (include/rrt_test.h) -- the production march_inline / vacuum_run on rays a test chose -- is compared with.

Per step, in float32 throughout: the radius sqrt((x*x + y*y) + z*z) of the pre-step position; the horizon test
r < 2.0f * 1.01f (the ray ends, `hit`, the step is not counted); the zone rule of raymarcher.cu:56-62 for the step size; one
RK4 step of the oracle (rrto_rk4, pinned to the reference's integrate_rk4 by tests/test_oracle_units.py); the escape test on the
pre-step position and the post-step velocity (r > 250 and dot > 0: the ray ends, the step is counted).  A ray that does neither
ends with steps = max_steps.  tests/test_march_ref.py proves the restatement against the oracle's own frames, bit for bit.

arith = FMAD is RRT_ARITH_FMAD's march: the squared radius and the escape test's dot product are the fused
fma(z, z', fma(y, y', x*x')) (rrto_dot_arith: C's exact fmaf), the step is the oracle's FMAD step (rrto_rk4_arith); the loop is
the same, and the same proof holds it to the oracle's FMAD frames.

VIEWS / SPINS / BUDGETS are the cases of that proof; the GPU modules draw their rays from the same views."""
import numpy as np

F = np.float32

HORIZON = F(2.0) * F(1.01)                     # EVENT_HORIZON * 1.01f
STEP = F(0.3)                                  # STEP_SIZE_M
DISK_H5, DISK_R = F(0.8) * F(5.0), F(25.0) + F(5.0)      # DISK_H_M * 5.0f, DISK_OUT_M + 5.0f
CLOUD_H15, CLOUD_R = F(0.5) * F(1.5), F(25.0)            # CLOUD_H_M * 1.5f, CLOUD_OUT_M
STRICT, FMAD = 0, 2                            # RRT_ARITH_STRICT, RRT_ARITH_FMAD; FAST has no restatement
VACUUM_R = F(30.0)                             # beyond it no zone and no horizon: the wave-uniform vacuum step's domain

# (position, yaw, pitch) for CameraState.from_angles
VIEWS = {
    "default": ((0.0, 10.0, -60.0), 0.0, -10.0),          # the reference's start-up camera
    "skimmer": ((35.0, 0.8, 10.0), -106.0, -1.2),         # grazes the disk plane
    "in_disk": ((14.0, 0.05, 3.0), 200.0, 2.0),           # inside the disk, in both media zones from step 0
    "far": ((0.0, 40.0, -300.0), 0.0, -5.0),              # hundreds of vacuum steps before anything else
    "inside_horizon": ((0.0, 1.5, -1.0), 10.0, -30.0),    # every ray ends at step 0
}
SPINS = (0.9, 0.0)
BUDGETS = (1, 2, 7, 150, 1000, 2000)


def primary_rays(po, cam_array, w, h, sky, **prm):
    """every pixel's primary ray (pos, vel), each (w*h, 3), rows top-down: the oracle's frame at max_steps = 0"""
    a = cam_array
    o = po.render(po.camera(a[0], a[1], a[2], a[3]), po.default_effects(), po.default_params(max_steps=0, **prm), 0.0, w, h, sky,
                  want=("diag",))
    return o["pos"].copy(), o["vel"].copy()


def radius(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.sqrt((x * x + y * y) + z * z)


def radius_arith(units, p, arith):
    """the march's loop-top radius in arithmetic `arith`: the correctly rounded root of the (strict or fused) squared radius"""
    if arith == STRICT:
        return radius(p)
    return np.sqrt(units.dot_arith(p, p, arith))


def march_ref(p, v, spin, max_steps, first_step=None, po=None, arith=STRICT):
    """march rays (p, v) (n, 3) until step max_steps; ray i starts at step first_step[i] (default 0).  po: the oracle binding
    (the `po` fixture; imported here when None).  arith: STRICT or FMAD.
    Returns (p, v, steps, hit): final state, the ray's step count, whether the horizon test ended it."""
    if po is None:
        from oracle import pyoracle as po
    p = np.array(p, F).reshape(-1, 3)
    v = np.array(v, F).reshape(-1, 3)
    n = len(p)
    k0 = np.zeros(n, np.int32) if first_step is None else np.asarray(first_step, np.int32)
    steps = np.maximum(k0, np.int32(max_steps)).astype(np.int32)          # a ray that runs out of steps
    hit = np.zeros(n, np.int32)
    alive = np.ones(n, bool)
    units = po.units()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(int(k0.min()) if n else 0, int(max_steps)):
            idx = np.flatnonzero(alive & (k0 <= k))
            if len(idx) == 0:
                if not alive.any():
                    break
                continue
            q = p[idx]
            r = radius_arith(units, q, arith)
            assert r.dtype == F
            fell = r < HORIZON
            hit[idx[fell]] = 1
            steps[idx[fell]] = k
            alive[idx[fell]] = False
            idx, q, r = idx[~fell], q[~fell], r[~fell]
            if len(idx) == 0:
                continue
            near = r < F(18.0)
            in_disk = (np.abs(q[:, 1]) < DISK_H5) & (r < DISK_R)
            in_cloud = (np.abs(q[:, 1]) < CLOUD_H15) & (r < CLOUD_R)
            hstep = np.where(near, STEP * F(0.1), np.where(in_disk, STEP * F(0.3), np.where(in_cloud, STEP * F(0.5), STEP))).astype(F)
            pn, vn = units.rk4(q, v[idx], hstep, spin) if arith == STRICT else units.rk4_arith(q, v[idx], hstep, spin, arith)
            p[idx], v[idx] = pn, vn
            d = (q[:, 0] * vn[:, 0] + q[:, 1] * vn[:, 1]) + q[:, 2] * vn[:, 2] if arith == STRICT else units.dot_arith(q, vn, arith)
            out = (r > F(250.0)) & (d > 0)
            steps[idx[out]] = k + 1
            alive[idx[out]] = False
    return p, v, steps, hit
