"""RRT_ARITH_FMAD's definition -- the oracle's FMAD mode (oracle/rrt_oracle.c: geodesic_acc_fmad / integrate_rk4_fmad, the fused
loop-top radius and escape test) -- examined on the CPU, before any GPU frame is held to it:

  1. it is not strict: the fused step's bits differ from the strict step's on a measurable share of single steps and on most
     100-step chains, so a GPU test that asserts equality with it cannot pass by running strict arithmetic;
  2. it is the mathematics: against a binary64 RK4 of the same equations the fused chain is as accurate as the strict
     restatement of the reference (rms error ratio <= 1.05; measured 0.99-1.01);
  3. it is the class the documents say: on the twelve scenes of tests/golden/frames_ref_fma.npz its frames deviate from the
     strictly compiled reference no more than the reference's own kernel compiled by a contracting compiler does -- the rule
     tests/test_gpu_tolerance.py::test_fmad_deviates_less_than_a_contracted_reference applies to the GPU frame.

The yardstick is the strict restatement of the reference and binary64 throughout, never the GPU."""
import numpy as np
import pytest

import march_ref as mr

F = np.float32
H_NEAR, H_DISK, H_VAC = mr.STEP * F(0.1), mr.STEP * F(0.3), mr.STEP       # the zone rule's three step sizes (raymarcher.cu:54-62)
SPINS = (0.9, 0.0)


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _zone_rays(rng, zone, n):
    """random rays of one zone of the march: near the hole (2.1 <= r < 18), in the disk zone (18 <= r < 30, |y| < 4), in the
    vacuum (30 <= r <= 250); unit velocities in random directions"""
    d = _unit(rng, n)
    if zone == "near":
        p = d * rng.uniform(2.1, 18.0, (n, 1))
    elif zone == "disk":
        phi = rng.uniform(0, 2 * np.pi, n)
        rc = rng.uniform(18.0, 29.5, n)
        y = rng.uniform(-3.9, 3.9, n)
        p = np.stack([rc * np.cos(phi), y, rc * np.sin(phi)], axis=1)
        p *= np.minimum(1.0, 29.9 / np.linalg.norm(p, axis=1))[:, None]
    else:
        p = d * rng.uniform(30.0, 250.0, (n, 1))
    return p.astype(F), _unit(rng, n).astype(F)


def _tangential(rng, n, r_lo, r_hi):
    """rays at r in [r_lo, r_hi] with unit velocities at right angles to the radius"""
    d = _unit(rng, n)
    t = np.cross(d, _unit(rng, n))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    return (d * rng.uniform(r_lo, r_hi, (n, 1))).astype(F), t.astype(F)


def _chain(units, p, v, h, spin, n_steps, arith):
    hs = np.full(len(p), h, F)
    for _ in range(n_steps):
        p, v = units.rk4_arith(p, v, hs, spin, arith)
    return p, v


# ---- the same equations in binary64 (geodesics.h:30-45, integrators.h:23-59), nothing else shared with the oracle ----
def _acc64(p, v, spin):
    r2 = (p * p).sum(axis=1)
    r = np.sqrt(r2)
    L = np.cross(p, v)
    L2 = (L * L).sum(axis=1)
    radial = (-1.5 * 2.0 * L2 / (r2 * r2 * r))[:, None] * p
    ds = (2.0 * spin * 2.0) / (r2 * r)
    drag = np.stack([p[:, 2], np.zeros(len(p)), -p[:, 0]], axis=1) * ds[:, None]
    return np.where((r < 1.0)[:, None], 0.0, radial + drag)


def _chain64(p, v, h, spin, n_steps):
    p, v, h, spin = p.astype(np.float64), v.astype(np.float64), float(h), float(F(spin))
    for _ in range(n_steps):
        kv1 = _acc64(p, v, spin); kp1 = v
        v2 = v + kv1 * (h * 0.5); p2 = p + kp1 * (h * 0.5)
        kv2 = _acc64(p2, v2, spin); kp2 = v2
        v3 = v + kv2 * (h * 0.5); p3 = p + kp2 * (h * 0.5)
        kv3 = _acc64(p3, v3, spin); kp3 = v3
        v4 = v + kv3 * h; p4 = p + kp3 * h
        kv4 = _acc64(p4, v4, spin); kp4 = v4
        v = v + (kv1 + 2.0 * kv2 + 2.0 * kv3 + kv4) * (h / 6.0)
        p = p + (kp1 + 2.0 * kp2 + 2.0 * kp3 + kp4) * (h / 6.0)
    return p, v


def _rms(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b) ** 2).sum(axis=1).mean()))


def test_the_fmad_entry_points_are_the_strict_ones_in_strict_mode_and_refuse_fast(po):
    rng = np.random.default_rng(1)
    units = po.units()
    p, v = _zone_rays(rng, "near", 4096)
    h = np.full(len(p), H_NEAR, F)
    for spin in SPINS:
        assert np.array_equal(_bits(units.geodesic_acc_arith(p, v, spin, mr.STRICT)), _bits(units.geodesic_acc(p, v, spin)))
        a, b = units.rk4_arith(p, v, h, spin, mr.STRICT), units.rk4(p, v, h, spin)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(units.dot_arith(p, v, mr.STRICT)), _bits((p[:, 0] * v[:, 0] + p[:, 1] * v[:, 1]) + p[:, 2] * v[:, 2]))
    # each fused term is rounded once: fmaf redone in exact rational arithmetic (nearest float of a*b + c, ties to even)
    from fractions import Fraction

    def fma_exact(a, b, c):
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        near = F(float(a) * float(b) + float(c))                   # within an ulp of the answer
        cands = (near, np.nextafter(near, F(-np.inf)), np.nextafter(near, F(np.inf)))
        return min(cands, key=lambda t: (abs(Fraction(float(t)) - exact), int(_bits(t)[0]) & 1))

    fused = units.dot_arith(p[:512], v[:512], mr.FMAD)
    assert (fused != units.dot_arith(p[:512], v[:512], mr.STRICT)).any()
    for (px, py, pz), (vx, vy, vz), got in zip(p[:512], v[:512], fused):
        assert _bits(got) == _bits(fma_exact(pz, vz, fma_exact(py, vy, F(px * vx)))), (px, py, pz, vx, vy, vz, got)
    for call in (lambda: units.rk4_arith(p, v, h, 0.9, 1), lambda: units.geodesic_acc_arith(p, v, 0.9, 1), lambda: units.dot_arith(p, p, 3),
                 lambda: units.rk4_arith(p, v, h, 0.9, -1)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("spin", SPINS)
def test_fmad_is_not_strict(po, spin):
    """conditions on the inputs of every FMAD equality test: single steps of 20 000 random rays per zone differ from the strict
    step in some bit on >= 0.5 % of the rays (the tree alone: 1.7 % or more), 100-step vacuum chains on >= 30 % (53 % or more)"""
    rng = np.random.default_rng(20261019)
    units = po.units()
    for zone, h in (("near", H_NEAR), ("disk", H_DISK), ("vacuum", H_VAC)):
        p, v = _zone_rays(rng, zone, 20000)
        hs = np.full(len(p), h, F)
        ps, vs = units.rk4(p, v, hs, spin)
        pf, vf = units.rk4_arith(p, v, hs, spin, mr.FMAD)
        differ = ((_bits(ps) != _bits(pf)) | (_bits(vs) != _bits(vf))).any(axis=1).mean()
        print(f"single {zone} steps, a = {spin:g}: {100 * differ:.2f} % differ from the strict step")
        assert differ >= 0.005, (zone, spin, differ)
    p, v = _tangential(rng, 4096, 60.0, 200.0)
    ps, vs = _chain(units, p, v, H_VAC, spin, 100, mr.STRICT)
    pf, vf = _chain(units, p, v, H_VAC, spin, 100, mr.FMAD)
    differ = ((_bits(ps) != _bits(pf)) | (_bits(vs) != _bits(vf))).any(axis=1).mean()
    print(f"100 vacuum steps, a = {spin:g}: {100 * differ:.1f} % of the rays differ from the strict chain")
    assert differ >= 0.30, (spin, differ)


# (label, r range, step size, steps, rays): the near-hole rays have an impact parameter >= 6 > sqrt(27), the critical one: well
# conditioned.  16384 of them: at 50 steps a larger set than the vacuum one costs nothing and narrows the ratio's own scatter.
CHAINS = (("vacuum", 60.0, 200.0, H_VAC, 100, 4096), ("near hole", 6.0, 18.0, H_NEAR, 50, 16384))


@pytest.mark.parametrize("spin", SPINS)
@pytest.mark.parametrize("chain", CHAINS, ids=[c[0].replace(" ", "_") for c in CHAINS])
def test_fmad_is_as_accurate_as_the_strict_restatement(po, chain, spin):
    """chains of RK4 steps against binary64: rms error of the FMAD chain <= 1.05 x the strict chain's, positions and velocities"""
    label, r_lo, r_hi, h, n_steps, n = chain
    units = po.units()
    for seed in (11, 12, 13):
        p, v = _tangential(np.random.default_rng(seed), n, r_lo, r_hi)
        p64, v64 = _chain64(p, v, h, spin, n_steps)
        ps, vs = _chain(units, p, v, h, spin, n_steps, mr.STRICT)
        pf, vf = _chain(units, p, v, h, spin, n_steps, mr.FMAD)
        ep, ev = _rms(pf, p64) / _rms(ps, p64), _rms(vf, v64) / _rms(vs, v64)
        print(f"{label}, a = {spin:g}, seed {seed}: rms error FMAD / strict = {ep:.4f} (position), {ev:.4f} (velocity); "
              f"strict rms position error {_rms(ps, p64):.3e}")
        assert _rms(ps, p64) > 0 and _rms(vs, v64) > 0
        assert ep <= 1.05 and ev <= 1.05, (label, spin, seed, ep, ev)


def test_fmad_oracle_deviates_less_than_a_contracted_reference(po, sky, frames_ref, frames_ref_fma):
    """the rule of tests/test_gpu_tolerance.py::test_fmad_deviates_less_than_a_contracted_reference, applied to the DEFINITION
    on a machine without a GPU: the oracle's FMAD frame in libm mode against the strictly compiled reference frame, beside the
    reference's own kernel under a contracting compiler (tests/golden/frames_ref_fma.npz), twelve scenes"""
    from conftest import contraction_counts
    names = ("G1", "G2", "G3", "G4", "G5", "K1", "K2", "R1", "B1", "B2", "B3", "B4")
    keys = ("steps_differ", "off_by_more_than_1", "deviant")
    tot = {k: dict.fromkeys(keys, 0) for k in ("contracted", "fmad")}
    differs_from_strict = 0
    for name in names:
        src = frames_ref_fma if name.startswith("B") else frames_ref
        w, h, spin, vol, t = frames_ref_fma[f"{name}_scene"]
        w, h, spin, vol, t = int(w), int(h), float(F(spin)), int(vol), float(F(t))
        fl, fv = frames_ref_fma[f"{name}_fx_flags"], frames_ref_fma[f"{name}_fx_vals"]
        fx = po.default_effects(use_bloom=int(fl[0]), use_vignette=int(fl[1]), use_ca=int(fl[2]), use_lens=int(fl[3]),
                                bloom_threshold=float(fv[0]), bloom_intensity=float(fv[1]), vignette_intensity=float(fv[2]),
                                ca_amount=float(fv[3]), distortion_amount=float(fv[4]))
        a = frames_ref_fma[f"{name}_camera"]
        s8, ss = src[f"{name}_rgba8"], src[f"{name}_steps"]
        con, _ = contraction_counts(s8, ss, frames_ref_fma[f"{name}_fma_rgba8"], frames_ref_fma[f"{name}_fma_steps"])
        rows = {"contracted": con}
        for tag, arith in (("fmad", po.ARITH_FMAD), ("strict", po.ARITH_STRICT)):
            o = po.render(po.camera(a[0], a[1], a[2], a[3]), fx,
                          po.default_params(spin=spin, volumetrics=vol, math_mode=po.MATH_LIBM, arith_mode=arith), t, w, h, sky,
                          want=("rgba8", "diag"))
            rows[tag], _ = contraction_counts(s8, ss, o["rgba8"], o["steps"])
        print(f"{name} {w}x{h} a={spin:g} vol={vol}: " + " | ".join(
            f"{k}: steps {r['steps_differ']}, >1 LSB {r['off_by_more_than_1']}, deviant {r['deviant']}, any byte {r['bytes_differ']}"
            for k, r in rows.items()))
        assert rows["strict"]["bytes_differ"] == 0 and rows["strict"]["steps_differ"] == 0      # the strict restatement is the reference
        differs_from_strict += rows["fmad"]["bytes_differ"] + rows["fmad"]["steps_differ"]
        for q in keys:
            tot["contracted"][q] += rows["contracted"][q]
            tot["fmad"][q] += rows["fmad"][q]
            assert rows["fmad"][q] <= rows["contracted"][q] + 3, (name, q, rows)
    print("total:", tot)
    for q in keys:
        assert tot["fmad"][q] <= tot["contracted"][q], (q, tot)
    assert differs_from_strict > 0                         # an FMAD mode that rendered strict frames would pass the rule emptily
