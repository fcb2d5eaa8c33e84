"""A numpy restatement of exposure control (include/rrt.h: rrt_launch_exposure, steps 1-6) for the tests: uint32 bit operations for
the bins, float64 and float32 where the contract says so, one operation per step in the contract's order.  The resolve removes the
cut counts bin by bin, literally as the contract words it (the library intersects rank intervals instead).  Frames are (h, w, 4)
float32 arrays; `po` is the CPU oracle binding, whose portable exp is the library's rrt_expf."""
import math

import numpy as np

F = np.float32
BINS = 256
LN2 = F(0.693147182)


def luma(hdr):
    """step 1: the glow's luma of (..., >=3) float32, in its association"""
    r, g, b = (np.ascontiguousarray(hdr[..., c], dtype=F) for c in range(3))
    with np.errstate(all="ignore"):
        y = (r * F(0.2126) + g * F(0.7152)) + b * F(0.0722)
    assert y.dtype == F
    return y


def bin_of(y):
    """step 1: (metered, bin) of float32 lumas"""
    u = np.ascontiguousarray(y, F).view(np.uint32)
    metered = (u > np.uint32(0)) & (u < np.uint32(0x7F800000))
    b = np.clip((u >> np.uint32(20)).astype(np.int64) - 888, 0, BINS - 1)
    return metered, b


def histogram(hdr):
    """c_b of a frame: uint32[256]"""
    metered, b = bin_of(luma(hdr))
    return np.bincount(b[metered].ravel(), minlength=BINS).astype(np.uint32)


def bin_centres():
    """step 2: L_b in float64, from numpy's log2"""
    b = np.arange(BINS, dtype=np.int64) + 888
    e, j = b >> 3, b & 7
    return (e - 127).astype(np.float64) + np.log2(1.0 + (j.astype(np.float64) + 0.5) / 8.0)


def clamp(x, lo, hi):
    x, lo, hi = F(x), F(lo), F(hi)
    return lo if x < lo else (hi if x > hi else x)


def resolve(hist, table, s):
    """step 3: (N, m, target) of a histogram; m and target are None when nothing was metered.  s: an ExposureSettings (or anything
    with its fields); table: the library's L_b (rrt_exposure_bin_ev)"""
    r = [int(c) for c in hist]
    n = sum(r)
    if n == 0:
        return 0, None, None
    lo, hi = n * int(s.low_permille) // 1000, n * int(s.high_permille) // 1000
    for b in range(BINS):                       # lo counts from the lowest bins upwards
        take = min(r[b], lo)
        r[b] -= take
        lo -= take
    for b in range(BINS - 1, -1, -1):           # hi counts from the highest bins downwards
        take = min(r[b], hi)
        r[b] -= take
        hi -= take
    assert lo == 0 and hi == 0
    kept = sum(r)
    assert kept >= 1
    acc = 0.0                                   # Python floats: binary64, one rounding per operation
    for b in range(BINS):
        acc = acc + float(r[b]) * float(table[b])
    m = acc / float(kept)
    log2_key = math.log2(float(F(s.key)))       # the host's log2, in double
    target = clamp(F(log2_key - m) + F(s.ev), s.min_ev, s.max_ev)
    return n, m, target


class State:
    """step 4: the state a reset leaves, advanced by step()"""

    def __init__(self):
        self.ev, self.frames = F(0.0), 0

    def step(self, hist, table, s):
        n, m, target = resolve(hist, table, s)
        if n == 0:
            if self.frames == 0:
                self.ev = clamp(s.ev, s.min_ev, s.max_ev)
        elif self.frames == 0:
            self.ev = target
        else:
            alpha = F(s.adapt_up) if target > self.ev else F(s.adapt_down)
            self.ev = F(self.ev + F(F(target - self.ev) * alpha))
        self.frames += 1
        assert type(self.ev) is F
        return n, m, target


def scale_of(po, ev):
    """step 5: rrt_expf(ev * 0.693147182f)"""
    return F(po.math_fn(0, po.MATH_PORTABLE, np.array([F(ev) * LN2], F))[0])


def apply(hdr, scale):
    """step 6 up to the tone map: rgb * scale, alpha kept"""
    out = np.array(hdr, F, copy=True)
    with np.errstate(all="ignore"):
        out[..., :3] = out[..., :3] * F(scale)
    return out


def tone_map(po, rgb):
    """(uint8)(int)((1 - exp(-x * 0.8f)) * 255) with the portable exp (raymarcher.cu:164-173), alpha 255"""
    x = (-np.asarray(rgb, F)) * F(0.8)
    e = po.math_fn(0, po.MATH_PORTABLE, x.ravel()).reshape(x.shape)
    v = (F(1.0) - e) * F(255.0)
    out = (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)
    return np.concatenate([out, np.full(out.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def library_table(rrt):
    return np.array([rrt.exposure_bin_ev(b) for b in range(BINS)], np.float64)


def expose(po, rrt, hdr, s, state=None, table=None):
    """one launch: (hist or None, scale, scaled hdr, rgba8); auto mode advances `state`"""
    if s.mode == 0:
        hist, scale = None, scale_of(po, s.ev)
    else:
        hist = histogram(hdr)
        state.step(hist, table if table is not None else library_table(rrt), s)
        scale = scale_of(po, state.ev)
    out = apply(hdr, scale)
    return hist, scale, out, tone_map(po, out[..., :3])
