"""A numpy float32 restatement of the HDR glow (include/rrt.h: rrt_launch_glow, steps 1-4) for the tests.  Every operation is one
float32 operation in the contract's order; the taps come from the library (rrt_glow_weights).  Frames are (h, w, 4) arrays in the
stored layout: axis 0 the stored (bottom-up) row, axis 1 the column."""
import numpy as np

F = np.float32


def bright_pass(hdr, threshold):
    """step 1: the soft-knee bright pass of the rgb of (h, w, >=3) float32, as three (h, w) planes"""
    r, g, b = (np.ascontiguousarray(hdr[..., c], dtype=F) for c in range(3))
    t = F(threshold)
    luma = (r * F(0.2126) + g * F(0.7152)) + b * F(0.0722)
    on = luma > t
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(on, (luma - t) / luma, F(0)).astype(F)
    z = F(0)
    return [np.where(on, c * f, z).astype(F) for c in (r, g, b)]


def blur_axis(x, taps, axis):
    """step 3 along one axis: acc = 0, then acc = acc + w[k + R] * x[clamp(i + k)] for k = -R ... R ascending"""
    taps = np.asarray(taps, F)
    r = (taps.size - 1) // 2
    n = x.shape[axis]
    idx = np.arange(n)
    acc = np.zeros_like(x, dtype=F)
    for k in range(-r, r + 1):
        src = np.take(x, np.clip(idx + k, 0, n - 1), axis=axis)
        acc = acc + taps[k + r] * src
    assert acc.dtype == F
    return acc


def glow_hdr(hdr, taps, threshold, intensity):
    """steps 1-4 up to the tone map: out = H + G * s, (h, w, 3) float32.  taps: one array per lobe (rrt_glow_weights)"""
    hdr = np.asarray(hdr, F)
    b = bright_pass(hdr, threshold)
    g = None
    for t in taps:
        v = [blur_axis(blur_axis(c, t, 1), t, 0) for c in b]
        g = v if g is None else [gc + vc for gc, vc in zip(g, v)]
    s = F(intensity) / F(len(taps))
    out = np.stack([hdr[..., c] + g[c] * s for c in range(3)], axis=-1)
    assert out.dtype == F
    return out


def lobe_taps(rrt, glow, height):
    return [rrt.glow_weights(glow, height, l) for l in range(glow.lobes)]
