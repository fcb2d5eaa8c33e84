"""A numpy float32 restatement of a depth-of-field sample's primary ray (include/rrt.h: rrt_launch_raymarch_dof) for the tests: the
origin and D (before normalisation) in the contract's order, every operation one float32 operation, and of rrt_lens_points' spiral
in double.  Pixel arrays are indexed [y, x] with y the virtual row as the kernel sees it (+y toward `up`)."""
import math

import numpy as np

import projection_ref as pr

F = np.float32


def shifts(lx, ly, focus):
    """(cx, cy) = (lx / focus, ly / focus), rounded on the host"""
    return F(F(lx) / F(focus)), F(F(ly) / F(focus))


def ray(W, H, cam, lx, ly, focus, x=None, y=None, lens=None):
    """(origin (3,), D (..., 3)) through the lens point (lx, ly) at integer pixel arrays x, y (default: the whole W x H frame,
    [y, x]); cam: (4, 3) pos, forward, right, up; lens: rrt_effects' distortion_amount or None"""
    if x is None:
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cam = np.asarray(cam, F)
    pos, fw, rt, up = cam
    lx, ly = F(lx), F(ly)
    cx, cy = shifts(lx, ly, focus)
    uvx, uvy = np.asarray(x).astype(F) / F(W), np.asarray(y).astype(F) / F(H)
    if lens is not None:                                       # rrt_device.h: lens_distort
        tx, ty = uvx - F(0.5), uvy - F(0.5)
        r2 = tx * tx + ty * ty
        g = F(1.0) + r2 * F(lens)
        uvx, uvy = tx * g + F(0.5), ty * g + F(0.5)
    u = uvx * F(2.0) - F(1.0)
    v = uvy * F(2.0) - F(1.0)
    u = u * (F(W) / F(H))
    if cx != 0:                                                # the zero rule: a zero of either sign changes nothing
        u = u - cx
    if cy != 0:
        v = v - cy
    u, v = np.broadcast_arrays(u, v)
    D = np.stack([fw[i] + (rt[i] * u + up[i] * v) for i in range(3)], axis=-1).astype(F)
    org = pos.copy()
    if lx != 0:
        org = (org + rt * lx).astype(F)
    if ly != 0:
        org = (org + up * ly).astype(F)
    return org, D


def rays(W, H, cam, lx, ly, focus):
    """(origin (3,), unit dir (H, W, 3)) of every pixel: what rrt_lens_ray returns"""
    o, D = ray(W, H, cam, lx, ly, focus)
    return o, pr.normalize(D)


def points(aperture, n, rotation=0.0):
    """rrt_lens_points: (n, 2) float32 -- (0, 0) for n = 1, else Vogel's spiral in double, rounded to float"""
    if n == 1:
        return np.zeros((1, 2), F)
    a, rot = float(F(aperture)), float(F(rotation))
    golden = 3.14159265358979323846 * (3.0 - math.sqrt(5.0))
    out = np.zeros((n, 2), F)
    for k in range(n):
        r = a * math.sqrt((k + 0.5) / n)
        th = rot + k * golden
        out[k] = (r * math.cos(th), r * math.sin(th))
    return out


def bit_reverse(m, n):
    """m's log2(n) bits reversed (n a power of two): the drivers' lens point of sample m"""
    r = 0
    while n > 1:
        r, m, n = (r << 1) | (m & 1), m >> 1, n >> 1
    return r
