"""A numpy float32 restatement of a stereo eye's primary ray (include/rrt.h: rrt_stereo) for the tests: the origin and D (before
normalisation) in the contract's order, built on projection_ref (the panorama's ray, sin and cos through the oracle's portable
rrt_sincosf).  Pixel arrays are eye-local, indexed [y, x] with y the virtual row as the kernel sees it (+y toward `up`)."""
import numpy as np

import projection_ref as pr

F = np.float32
TOP_BOTTOM, SIDE_BY_SIDE = 1, 2
LEFT, RIGHT = 0, 1


def half_base(base):
    """hb = (float)(0.5 * (double)base)"""
    return F(0.5 * float(F(base)))


def radians(deg):
    """(float)((double)deg * 3.14159265358979323846 / 180.0)"""
    return F(float(F(deg)) * 3.14159265358979323846 / 180.0)


def composite(layout, w, h):
    """(width, height) of the composite of two w x h eyes"""
    return (2 * w, h) if layout == SIDE_BY_SIDE else (w, 2 * h)


def eye_half(layout, frame, eye, w, h):
    """eye `eye`'s w x h half of a stored (bottom-up) composite array (rows, cols, ...): top-bottom keeps the right eye in stored
    rows 0 ... h-1, side-by-side the left eye in columns 0 ... w-1"""
    if layout == TOP_BOTTOM:
        return frame[:h] if eye == RIGHT else frame[h:2 * h]
    return frame[:, :w] if eye == LEFT else frame[:, w:2 * w]


def ray(po, kind, fov, vfov, base, convergence, merge, W, H, eye, cam, x=None, y=None, lens=None):
    """(origin (..., 3), D (..., 3)) of eye `eye` at integer pixel arrays x, y (default: the whole W x H eye frame, [y, x]);
    cam: (4, 3) pos, forward, right, up; merge: (from, to) degrees; lens: rrt_effects' distortion_amount (pinhole) or None"""
    if x is None:
        y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cam = np.asarray(cam, F)
    pos, fw, rt, up = cam
    xf, yf = np.asarray(x).astype(F), np.asarray(y).astype(F)
    hb = half_base(base)
    if kind == pr.EQUIRECT:
        D, _ = pr.d_vector(po, kind, fov, vfov, W, H, x, y, cam)             # projection_dir's D, bit for bit
        lon = ((xf + F(0.5)) / F(W) * F(2.0) - F(1.0)) * pr.half_angle(fov)
        lat = ((yf + F(0.5)) / F(H) * F(2.0) - F(1.0)) * pr.half_angle(vfov)
        lon, lat = np.broadcast_arrays(lon, lat)
        s_lon, c_lon = pr._sincos(po, lon)
        a = np.abs(lat)
        lo, hi = radians(merge[0]), radians(merge[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            ramp = ((hi - a) / (hi - lo)).astype(F)
        f = np.where(a <= lo, F(1.0), np.where(a >= hi, F(0.0), ramp)).astype(F)
        k = (f * hb).astype(F)
        if eye == LEFT:
            k = -k
        R = np.stack([rt[i] * c_lon - fw[i] * s_lon for i in range(3)], axis=-1).astype(F)
    else:
        uvx, uvy = xf / F(W), yf / F(H)
        if lens is not None:                                   # rrt_device.h: lens_distort
            tx, ty = uvx - F(0.5), uvy - F(0.5)
            r2 = tx * tx + ty * ty
            g = F(1.0) + r2 * F(lens)
            uvx, uvy = tx * g + F(0.5), ty * g + F(0.5)
        u = uvx * F(2.0) - F(1.0)
        v = uvy * F(2.0) - F(1.0)
        u = u * (F(W) / F(H))
        ke = -hb if eye == LEFT else hb
        c = F(ke / F(convergence)) if convergence != 0 else F(0.0)
        if c != 0:
            u = u - c
        u, v = np.broadcast_arrays(u, v)
        D = np.stack([fw[i] + (rt[i] * u + up[i] * v) for i in range(3)], axis=-1).astype(F)
        k = np.full(u.shape, ke, F)
        R = np.broadcast_to(rt, u.shape + (3,))
    moved = (pos + R * k[..., None]).astype(F)
    origin = np.where((k != 0)[..., None], moved, np.broadcast_to(pos, moved.shape)).astype(F)
    return origin, D.astype(F)


def rays(po, kind, fov, vfov, base, convergence, merge, W, H, eye, cam):
    """(origin (H, W, 3), unit dir (H, W, 3)) of every pixel of the eye: what rrt_stereo_ray returns"""
    o, D = ray(po, kind, fov, vfov, base, convergence, merge, W, H, eye, cam)
    return o, pr.normalize(D)
