"""A numpy float32 restatement of a panorama's primary ray (include/rrt.h: rrt_projection) for the tests.  Every operation is one
float32 operation in the contract's order; sin and cos are the oracle's portable rrt_sincosf (pinned bit for bit to the device's),
normalize and the nudge hash are restated as rrt_device.h / rrt_kernels.h write them.  Pixel arrays are indexed [y, x] with y the
virtual row as the kernel sees it (+y toward `up`), not the stored (bottom-up) row."""
import numpy as np

F = np.float32
PINHOLE, EQUIRECT, FISHEYE = 0, 1, 2
M32 = np.uint64(0xFFFFFFFF)


def half_angle(deg):
    """(float)((double)deg * 3.14159265358979323846 / 360.0)"""
    return F(float(F(deg)) * 3.14159265358979323846 / 360.0)


def _sincos(po, x):
    flat = np.ascontiguousarray(x, F).ravel()
    s = po.math_fn(2, po.MATH_PORTABLE, flat).reshape(x.shape)
    c = po.math_fn(3, po.MATH_PORTABLE, flat).reshape(x.shape)
    return s.astype(F), c.astype(F)


def factors(po, kind, fov, vfov, W, H, x, y):
    """(A, B, C, inside) of D = fw*A + (rt*B + up*C) at integer pixel arrays x, y"""
    xf, yf = np.asarray(x).astype(F), np.asarray(y).astype(F)
    inside = np.ones(np.broadcast(xf, yf).shape, bool)
    if kind == EQUIRECT:
        lon = ((xf + F(0.5)) / F(W) * F(2.0) - F(1.0)) * half_angle(fov)
        lat = ((yf + F(0.5)) / F(H) * F(2.0) - F(1.0)) * half_angle(vfov)
        lon, lat = np.broadcast_arrays(lon, lat)
        s_lat, c_lat = _sincos(po, lat)
        s_lon, c_lon = _sincos(po, lon)
        return c_lat * c_lon, c_lat * s_lon, s_lat, inside
    if kind == FISHEYE:
        u = (F(2.0) * (xf + F(0.5)) - F(W)) / F(H)
        v = (F(2.0) * (yf + F(0.5)) - F(H)) / F(H)
        u, v = np.broadcast_arrays(u, v)
        r2 = u * u + v * v
        inside = ~(r2 > F(1.0))
        r = np.sqrt(np.where(inside, r2, F(0.0))).astype(F)
        s_t, c_t = _sincos(po, r * half_angle(fov))
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(r > F(0.0), s_t / r, F(0.0)).astype(F)
        return c_t, u * k, v * k, inside
    u = (xf / F(W)) * F(2.0) - F(1.0)                      # raymarcher.cu:20-34, no lens
    v = (yf / F(H)) * F(2.0) - F(1.0)
    u = u * (F(W) / F(H))
    u, v = np.broadcast_arrays(u, v)
    return np.ones_like(u), u, v, inside


def d_vector(po, kind, fov, vfov, W, H, x, y, cam):
    """(D (..., 3) before normalisation, inside); cam: (4, 3) pos, forward, right, up"""
    cam = np.asarray(cam, F)
    A, B, C, inside = factors(po, kind, fov, vfov, W, H, x, y)
    D = np.stack([cam[1, i] * A + (cam[2, i] * B + cam[3, i] * C) for i in range(3)], axis=-1).astype(F)
    return D, inside


def normalize(D):
    """rrt_device.h: normalize (length: sqrtf((x*x + y*y) + z*z), then below 1e-6f the zero vector)"""
    D = np.asarray(D, F)
    mag = np.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (D / mag[..., None]).astype(F)
    return np.where((mag < F(1e-6))[..., None], F(0.0), out).astype(F)


def directions(po, kind, fov, vfov, W, H, cam):
    """(dir (H, W, 3), inside (H, W)) of every pixel of a W x H frame: what rrt_projection_ray returns, before any nudge"""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    D, inside = d_vector(po, kind, fov, vfov, W, H, x, y, cam)
    return np.where(inside[..., None], normalize(D), F(0.0)).astype(F), inside


def _mix(v):
    v = v & M32
    v ^= v >> np.uint64(16); v = (v * np.uint64(0x7FEB352D)) & M32
    v ^= v >> np.uint64(15); v = (v * np.uint64(0x846CA68B)) & M32
    v ^= v >> np.uint64(16)
    return v


def nudge(vel, K, seed, x, y):
    """rrt_kernels.h: nudge_component on every component of vel (..., 3) at integer pixel arrays x, y"""
    vel = np.asarray(vel, F)
    x = np.asarray(x, np.uint64); y = np.asarray(y, np.uint64)
    out = np.empty_like(vel)
    base = _mix((x * np.uint64(0x9E3779B1) + y) & M32)
    for comp in range(3):
        salt = np.uint64((int(seed) * 0x85EBCA6B + comp * 0xC2B2AE35) & 0xFFFFFFFF)
        h = _mix(base ^ salt)
        k = (h % np.uint64(2 * K + 1)).astype(np.int64) - K
        b = np.ascontiguousarray(vel[..., comp]).view(np.uint32).astype(np.int64)
        m = b & 0x7FFFFFFF
        m = np.where(b >> 31 != 0, -m, m) + k
        bits = np.where(m < 0, 0x80000000 | (-m), m).astype(np.uint32)
        out[..., comp] = bits.view(F)
    return out
