"""Adaptive supersampling's mask rule (include/rrt.h: rrt_launch_raymarch_adaptive), restated in numpy integer arithmetic: test
infrastructure shared by tests/test_adaptive_host.py and tests/test_gpu_adaptive.py."""
import numpy as np


def mask(rgba8, T):
    """(h, w) bool: pixel p of the stored (h, w, 4) uint8 frame is refined iff it differs from its left, right, upper or lower
    neighbour by more than T in r, g or b.  Alpha is ignored; at the frame's edge the missing neighbour is the pixel itself (a
    difference of 0): no wrap.  Each pair of neighbours marks both of its pixels."""
    a = np.asarray(rgba8)
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 4, (a.dtype, a.shape)
    c = a[..., :3].astype(np.int32)
    m = np.zeros(c.shape[:2], bool)
    across = np.abs(c[:, 1:] - c[:, :-1]).max(axis=2) > T        # (h, w - 1): column x against x + 1
    m[:, 1:] |= across
    m[:, :-1] |= across
    along = np.abs(c[1:] - c[:-1]).max(axis=2) > T               # (h - 1, w): row against the next
    m[1:] |= along
    m[:-1] |= along
    return m


def expected(base, ss, m):
    """out = where(mask, ss, base) for (h, w, 4) frames of any dtype"""
    return np.where(m[..., None], ss, base)
