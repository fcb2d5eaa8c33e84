"""A numpy restatement of the HDR10 output (include/rrt_yuv.h, "HDR10 output", steps A-G) for the tests: binary32 arithmetic, one
operation per step in the definition's order; the codes, the 4:2:0 siting and the plane layout are yuv_ref's.  `po` is the CPU oracle
binding, whose portable exp and pow are the library's rrt_expf and rrt_powf: the transcendental functions are the oracle's, not the
library's own.  Frames are (h, w, 4) arrays, rows bottom-up; a format is yuv_ref's (chroma, full, 10)."""
import math

import numpy as np

import yuv_ref as yr

F = np.float32
KR, KB = 0.2627, 0.0593
KG = 1.0 - KR - KB
FORMATS = [(c, f, 10) for f in (False, True) for c in (420, 444)]
DEFAULT = (203.0, 1000.0, 0.5)                       # white_nits, peak_nits, knee
M1, M2 = F(0.1593017578125), F(78.84375)
C1, C2, C3 = F(0.8359375), F(18.8515625), F(18.6875)
GAMUT = [[F(0.6274), F(0.3293), F(0.0433)], [F(0.0691), F(0.9195), F(0.0114)], [F(0.0164), F(0.0880), F(0.8956)]]
MASTER = "G(8500,39850)B(6550,2300)R(35400,14600)WP(15635,16450)L({},1)"


def matrix():
    return [[KR, KG, KB],
            [-KR / (2.0 * (1.0 - KB)), -KG / (2.0 * (1.0 - KB)), 0.5],
            [0.5, -KG / (2.0 * (1.0 - KR)), -KB / (2.0 * (1.0 - KR))]]


def coefficients(full):
    """step E: (3 x 3 int64, 3 offsets) by the double formula"""
    A, off = yr.scales(full, 10)
    return (np.array([[yr.llround(K * float(A[r]) * 1073741824.0 / 65535.0) for K in row] for r, row in enumerate(matrix())], np.int64),
            np.array(off, np.int64))


def derived(settings):
    """(white, peak, knee, K, span, inv) in binary32"""
    white, peak, knee = (F(v) for v in settings)
    K = knee * peak
    span = peak - K
    with np.errstate(all="ignore"):
        inv = F(0.0) if knee == F(1.0) else F(1.0) / span
    return white, peak, knee, K, span, inv


def _exp(po, x):
    return po.math_fn(0, po.MATH_PORTABLE, np.asarray(x, F).ravel()).reshape(np.shape(x))


def _pow(po, x, y):
    x = np.asarray(x, F)
    return po.math_fn(1, po.MATH_PORTABLE, x.ravel(), np.full(x.size, y, F)).reshape(x.shape)


def light(H, settings):
    """A: (..., 3) nits"""
    H = np.asarray(H, F)
    with np.errstate(all="ignore"):
        return np.where(H > F(0.0), H * F(settings[0]), F(0.0)).astype(F)


def gamut(a):
    """B"""
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        return np.stack([(g[0] * a[..., 0] + g[1] * a[..., 1]) + g[2] * a[..., 2] for g in GAMUT], axis=-1).astype(F)


def shoulder(po, b, settings):
    """C"""
    _, peak, knee, K, span, inv = derived(settings)
    b = np.asarray(b, F)
    with np.errstate(all="ignore"):
        if knee == F(1.0):
            over = np.full(b.shape, peak, F)
        else:
            over = K + span * (F(1.0) - _exp(po, -((b - K) * inv)))
        c = np.where(b <= K, b, over).astype(F)
        return np.minimum(c, peak).astype(F)


def pq(po, c):
    """D: nits -> sixteen-bit components (int64)"""
    c = np.asarray(c, F)
    y = c * F(1.0e-4)
    p = _pow(po, y, M1)
    e = _pow(po, (C1 + C2 * p) / (F(1.0) + C3 * p), M2)
    v = e * F(65535.0) + F(0.5)
    assert v.dtype == F
    return np.minimum(np.trunc(v).astype(np.int64), 65535)


def nits(po, frame, settings):
    """A-C of an (h, w, 4) frame: (h, w, 3) float32"""
    return shoulder(po, gamut(light(np.asarray(frame, F)[..., :3], settings)), settings)


def code(S, row, n, full):
    coef, off = coefficients(full)
    S = np.asarray(S, np.int64)
    v = S[..., 0] * coef[row, 0] + S[..., 1] * coef[row, 1] + S[..., 2] * coef[row, 2]
    v = (v + (int(off[row]) << (30 + n)) + (1 << (29 + n))) >> (30 + n)
    return np.clip(v, 0, 1023)


def planes(q, fmt):
    """yuv_ref.planes with BT.2020's coefficients"""
    chroma, full, bits = fmt
    assert bits == 10
    d = np.asarray(q, np.int64)[::-1]
    h, w = d.shape[:2]
    y = code(d, 0, 0, full)
    if chroma == 444:
        return y, code(d, 1, 0, full), code(d, 2, 0, full)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    rows, cols = np.minimum(np.arange(2 * ch), h - 1), np.minimum(np.arange(2 * cw), w - 1)
    e = d[rows][:, cols]
    S = e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2]
    return y, code(S, 1, 2, full), code(S, 2, 2, full)


def new_state():
    """F's state as a dict of Python integers"""
    return {"frame_sum": 0, "max_frame_sum": 0, "frame_max": 0, "max_cll": 0, "frames": 0, "reserved": 0}


def meter(c, state):
    """F: a frame's nits into the state, pack and fold.  Every pixel of the (h, w, 3) array counts once."""
    m = np.maximum(np.maximum(c[..., 0], c[..., 1]), c[..., 2]).astype(F)
    v = m * F(64.0)
    assert v.dtype == F
    fx = np.trunc(v).astype(np.int64)
    state["frame_sum"] += int(fx.sum())
    state["frame_max"] = max(state["frame_max"], int(fx.max()))
    state["max_frame_sum"] = max(state["max_frame_sum"], state["frame_sum"])
    state["max_cll"] = max(state["max_cll"], state["frame_max"])
    state["frames"] += 1
    state["frame_sum"] = state["frame_max"] = 0
    return state


def frame(po, hdr, fmt, settings=DEFAULT, state=None):
    """the frame bytes (uint8 array); with a state, the frame is metered and folded into it"""
    c = nits(po, hdr, settings)
    if state is not None:
        meter(c, state)
    return yr.pack(planes(pq(po, c), fmt), 10)


def state_words(state):
    """the state as the 32 bytes the library keeps"""
    return np.array([(state["frame_sum"], state["max_frame_sum"], state["frame_max"], state["max_cll"], state["frames"],
                      state["reserved"])], np.dtype([("a", "<u8"), ("b", "<u8"), ("c", "<u4"), ("d", "<u4"), ("e", "<u4"), ("f", "<u4")])).tobytes()


def levels(state, w, h):
    """MaxCLL, MaxFALL: ceilings in integers"""
    per = 64 * w * h
    return {"max_cll": -(-state["max_cll"] // 64), "max_fall": -(-state["max_frame_sum"] // per), "frames": state["frames"]}


def sidecar(settings, lv):
    """G: the bytes of <path>.hdr10.json"""
    white, peak, knee = (float(F(v)) for v in settings)
    md = MASTER.format(int(math.floor(peak * 10000.0 + 0.5)))
    return ("{\n"
            f'  "white_nits": {white:.9g},\n'
            f'  "peak_nits": {peak:.9g},\n'
            f'  "knee": {knee:.9g},\n'
            f'  "max_cll": {lv["max_cll"]},\n'
            f'  "max_fall": {lv["max_fall"]},\n'
            f'  "frames": {lv["frames"]},\n'
            f'  "master_display": "{md}",\n'
            f'  "x265": "--colorprim bt2020 --transfer smpte2084 --colormatrix bt2020nc --master-display \\"{md}\\" '
            f'--max-cll \\"{lv["max_cll"]},{lv["max_fall"]}\\"",\n'
            '  "ffmpeg": "-color_primaries bt2020 -color_trc smpte2084 -colorspace bt2020nc"\n'
            "}\n").encode()
