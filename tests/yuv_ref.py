"""A numpy restatement of the Y'CbCr packing (include/rrt_yuv.h, steps 1-5) for the tests: int64 arithmetic throughout, one
operation per step in the definition's order.  Frames are (h, w, 4) arrays, rows bottom-up as every launch writes them; a format is
(chroma, full, bits) with chroma 420 | 444, full False | True, bits 8 | 10.  `po` is the CPU oracle binding, whose portable exp is
the library's rrt_expf: the HDR path's tone map is the oracle's, as in exposure_ref.tone_map, not the library's own."""
import math

import numpy as np

F = np.float32
FORMATS = [(c, f, b) for b in (8, 10) for f in (False, True) for c in (420, 444)]
TAG = {(420, 8): "420jpeg", (444, 8): "444", (420, 10): "420p10", (444, 10): "444p10"}
KR, KB = 0.2126, 0.0722
KG = 1.0 - KR - KB


def matrix():
    """step 2's rows (Y, Cb, Cr) as Python floats: binary64, one rounding per operation"""
    return [[KR, KG, KB],
            [-KR / (2.0 * (1.0 - KB)), -KG / (2.0 * (1.0 - KB)), 0.5],
            [0.5, -KG / (2.0 * (1.0 - KR)), -KB / (2.0 * (1.0 - KR))]]


def scales(full, bits):
    """(A per row, offset per row)"""
    k = 1 << (bits - 8)
    if full:
        return [(1 << bits) - 1] * 3, [0, 1 << (bits - 1), 1 << (bits - 1)]
    return [219 * k, 224 * k, 224 * k], [16 * k, 1 << (bits - 1), 1 << (bits - 1)]


def llround(x):
    """C's llround: halves away from zero"""
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def coefficients(full, bits):
    """step 2: (3 x 3 int64, 3 offsets) by the double formula"""
    A, off = scales(full, bits)
    return (np.array([[llround(K * float(A[r]) * 1073741824.0 / 65535.0) for K in row] for r, row in enumerate(matrix())], np.int64),
            np.array(off, np.int64))


def q_from_rgba8(frame):
    """step 1 from bytes: (h, w, 3) int64"""
    return np.asarray(frame, np.uint8)[..., :3].astype(np.int64) * 257


def tone(po, rgb):
    """1.0f - rrt_expf(-H * 0.8f) with the oracle's portable exp: exposure_ref.tone_map up to its cast"""
    with np.errstate(all="ignore"):
        x = (-np.asarray(rgb, F)) * F(0.8)
        e = po.math_fn(0, po.MATH_PORTABLE, x.ravel()).reshape(x.shape)
        return F(1.0) - e


def q_from_hdr(po, frame):
    """step 1 from linear HDR: (h, w, 3) int64; NaN and t <= 0 give 0"""
    t = tone(po, np.asarray(frame, F)[..., :3])
    with np.errstate(all="ignore"):
        v = t * F(65535.0)
        assert v.dtype == F
        pos = t > F(0.0)
        q = np.where(pos, np.minimum(np.trunc(np.where(pos, v, F(0.0))).astype(np.int64), 65535), 0)
    return q


def code(S, row, n, full, bits):
    """step 3 on (..., 3) int64 sums of 2^n pixels"""
    coef, off = coefficients(full, bits)
    S = np.asarray(S, np.int64)
    v = S[..., 0] * coef[row, 0] + S[..., 1] * coef[row, 1] + S[..., 2] * coef[row, 2]
    v = (v + (int(off[row]) << (30 + n)) + (1 << (29 + n))) >> (30 + n)
    return np.clip(v, 0, (1 << bits) - 1)


def planes(q, fmt):
    """(Y, Cb, Cr) as int64 arrays in display order (top-down) from (h, w, 3) q in buffer order (bottom-up)"""
    chroma, full, bits = fmt
    d = np.asarray(q, np.int64)[::-1]
    h, w = d.shape[:2]
    y = code(d, 0, 0, full, bits)
    if chroma == 444:
        return y, code(d, 1, 0, full, bits), code(d, 2, 0, full, bits)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    rows, cols = np.minimum(np.arange(2 * ch), h - 1), np.minimum(np.arange(2 * cw), w - 1)
    e = d[rows][:, cols]
    S = e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2]
    return y, code(S, 1, 2, full, bits), code(S, 2, 2, full, bits)


def pack(ps, bits):
    """step 4: the planes' bytes, tightly packed"""
    dt = np.uint8 if bits == 8 else np.dtype("<u2")
    return np.frombuffer(b"".join(np.ascontiguousarray(p.astype(dt)).tobytes() for p in ps), np.uint8)


def frame_from_rgba8(frame, fmt):
    return pack(planes(q_from_rgba8(frame), fmt), fmt[2])


def frame_from_hdr(po, frame, fmt):
    return pack(planes(q_from_hdr(po, frame), fmt), fmt[2])


def frame_bytes(fmt, w, h):
    """(bytes, plane offsets)"""
    chroma, _, bits = fmt
    bps = 1 if bits == 8 else 2
    cw, ch = ((w + 1) >> 1, (h + 1) >> 1) if chroma == 420 else (w, h)
    return (w * h + 2 * cw * ch) * bps, (0, w * h * bps, (w * h + cw * ch) * bps)


def header(fmt, w, h, fps_num=24, fps_den=1):
    """step 5's header line"""
    chroma, full, bits = fmt
    return (f"YUV4MPEG2 W{w} H{h} F{fps_num}:{fps_den} Ip A1:1 C{TAG[(chroma, bits)]} "
            f"XCOLORRANGE={'FULL' if full else 'LIMITED'}\n").encode()


def parse_y4m(data, fmt, w, h):
    """(header line, [frame bytes as uint8 arrays]) of a stream; asserts the framing"""
    end = data.index(b"\n") + 1
    n, _ = frame_bytes(fmt, w, h)
    frames, at = [], end
    while at < len(data):
        assert data[at:at + 6] == b"FRAME\n", data[at:at + 6]
        frames.append(np.frombuffer(data[at + 6:at + 6 + n], np.uint8))
        assert len(frames[-1]) == n
        at += 6 + n
    return data[:end], frames


def sizes(geometry):
    """the sizes the host and the GPU tests share: the odd ones, those around 1023 (a Cb plane at an odd address), and those that
    straddle a strip's and a workgroup's width by -1, 0, +1 (from the library's own geometry)"""
    fixed = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 5), (7, 5), (64, 48), (65, 47), (1022, 3), (1023, 3)]
    sw, block = geometry["strip_w"], geometry["strip_w"] * geometry["threads"]
    around = [(sw + d, 3) for d in (-1, 0, 1)] + [(block + d, 2 * geometry["strip_h"] + 1) for d in (-1, 0, 1)]
    return fixed + [s for s in around if s not in fixed]


def hdr_frame(rng, w, h):
    """log-uniform over 2^-20 ... 2^20 with zeros, negatives, NaN and +-inf mixed in"""
    a = np.exp2(rng.uniform(-20.0, 20.0, (h, w, 4))).astype(F)
    kind = rng.integers(0, 24, (h, w, 4))
    for k, v in ((0, 0.0), (1, -1.5), (2, np.nan), (3, np.inf), (4, -np.inf), (5, -0.0)):
        a[kind == k] = F(v)
    return a
