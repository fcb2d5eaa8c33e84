"""The definition of include/rrt_png.h, steps 1-6, restated in numpy -- samples, the five filters, the adaptive choice, the payload,
the row sums and their fold, the file -- and a reader written from the PNG specification's layout (chunk walk, CRC check,
zlib.decompress of the joined IDATs, which verifies the Adler-32, and the unfilter).  Nothing here calls the library."""
import struct
import zlib

import numpy as np

import yuv_ref

F = np.float32
FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")
ADAPTIVE = 5
SLICE_BYTES = 1 << 20
SOFTWARE = b"relativisticraytracer_amd"
HOST_WIDTHS, HOST_HEIGHTS = (1, 2, 5, 7, 8, 9, 63, 64, 65), (1, 2, 17)


def raw_from_rgba8(frame):
    """step 1, depth 8: (h, w * 3) uint8, top-down"""
    return np.ascontiguousarray(np.asarray(frame, np.uint8)[::-1, :, :3]).reshape(frame.shape[0], -1)


def q_from_hdr(po, frame):
    """step 1, depth 16: q_c of "Y4M output", (h, w, 3) uint16, top-down"""
    return yuv_ref.q_from_hdr(po, frame)[::-1].astype(np.uint16)


def raw_from_hdr(po, frame):
    """(h, w * 6) uint8, top-down: every sample two bytes, most significant first"""
    return np.ascontiguousarray(q_from_hdr(po, frame).astype(">u2")).view(np.uint8).reshape(frame.shape[0], -1)


def candidates(raw, bpp):
    """step 2: (5, h, n) uint8 -- every filter of every row, always from RAW bytes"""
    x = raw.astype(np.int64)
    a = np.zeros_like(x)
    a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    da, db, dc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((da <= db) & (da <= dc), a, np.where(db <= dc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)


def scores(cand):
    """step 3: (h, 5) int64"""
    v = cand.astype(np.int64)
    return np.where(v < 128, v, 256 - v).sum(axis=2).T


def choice(cand, filter_name):
    """the filter type of every row: (h,) int64; np.argmin takes the first of equal scores, the lowest type"""
    k = FILTERS.index(filter_name)
    return np.argmin(scores(cand), axis=1) if k == ADAPTIVE else np.full(cand.shape[1], k, np.int64)


def payload(raw, bpp, filter_name):
    """steps 2-5: (the payload as (h, stride) uint8, the types, the row sums as (h, 2) uint32)"""
    cand = candidates(raw, bpp)
    types = choice(cand, filter_name)
    h, n = raw.shape
    out = np.empty((h, 1 + n), np.uint8)
    out[:, 0] = types
    out[:, 1:] = cand[types, np.arange(h)]
    assert n < 1 << 20                                  # 255 * stride^2 / 2 stays far inside int64
    d, weights = out.astype(np.int64), np.arange(1 + n, 0, -1, dtype=np.int64)
    sums = np.stack([d.sum(axis=1) % 65521, (d * weights).sum(axis=1) % 65521], axis=1).astype(np.uint32)
    return out, types, sums


def adler32(sums, stride):
    A, B = 1, 0
    for s1, s2 in np.asarray(sums, np.uint32).reshape(-1, 2).tolist():
        B = (B + s2 + stride * A) % 65521
        A = (A + s1) % 65521
    return B << 16 | A


def chunk(kind, data):
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def header(w, h, depth):
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, 2, 0, 0, 0)) + chunk(b"sRGB", b"\x00")
            + chunk(b"tEXt", b"Software\x00" + SOFTWARE))


def slices(stride, h):
    rows = min(-(-SLICE_BYTES // stride), h)
    return rows, -(-h // rows)


def write_file(pay, sums, w, h, depth, level=4, strategy=zlib.Z_FILTERED):
    """step 6 from a payload of (h, stride) bytes"""
    stride = pay.shape[1]
    rows, n = slices(stride, h)
    out = [header(w, h, depth)]
    for i in range(n):
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
        data = z.compress(pay[i * rows:(i + 1) * rows].tobytes()) + z.flush(zlib.Z_FINISH if i == n - 1 else zlib.Z_SYNC_FLUSH)
        if i == 0:
            data = b"\x78\x01" + data
        if i == n - 1:
            data += struct.pack(">I", adler32(sums, stride))
        out.append(chunk(b"IDAT", data))
    return b"".join(out) + chunk(b"IEND", b"")


def unfilter(pay, bpp):
    """the inverse of step 2, row by row, from the specification: (h, n) uint8"""
    h, stride = pay.shape
    n = stride - 1
    raw = np.zeros((h, n), np.uint8)
    zero = np.zeros(n, np.int64)
    for r in range(h):
        t, v = int(pay[r, 0]), pay[r, 1:].astype(np.int64)
        up = raw[r - 1].astype(np.int64) if r else zero
        assert 0 <= t <= 4, t
        if t == 0:
            cur = v
        elif t == 2:
            cur = v + up
        else:               # the byte to the left is a result: pixel by pixel
            cur = np.zeros(n, np.int64)
            for i in range(0, n, bpp):
                a = cur[i - bpp:i] if i else zero[:bpp]
                b = up[i:i + bpp]
                c = up[i - bpp:i] if i else zero[:bpp]
                if t == 1:
                    pred = a
                elif t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    da, db, dc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
                    pred = np.where((da <= db) & (da <= dc), a, np.where(db <= dc, b, c))
                cur[i:i + bpp] = (v[i:i + bpp] + pred) & 255
        raw[r] = cur & 255
    return raw


def read_file(data):
    """{"width", "height", "depth", "chunks": [type, ...], "idat": [sizes], "text", "samples": (h, w, 3) uint8 | uint16, "types"}"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, kinds, idat, fields, text, intent = 8, [], [], None, None, None
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        kinds.append(kind.decode())
        if kind == b"IHDR":
            fields = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"tEXt":
            text = tuple(body.split(b"\x00", 1))
        elif kind == b"sRGB":
            intent = body[0]
        at += 12 + n
    assert at == len(data) and kinds[0] == "IHDR" and kinds[-1] == "IEND"
    w, h, depth, colour, compression, filtering, interlace = fields
    assert (colour, compression, filtering, interlace) == (2, 0, 0, 0)
    bpp = 3 * depth // 8
    pay = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8).reshape(h, 1 + w * bpp)      # raises on a wrong Adler-32
    raw = unfilter(pay, bpp)
    samples = raw.reshape(h, w, 3) if depth == 8 else raw.view(">u2").astype(np.uint16).reshape(h, w, 3)
    return {"width": w, "height": h, "depth": depth, "chunks": kinds, "idat": [len(b) for b in idat], "text": text, "intent": intent,
            "samples": samples, "types": pay[:, 0].copy()}


# ---- fixtures

def _paeth(a, b, c):
    p = a + b - c
    da, db, dc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((da <= db) & (da <= dc), a, np.where(db <= dc, b, c))


def _structure(rng, w, h):
    """(h, w, 4) values 0 ... 255, TOP-DOWN, built so that adaptive picks every type somewhere when h >= 17 and w >= 5: noise (None),
    a ramp along the row (Sub), a repeated row (Up), a row within 1 of its Paeth prediction, a row within 1 of the mean of left and
    above (Average), and two all-zero rows: None and Sub tie on the first, all five on the second"""
    top = np.zeros((h, w, 4), np.int64)
    x = np.arange(w)[:, None]
    for r in range(h):
        kind = r % 8
        if kind == 1:
            top[r] = rng.integers(0, 256, 4)[None, :] + x * rng.integers(3, 9, 4)[None, :]
        elif kind == 2:
            top[r] = top[r - 1]
        elif kind in (3, 4):
            for i in range(w):
                a, b, c = (top[r, i - 1] if i else 0), top[r - 1, i], (top[r - 1, i - 1] if i else 0)
                top[r, i] = ((_paeth(a, b, c) if kind == 3 else (a + b) >> 1) + rng.integers(-1, 2, 4)) & 255
        elif kind in (5, 6):
            top[r] = 0
        else:
            top[r] = rng.integers(0, 256, (w, 4))
    return top & 255


def rgba8_frame(rng, w, h):
    """(h, w, 4) uint8, bottom-up rows, of _structure; the alpha bytes are noise: they are ignored"""
    top = _structure(rng, w, h)
    top[..., 3] = rng.integers(0, 256, (h, w))
    return top.astype(np.uint8)[::-1].copy()          # a copy: a one-row view would keep its negative stride


def hdr_frame(rng, w, h):
    """(h, w, 4) float32, bottom-up: the tone map's inverse of _structure * 257, so that the structure survives step 1; NaN, +-inf,
    negatives and zeros are mixed into the noise rows, and the second zero row is NaN (q = 0 all the same)"""
    top = _structure(rng, w, h)
    lin = (-np.log1p(-np.minimum(top * 257.0 + 0.5, 65534.0) / 65535.0) / 0.8).astype(F)
    lin[top == 0] = F(0.0)
    for r in range(h):
        if r % 8 in (0, 7):
            kind = rng.integers(0, 24, (w, 4))
            for k, v in ((0, 0.0), (1, -1.5), (2, np.nan), (3, np.inf), (4, -np.inf), (5, -0.0), (6, 1e-30), (7, 3e38)):
                lin[r][kind == k] = F(v)
        elif r % 8 == 6:
            lin[r] = F(np.nan)
    return lin[::-1].copy()


def gpu_sizes(band_rows, wide_threads, narrow_threads):
    """the frames of tests/test_gpu_png.py, the smallest that can go wrong (tests/test_png_geometry.py checks, without a GPU, that
    they still reach what they are there for): name -> (w, h)"""
    sizes = {"one pixel": (1, 1)}
    for w in range(21, 37):                 # sixteen consecutive widths: stride mod 16 takes every residue (depth 8), every odd one (16)
        sizes[f"width {w}"] = (w, 5)
    sizes["two bands plus a row"] = (33, 2 * band_rows + 1)
    sizes["a row of several segments"] = (16384, 3)
    sizes["more chunks than threads"] = (16 * wide_threads // 3 + 40, band_rows + 2)
    sizes["more rows than a narrow workgroup"] = (7, 2 * narrow_threads + 2)
    return sizes


NARROW_SIZES = ("one pixel", "width 21", "width 22", "width 23", "width 24", "two bands plus a row", "more rows than a narrow workgroup")
