"""A numpy restatement of include/rrt_exr.h, independent of the C code: the half conversion in integer arithmetic, the chunk
payload, the pre-deflate filter and its inverse, the file header, a writer and -- the independent check, since no OpenEXR library
is at hand -- a reader that parses a file from the format's published layout (magic, version, attributes, offset table, chunks),
inflates, un-filters and returns the channels.

A format here is (type, compression, half_max): type "half" | "float", compression "none" | "zips" | "zip"."""
import struct
import zlib

import numpy as np

TYPES = {"half": 1, "float": 2}
COMPRESSIONS = {"none": 0, "zips": 2, "zip": 3}
FORMATS = [(t, c) for t in ("half", "float") for c in ("none", "zips", "zip")]
SOFTWARE = b"relativisticraytracer_amd"


def half_bits(x, half_max=65504.0):
    """binary32 -> binary16 bits (uint16 array), round to nearest even, subnormals kept; NaN -> +0, what rounds above half_max
    (inf included) -> +-half_max.  Integer arithmetic on the bits."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    e = a >> 23
    mant = (a & 0x7FFFFF) | 0x800000                 # the value is mant * 2^(e - 150) for e >= 1
    # a half's unit: 2^-24 below 2^-14 (subnormals, e <= 112), else 2^(e - 127 - 10): shift the 24-bit significand right
    shift = np.where(e <= 112, 126 - e, 13)
    shift = np.clip(shift, 13, 40)
    q = mant >> shift
    rem = mant - (q << shift)
    half = np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    # normals: q in [1024, 2048]; the exponent field is e - 112, and q - 1024 adds into it (a carry moves to the next exponent)
    h = np.where(e <= 112, q, ((e - 112) << 10) + (q - 1024))
    h = np.where(a >= 0x47800000, 0x7C00, h)         # 65536 and above, inf
    top = int(np.array([half_max], np.float16).view(np.uint16)[0])
    assert float(np.array([top], np.uint16).view(np.float16)[0]) == float(half_max), "half_max is not a half"
    h = np.minimum(h, top)
    out = np.where(a > 0x7F800000, 0, sign | h)
    return out.astype(np.uint16).reshape(np.shape(x))


def lines_per_chunk(compression):
    return 16 if compression == "zip" else 1


def samples(hdr, type_, half_max=65504.0):
    """(h, 3, w) stored samples, top-down, channels B, G, R: uint16 for half, uint32 for float"""
    a = np.ascontiguousarray(hdr, np.float32)
    top_down = a[::-1, :, 2::-1].transpose(0, 2, 1)          # rows flipped; channels z, y, x = B, G, R
    if type_ == "half":
        return half_bits(np.ascontiguousarray(top_down), half_max)
    return np.ascontiguousarray(top_down).view(np.uint32)


def filter(raw):
    """the format's step in front of deflate: even bytes, then odd bytes, then byte differences + 128"""
    raw = np.frombuffer(bytes(raw), np.uint8)
    tmp = np.concatenate([raw[0::2], raw[1::2]]).astype(np.int64)
    out = tmp.copy()
    out[1:] = (tmp[1:] - tmp[:-1] + 128) & 255
    return out.astype(np.uint8).tobytes()


def unfilter(data):
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    d[1:] -= 128
    tmp = (np.cumsum(d) & 255).astype(np.uint8)
    n = tmp.size
    raw = np.empty(n, np.uint8)
    raw[0::2] = tmp[:n // 2]
    raw[1::2] = tmp[n // 2:]
    return raw.tobytes()


def raw_chunks(hdr, fmt):
    """[(y, raw bytes)] of every chunk"""
    type_, compression = fmt[0], fmt[1]
    s = samples(hdr, type_, *fmt[2:3])
    s = s.astype("<u2" if type_ == "half" else "<u4")
    lines = lines_per_chunk(compression)
    return [(y, s[y:y + lines].tobytes()) for y in range(0, s.shape[0], lines)]


def payload(hdr, fmt):
    """the bytes a pack launch leaves: the chunks one behind the other, filtered unless the compression is none"""
    return np.frombuffer(b"".join(raw if fmt[1] == "none" else filter(raw) for _, raw in raw_chunks(hdr, fmt)), np.uint8)


def _attr(name, type_, data):
    return name + b"\0" + type_ + b"\0" + struct.pack("<i", len(data)) + data


def header(fmt, w, h, fps_num=24, fps_den=1):
    chlist = b"".join(n + b"\0" + struct.pack("<iB3xii", TYPES[fmt[0]], 0, 1, 1) for n in (b"B", b"G", b"R")) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    return (bytes([0x76, 0x2F, 0x31, 0x01]) + struct.pack("<i", 2)
            + _attr(b"channels", b"chlist", chlist)
            + _attr(b"compression", b"compression", bytes([COMPRESSIONS[fmt[1]]]))
            + _attr(b"dataWindow", b"box2i", box)
            + _attr(b"displayWindow", b"box2i", box)
            + _attr(b"lineOrder", b"lineOrder", b"\0")
            + _attr(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
            + _attr(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))
            + _attr(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
            + _attr(b"chromaticities", b"chromaticities", struct.pack("<8f", 0.64, 0.33, 0.30, 0.60, 0.15, 0.06, 0.3127, 0.3290))
            + _attr(b"framesPerSecond", b"rational", struct.pack("<iI", fps_num, fps_den))
            + _attr(b"software", b"string", SOFTWARE)
            + b"\0")


def write_file(hdr, fmt, fps=24, level=4):
    """the whole file's bytes; with zips / zip a chunk that deflate does not shrink is stored raw"""
    a = np.ascontiguousarray(hdr, np.float32)
    h, w = a.shape[:2]
    head = header(fmt, w, h, fps, 1)
    pieces = []
    for y, raw in raw_chunks(a, fmt):
        data = raw
        if fmt[1] != "none":
            z = zlib.compress(filter(raw), level)
            data = z if len(z) < len(raw) else raw
        pieces.append((y, data))
    at, table, body = len(head) + 8 * len(pieces), [], b""
    for y, data in pieces:
        table.append(at + len(body))
        body += struct.pack("<ii", y, len(data)) + data
    return head + struct.pack(f"<{len(table)}Q", *table) + body


def _cstr(b, at):
    end = b.index(b"\0", at)
    return b[at:end], end + 1


def read_file(data):
    """Parse an EXR file's bytes.  Returns {"attributes": {name: (type, bytes)}, "width", "height", "type", "compression",
    "channels": {"B" | "G" | "R": (h, w) array, float16 or float32}, "raw_chunks": how many compressed-format chunks were stored
    raw}.  Asserts what a scanline reader relies on."""
    b = bytes(data)
    assert b[:4] == bytes([0x76, 0x2F, 0x31, 0x01]), "magic"
    version, = struct.unpack_from("<i", b, 4)
    assert version == 2, "version 2, no flags: single part, scanlines"
    at, attrs = 8, {}
    while b[at] != 0:
        name, at = _cstr(b, at)
        type_, at = _cstr(b, at)
        size, = struct.unpack_from("<i", b, at)
        attrs[name.decode()] = (type_.decode(), b[at + 4:at + 4 + size])
        at += 4 + size
    at += 1
    for required in ("channels", "compression", "dataWindow", "displayWindow", "lineOrder", "pixelAspectRatio", "screenWindowCenter",
                     "screenWindowWidth"):
        assert required in attrs, required
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    assert (x0, y0) == (0, 0) and attrs["displayWindow"][1] == attrs["dataWindow"][1]
    w, h = x1 + 1, y1 + 1
    assert attrs["lineOrder"] == ("lineOrder", b"\0")
    ch, cat, names, ptype = attrs["channels"][1], 0, [], None
    while ch[cat] != 0:
        name, cat = _cstr(ch, cat)
        t, plinear, xs, ys = struct.unpack_from("<iB3xii", ch, cat)
        cat += 16
        assert (xs, ys) == (1, 1) and (ptype is None or t == ptype)
        ptype = t
        names.append(name.decode())
    assert cat + 1 == len(ch) and names == sorted(names) == ["B", "G", "R"]
    comp = attrs["compression"][1][0]
    assert comp in (0, 2, 3) and ptype in (1, 2)
    lines = 16 if comp == 3 else 1
    bps = 2 if ptype == 1 else 4
    n_chunks = (h + lines - 1) // lines
    table = struct.unpack_from(f"<{n_chunks}Q", b, at)
    at += 8 * n_chunks
    dtype = np.dtype("<f2") if ptype == 1 else np.dtype("<f4")
    out = np.empty((h, 3, w), dtype)
    stored_raw = 0
    for i, pos in enumerate(table):
        assert pos == at, "chunks lie one behind the other in increasing y"
        y, size = struct.unpack_from("<ii", b, pos)
        rows = min(lines, h - i * lines)
        assert y == i * lines
        piece = b[pos + 8:pos + 8 + size]
        assert len(piece) == size
        n = rows * w * 3 * bps
        if comp != 0 and size < n:
            piece = unfilter(zlib.decompress(piece))
        elif comp != 0:
            stored_raw += 1
        assert len(piece) == n
        out[y:y + rows] = np.frombuffer(piece, dtype).reshape(rows, 3, w)
        at = pos + 8 + size
    assert at == len(b), "nothing behind the last chunk"
    return {"attributes": attrs, "width": w, "height": h, "type": {1: "half", 2: "float"}[ptype],
            "compression": {0: "none", 2: "zips", 3: "zip"}[comp], "raw_chunks": stored_raw,
            "channels": {name: out[:, k, :] for k, name in enumerate(("B", "G", "R"))}}


def hdr_frame(rng, w, h):
    """an (h, w, 4) float32 HDR frame: most values in the renderer's range, with zeros, tiny and huge values, negatives, infs and
    NaNs scattered in"""
    a = np.exp2(rng.uniform(-16.0, 6.0, (h, w, 4))).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 65520.0, 1e-8, -3.5, 6e-8, 3.4e38], np.float32)
    pick = rng.random((h, w, 4)) < 0.08
    a[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    return a


def conversion_inputs():
    """the binary32 values the half conversion is pinned on (float32 array): every half's value, each +-1 ulp; every midpoint
    between adjacent finite halves (and the one between 65504 and 65536), each +-1 ulp; the clamp's neighbourhood, FLT_MAX, infs,
    NaNs of both signs and several payloads, zeros; binary32 subnormals; the smallest half subnormal's half and quarter"""
    halves = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
    finite = np.arange(0x7C00, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float64)
    mid = (np.append(finite[:-1] + finite[1:], 65504.0 + 65536.0) / 2.0).astype(np.float32)      # exact: 12 significant bits
    assert np.array_equal(mid.astype(np.float64) * 2.0, np.append(finite[:-1] + finite[1:], 65504.0 + 65536.0))
    mid = np.concatenate([mid, -mid]).view(np.uint32)
    special = np.array([65504.0, 65519.996, 65520.0, 65536.0, 3.4028234663852886e38, np.inf, -np.inf, 0.0, -0.0, -65519.996, -65520.0,
                        2.0 ** -25, 2.0 ** -26, -2.0 ** -25, -2.0 ** -26, 1024.0, 1024.4, 1024.5, 1024.6, 1025.0, -1024.6, 2047.0],
                       np.float32).view(np.uint32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000, 0xFFA5A5A5], np.uint32)
    sub = np.array([0x00000001, 0x00000002, 0x00400000, 0x007FFFFF, 0x00800000, 0x80000001, 0x80400000, 0x807FFFFF, 0x00012345], np.uint32)
    around = np.concatenate([special, special + np.uint32(1), special - np.uint32(1)])
    return np.concatenate([halves, halves + np.uint32(1), halves - np.uint32(1), mid, mid + np.uint32(1), mid - np.uint32(1),
                           around, nans, sub]).view(np.float32)


def frame_of(values, w):
    """the values laid out as an (h, w, 4) frame: R, G, B of consecutive pixels, alpha 1, padded with 0.5"""
    v = np.ascontiguousarray(values, np.float32).ravel()
    h = -(-v.size // (3 * w))
    rgb = np.full(h * w * 3, 0.5, np.float32)
    rgb[:v.size] = v
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rgb.reshape(h, w, 3)
    return out


# the sizes the device tests run, by the branch each is there for (tests/test_exr_geometry.py checks, without a GPU, that each
# still reaches it): (w, h, bytes the payload pointer is moved off the 16-byte grid)
WIDE_CASES = [(8, 1, 0), (8, 16, 0), (64, 17, 0), (72, 33, 0), (1024, 16, 0)]
NARROW_CASES = [(1, 1, 0), (7, 3, 0), (9, 17, 0), (65, 16, 0)]
OFFSET_CASE = (64, 17, 2)          # an aligned width on the narrow path
WRAP_CASE = (256, 4112, 0)         # the grid's row dimension wraps
GPU_CASES = WIDE_CASES + NARROW_CASES + [OFFSET_CASE, WRAP_CASE]
