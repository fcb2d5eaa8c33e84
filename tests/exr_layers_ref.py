"""A numpy restatement of include/rrt_exr.h's data layers, independent of the C code: the six conversions, scanlines of mixed sample
sizes, chunks, the pre-deflate filter over them, the payload, the header and the whole file for ANY channel list, and a reader for
multi-channel files of all three pixel types written from the format's published layout.  The filter, its inverse and the half
conversion are tests/exr_ref.py's; nothing here calls the library.

A layer set here is (channels, planes): planes {key: (array, bottom_up)} with arrays (h, w, words) or (h, w), float32 or int32;
channels [(name, type, key, word)] with type "uint" | "half" | "float", in any order -- the file's order is the names' byte order."""
import struct
import zlib

import numpy as np

import exr_ref as xr

TYPES = {"uint": 0, "half": 1, "float": 2}
TYPE_NAMES = {v: k for k, v in TYPES.items()}
DTYPES = {"uint": np.dtype("<u4"), "half": np.dtype("<u2"), "float": np.dtype("<u4")}
VIEWS = {"uint": np.dtype("<u4"), "half": np.dtype("<f2"), "float": np.dtype("<f4")}
COMPRESSIONS = ("none", "zips", "zip")
LAYER_NAMES = ("steps", "horizon", "transmittance", "emission", "direction", "position")


def convert(values, type_, half_max=65504.0):
    """the stored samples of a float32 or int32 array: uint16 for half, uint32 otherwise"""
    v = np.ascontiguousarray(values)
    if v.dtype == np.int32:
        if type_ == "uint":
            return np.maximum(v, 0).astype(np.uint32)
        v = v.astype(np.float32)                     # round to nearest even
    else:
        assert v.dtype == np.float32 and type_ != "uint", "an F32 source is not stored as UINT"
    return xr.half_bits(v, half_max) if type_ == "half" else v.view(np.uint32)


def ordered(channels):
    out = sorted(channels, key=lambda c: c[0].encode())
    assert all(a[0] != b[0] for a, b in zip(out, out[1:])), "duplicate names"
    return out


def samples(channels, planes, half_max=65504.0):
    """[(name, type, (h, w) little-endian sample array)] top-down, in the file's order"""
    out = []
    for name, type_, key, word in ordered(channels):
        a, bottom_up = planes[key]
        a = np.asarray(a)
        a = a.reshape(a.shape[0], a.shape[1], -1)[:, :, word]
        if bottom_up:
            a = a[::-1]
        out.append((name, type_, convert(a, type_, half_max).astype(DTYPES[type_])))
    return out


def raw_chunks(channels, planes, compression, half_max=65504.0):
    """[(y, raw bytes)] of every chunk: its scanlines top-down, each the channels one behind the other"""
    s = samples(channels, planes, half_max)
    h = s[0][2].shape[0]
    lines = xr.lines_per_chunk(compression)
    return [(y0, b"".join(a[y].tobytes() for y in range(y0, min(y0 + lines, h)) for _, _, a in s)) for y0 in range(0, h, lines)]


def payload(channels, planes, compression, half_max=65504.0):
    return np.frombuffer(b"".join(raw if compression == "none" else xr.filter(raw)
                                  for _, raw in raw_chunks(channels, planes, compression, half_max)), np.uint8)


def bytes_per_pixel(channels):
    return sum(2 if t == "half" else 4 for _, t, _, _ in channels)


def chunk_table(channels, w, h, compression):
    """[(y, offset, bytes)] of every chunk in the payload"""
    lines, bpp = xr.lines_per_chunk(compression), bytes_per_pixel(channels)
    return [(y, y * w * bpp, min(lines, h - y) * w * bpp) for y in range(0, h, lines)]


def header(channels, w, h, compression, fps_num=24, fps_den=1):
    chlist = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", TYPES[t], 0, 1, 1) for n, t, _, _ in ordered(channels)) + b"\0"
    box = struct.pack("<4i", 0, 0, w - 1, h - 1)
    a = xr._attr
    return (bytes([0x76, 0x2F, 0x31, 0x01]) + struct.pack("<i", 2)
            + a(b"channels", b"chlist", chlist)
            + a(b"compression", b"compression", bytes([xr.COMPRESSIONS[compression]]))
            + a(b"dataWindow", b"box2i", box)
            + a(b"displayWindow", b"box2i", box)
            + a(b"lineOrder", b"lineOrder", b"\0")
            + a(b"pixelAspectRatio", b"float", struct.pack("<f", 1.0))
            + a(b"screenWindowCenter", b"v2f", struct.pack("<2f", 0.0, 0.0))
            + a(b"screenWindowWidth", b"float", struct.pack("<f", 1.0))
            + a(b"chromaticities", b"chromaticities", struct.pack("<8f", 0.64, 0.33, 0.30, 0.60, 0.15, 0.06, 0.3127, 0.3290))
            + a(b"framesPerSecond", b"rational", struct.pack("<iI", fps_num, fps_den))
            + a(b"software", b"string", xr.SOFTWARE)
            + b"\0")


def write_file(channels, planes, compression, fps=24, level=4, half_max=65504.0):
    """the whole file's bytes; with zips / zip a chunk that deflate does not shrink is stored raw"""
    first = np.asarray(planes[channels[0][2]][0])
    h, w = first.shape[:2]
    head = header(channels, w, h, compression, fps, 1)
    pieces = []
    for y, raw in raw_chunks(channels, planes, compression, half_max):
        data = raw
        if compression != "none":
            z = zlib.compress(xr.filter(raw), level)
            data = z if len(z) < len(raw) else raw
        pieces.append((y, data))
    table, body = [], b""
    for y, data in pieces:
        table.append(len(head) + 8 * len(pieces) + len(body))
        body += struct.pack("<ii", y, len(data)) + data
    return head + struct.pack(f"<{len(table)}Q", *table) + body


def read_file(data):
    """Parse a single-part scanline EXR file of any channel list.  Returns {"attributes", "width", "height", "compression",
    "types": {name: "uint" | "half" | "float"}, "names": the channels in the file's order, "channels": {name: (h, w) array --
    uint32, float16 or float32}, "raw_chunks": how many compressed-format chunks were stored raw}."""
    b = bytes(data)
    assert b[:4] == bytes([0x76, 0x2F, 0x31, 0x01]), "magic"
    assert struct.unpack_from("<i", b, 4)[0] == 2, "version 2, no flags: single part, scanlines, short names"
    at, attrs = 8, {}
    while b[at] != 0:
        name, at = xr._cstr(b, at)
        type_, at = xr._cstr(b, at)
        size, = struct.unpack_from("<i", b, at)
        attrs[name.decode()] = (type_.decode(), b[at + 4:at + 4 + size])
        at += 4 + size
    at += 1
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    assert (x0, y0) == (0, 0) and attrs["displayWindow"][1] == attrs["dataWindow"][1] and attrs["lineOrder"] == ("lineOrder", b"\0")
    w, h = x1 + 1, y1 + 1
    ch, cat, names, types = attrs["channels"][1], 0, [], {}
    while ch[cat] != 0:
        name, cat = xr._cstr(ch, cat)
        assert 1 <= len(name) <= 31
        t, plinear, xs, ys = struct.unpack_from("<iB3xii", ch, cat)
        cat += 16
        assert (xs, ys, plinear) == (1, 1, 0) and t in TYPE_NAMES
        names.append(name.decode())
        types[name.decode()] = TYPE_NAMES[t]
    assert cat + 1 == len(ch) and [n.encode() for n in names] == sorted(set(n.encode() for n in names)), "channels sorted, no duplicates"
    comp = attrs["compression"][1][0]
    assert comp in (0, 2, 3)
    lines = 16 if comp == 3 else 1
    bpp = sum(2 if types[n] == "half" else 4 for n in names)
    n_chunks = (h + lines - 1) // lines
    table = struct.unpack_from(f"<{n_chunks}Q", b, at)
    at += 8 * n_chunks
    out = {n: np.empty((h, w), VIEWS[types[n]]) for n in names}
    stored_raw = 0
    for i, pos in enumerate(table):
        assert pos == at, "chunks lie one behind the other in increasing y"
        y, size = struct.unpack_from("<ii", b, pos)
        rows = min(lines, h - i * lines)
        assert y == i * lines
        piece = b[pos + 8:pos + 8 + size]
        assert len(piece) == size
        n = rows * w * bpp
        if comp != 0 and size < n:
            piece = xr.unfilter(zlib.decompress(piece))
        elif comp != 0:
            stored_raw += 1
        assert len(piece) == n
        k = 0
        for r in range(rows):
            for name in names:
                dt = VIEWS[types[name]]
                out[name][y + r] = np.frombuffer(piece, dt, w, k)
                k += w * dt.itemsize
        at = pos + 8 + size
    assert at == len(b), "nothing behind the last chunk"
    return {"attributes": attrs, "width": w, "height": h, "compression": {0: "none", 2: "zips", 3: "zip"}[comp], "types": types,
            "names": names, "channels": out, "raw_chunks": stored_raw}


# ---- the layer sets and sizes the tests share

def standard_channels(layers, beauty):
    """B, G, R of type `beauty` next to the drivers' standard layers (--exr-layers): names, types and sources as the issue's table"""
    out = [("B", beauty, "hdr", 2), ("G", beauty, "hdr", 1), ("R", beauty, "hdr", 0)]
    table = {"steps": [("steps", "uint", "steps", 0)],
             "horizon": [("horizon", "half", "hit", 0)],
             "transmittance": [("transmittance", beauty, "rad", 3)],
             "emission": [("emission.B", beauty, "rad", 2), ("emission.G", beauty, "rad", 1), ("emission.R", beauty, "rad", 0)],
             "direction": [("direction." + "XYZ"[k], "float", "vel", k) for k in range(3)],
             "position": [("position." + "XYZ"[k], "float", "pos", k) for k in range(3)]}
    for name in layers:
        out += table[name]
    return out


# every type follows every other type across a channel seam: H F, F H, H U, U F, F U and, from a row's end to the next row, U H;
# an odd number of HALF channels lies ahead of b.float
MIXED = [("a.half", "half", "hdr", 0), ("b.float", "float", "vel", 1), ("c.half", "half", "steps", 0), ("d.uint", "uint", "hit", 0),
         ("e.float", "float", "steps", 0), ("f.uint", "uint", "steps", 0)]
LAYER_SETS = {"bgr_half": standard_channels((), "half"), "bgr_float": standard_channels((), "float"),
              "all_half": standard_channels(LAYER_NAMES, "half"), "all_float": standard_channels(LAYER_NAMES, "float"),
              "mixed": MIXED, "uint": [("steps", "uint", "steps", 0)]}


def random_planes(rng, w, h):
    """the six planes a debug launch leaves, of random bit patterns (NaNs and infs included) with the renderer's ranges mixed in:
    {key: (array, bottom_up)}"""
    def bits(*shape):
        a = rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(np.float32)
        tame = xr.hdr_frame(rng, w, h)[..., :shape[2]]
        pick = rng.random(shape) < 0.5
        a[pick] = tame[pick]
        return a
    steps = rng.integers(-5, 70000, (h, w), dtype=np.int64).astype(np.int32)
    edge = np.array([-1, 0, 1, 2047, 2048, 2049, 65504, 65519, 65520, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)
    pick = rng.random((h, w)) < 0.2
    steps[pick] = edge[rng.integers(0, edge.size, int(pick.sum()))]
    return {"hdr": (bits(h, w, 4), True), "rad": (bits(h, w, 4), False), "pos": (bits(h, w, 3), False), "vel": (bits(h, w, 3), False),
            "steps": (steps, False), "hit": (rng.integers(0, 2, (h, w), dtype=np.int64).astype(np.int32), False)}


def api_layers(rrt, channels, planes, w, h, compression, half_max=None, on=None):
    """the library's ExrLayers for a layer set; `on`: {key: tensor or array} to stand in for the planes' arrays (device tensors)"""
    fmt = rrt.ExrFormat("half", compression, half_max)
    on = on or {}
    return rrt.ExrLayers(fmt, w, h, [(n, t, on.get(k, planes[k][0]), word, planes[k][1]) for n, t, k, word in channels])


# the sizes the device tests run, by the branch each is there for (tests/test_exr_layers_geometry.py checks, without a GPU, that
# each reaches it): (w, h)
WIDE_CASES = [(8, 1), (8, 16), (24, 17), (64, 33), (72, 16)]
NARROW_CASES = [(1, 1), (7, 3), (9, 17), (65, 16)]
MOVED_CASE = (64, 17)              # with the payload moved 2 bytes, and again with one source moved 4 bytes: the narrow path
WRAP_CASE = (8, 4112)              # the grid's row dimension wraps on the wide path
