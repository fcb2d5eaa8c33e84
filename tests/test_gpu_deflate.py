"""Device deflate on the device: rrt_launch_deflate against rrt_deflate_host and the Python restatement (tests/deflate_ref.py), stream
bytes byte for byte and stream sizes word for word, on every fixture the host tests use (tests/test_deflate_geometry.py keeps them on
their branches), with guard bytes behind the output, the size table and the scratch, off the 16-byte grid, launched twice, and
captured into a graph; and both headless drivers' --png-deflate device files against their --png-deflate host files.

The same again at a full frame's cut (tests/deflate_ref.py: large_fixtures): hundreds of full-size segments -- stored ones, and dynamic
ones a few dozen bytes short of stored -- in streams of two, three and 34 segments with a short last stream, over three rounds of
deflate_offsets and more workgroups than the chip holds at once; on scratch another launch left behind; with d_out off the 16-byte
grid; and the drivers at frames of several slices, with more frames than twice the slots."""
import json
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import deflate_ref as dr
import png_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SENTINEL, GUARD = 0xA5, 64


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def cases(po):
    """every fixture, shared and left unchanged: {name: (bytes, device tensor holding them 16-byte aligned, stream_bytes)}"""
    import torch
    out = {}
    for name, (data, stream_bytes) in dr.fixtures(po).items():
        d = torch.from_numpy(np.ascontiguousarray(data)).cuda() if data.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
        assert d.data_ptr() % 16 == 0
        out[name] = (data.tobytes(), d, stream_bytes)
    return out


class Buffers:
    """output, size table and scratch of one plan, each in the middle of sentinels.  `shift`: d_out that many bytes off the 16-byte grid;
    `room`: another plan whose buffers these must hold as well"""

    def __init__(self, torch, rrt, n, stream_bytes, shift=0, room=None):
        self.plan = rrt.deflate_plan(n, stream_bytes)
        self.torch = torch
        self.bytes = (self.plan["out_bound"], 4 * self.plan["streams"], self.plan["scratch_bytes"])
        if room is not None:
            self.bytes = tuple(max(a, b) for a, b in zip(self.bytes, Buffers(torch, rrt, *room).bytes))
        self.bufs = [torch.empty(GUARD + b + GUARD + 16, dtype=torch.uint8, device="cuda") for b in self.bytes]
        self.at = [(-b.data_ptr()) % 16 + GUARD for b in self.bufs]      # 16-byte aligned starts
        self.at[0] += shift
        self.host = None

    def fill(self):
        for b in self.bufs:
            b.fill_(SENTINEL)
        self.host = None

    def views(self):
        return [b[a:] for b, a in zip(self.bufs, self.at)]

    def read(self, streams=None):
        """(streams, sizes) after checking that nothing outside the three buffers, nothing of d_out beyond the total and nothing of the
        size table beyond its `streams` entries (default: the plan's) was written: there the bytes are what they were before this
        launch -- the sentinel after a fill, an earlier launch's bytes otherwise"""
        self.torch.cuda.synchronize()
        before, host = self.host, [b.cpu().numpy() for b in self.bufs]
        self.host = host
        for h, a, n in zip(host, self.at, self.bytes):
            assert (h[:a] == SENTINEL).all() and (h[a + n:] == SENTINEL).all()
        streams = self.plan["streams"] if streams is None else streams
        table = host[1][self.at[1]:self.at[1] + self.bytes[1]]
        sizes = table[:4 * streams].view(np.uint32)
        total = int(sizes.sum())
        out = host[0][self.at[0]:self.at[0] + self.bytes[0]]
        assert total <= self.bytes[0]
        if before is None:
            assert (out[total:] == SENTINEL).all() and (table[4 * streams:] == SENTINEL).all()
        else:
            assert np.array_equal(out[total:], before[0][self.at[0] + total:self.at[0] + self.bytes[0]])
            assert np.array_equal(table[4 * streams:], before[1][self.at[1] + 4 * streams:self.at[1] + self.bytes[1]])
        ends = np.cumsum(sizes.astype(np.int64))
        return [out[e - s:e].tobytes() for s, e in zip(sizes.tolist(), ends.tolist())], sizes


def _launch(torch, rrt, d_src, n, stream_bytes, finish):
    b = Buffers(torch, rrt, n, stream_bytes)
    b.fill()
    out, sizes, scratch = b.views()
    rrt.launch_deflate(out, sizes, scratch, d_src, n, stream_bytes, finish)
    return b, b.read()


@pytest.mark.parametrize("finish", (1, 0))
def test_launch_equals_the_host_entry_point_and_the_restatement(finish, cases):
    import torch
    import relativisticraytracer_amd as rrt
    seen = {"stored": 0, "dynamic": 0, "empty": 0}
    for name, (data, d_src, stream_bytes) in cases.items():
        info = []
        want = dr.deflate(data, stream_bytes, finish, info)
        for note in info:
            seen["empty" if note["m"] == 0 else "stored" if note["stored"] else "dynamic"] += 1
        b, (got, sizes) = _launch(torch, rrt, d_src, len(data), stream_bytes, finish)
        assert sizes.tolist() == [len(s) for s in want], name
        bad = [j for j, (x, y) in enumerate(zip(got, want)) if x != y]
        assert not bad, (name, bad[:4], next(i for i, (x, y) in enumerate(zip(got[bad[0]], want[bad[0]])) if x != y))
        assert got == rrt.deflate_host(data, stream_bytes, finish), name
        b.fill()                                                    # a second launch into the same buffers: nothing is accumulated
        out, tab, scratch = b.views()
        rrt.launch_deflate(out, tab, scratch, d_src, len(data), stream_bytes, finish)
        again, sizes_again = b.read()
        assert again == got and np.array_equal(sizes_again, sizes), name
    assert min(seen.values()) > 0, seen


def test_an_input_off_the_16_byte_grid_gives_the_same_bytes(cases):
    """d_src 1 ... 15 bytes off the grid: the 16-byte loads align down, the buffer's ends go byte by byte"""
    import torch
    import relativisticraytracer_amd as rrt
    for name in ("runs across chunk boundaries", "n=32769", "stride 403", "n=3"):
        data, d_src, stream_bytes = cases[name]
        want = dr.deflate(data, stream_bytes, 1)
        holder = torch.full((len(data) + 48,), SENTINEL, dtype=torch.uint8, device="cuda")
        for shift in range(1, 16):
            at = (-holder.data_ptr()) % 16 + shift
            moved = holder[at:at + len(data)]
            moved.copy_(d_src[:len(data)])
            assert moved.data_ptr() % 16 == shift
            geometry = rrt.deflate_launch_geometry(len(data), stream_bytes, moved.data_ptr())
            assert geometry["head_bytes"] > 0                                 # the byte path is taken
            _, (got, _) = _launch(torch, rrt, moved, len(data), stream_bytes, 1)
            assert got == want, (name, shift)


def test_a_captured_launch_replays_the_same_bytes(cases):
    import torch
    import relativisticraytracer_amd as rrt
    data, d_src, stream_bytes = cases["n=65541"]
    want = dr.deflate(data, stream_bytes, 1)
    b = Buffers(torch, rrt, len(data), stream_bytes)
    out, tab, scratch = b.views()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_deflate(out, tab, scratch, d_src, len(data), stream_bytes, 1)
    for _ in range(2):
        b.fill()
        graph.replay()
        got, _ = b.read()
        assert got == want


def test_raw_addresses_and_a_side_stream(cases):
    import torch
    import relativisticraytracer_amd as rrt
    data, d_src, stream_bytes = cases["png 131x40 depth 8 adaptive"]
    b = Buffers(torch, rrt, len(data), stream_bytes)
    b.fill()
    out, tab, scratch = b.views()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rrt.launch_deflate(out.data_ptr(), tab.data_ptr(), scratch.data_ptr(), d_src.data_ptr(), len(data), stream_bytes, True, stream=s)
    s.synchronize()
    assert b.read()[0] == dr.deflate(data, stream_bytes, 1)


# ---- the large fixtures (tests/deflate_ref.py: large_fixtures; tests/test_deflate_geometry.py keeps them on their branches): full-size
# segments by the hundred, three rounds of deflate_offsets and more, streams of several segments with a short last one, more
# workgroups of deflate_segments than the chip holds at once

@pytest.fixture(scope="module")
def large():
    """{name: (bytes, device tensor holding them 16-byte aligned, stream_bytes)}, uploaded once and left unchanged"""
    import torch
    out = {}
    for name, (data, stream_bytes) in dr.large_fixtures().items():
        d = torch.from_numpy(np.ascontiguousarray(data)).cuda()
        assert d.data_ptr() % 16 == 0
        out[name] = (data.tobytes(), d, stream_bytes)
    return out


_host_streams = {}


def _host(rrt, name, data, stream_bytes, finish):
    """rrt.deflate_host's streams of a large fixture, made once"""
    if (name, finish) not in _host_streams:
        _host_streams[(name, finish)] = rrt.deflate_host(data, stream_bytes, finish)
    return _host_streams[(name, finish)]


def _check(got, sizes, name, data, stream_bytes, finish, rrt=None, note=None):
    """streams and sizes against the restatement (and the host entry point): on a mismatch the first differing (stream, segment, byte)"""
    want = dr.deflate(data, stream_bytes, finish)
    where = (name, finish, note)
    assert len(got) == len(want), where
    assert sizes.tolist() == [len(s) for s in want], where + (dr.first_difference(got, data, stream_bytes, finish),)
    assert got == want, where + (dr.first_difference(got, data, stream_bytes, finish),)
    if rrt is not None:
        assert got == _host(rrt, name, data, stream_bytes, finish), where


@pytest.mark.parametrize("finish", (1, 0))
@pytest.mark.parametrize("name", dr.LARGE_NAMES)
def test_large_launch_equals_the_host_entry_point_and_the_restatement(name, finish, large):
    import torch
    import relativisticraytracer_amd as rrt
    data, d_src, stream_bytes = large[name]
    _, (got, sizes) = _launch(torch, rrt, d_src, len(data), stream_bytes, finish)
    _check(got, sizes, name, data, stream_bytes, finish, rrt)


def test_scratch_that_another_launch_left_behind(large):
    """`two per stream`, then `three per stream`, then `two per stream` again into the same output, size table and scratch, nothing
    refilled in between: another table size, other slots, other lengths.  The header calls the scratch's contents meaningless."""
    import torch
    import relativisticraytracer_amd as rrt
    two, three = large["two per stream"], large["three per stream"]
    b = Buffers(torch, rrt, len(two[0]), two[2], room=(len(three[0]), three[2]))
    b.fill()
    out, tab, scratch = b.views()
    for k, name in enumerate(("two per stream", "three per stream", "two per stream")):
        data, d_src, stream_bytes = large[name]
        rrt.launch_deflate(out, tab, scratch, d_src, len(data), stream_bytes, 1)
        got, sizes = b.read(streams=len(dr.cuts(len(data), stream_bytes)))
        _check(got, sizes, name, data, stream_bytes, 1, note=f"launch {k}")


@pytest.mark.parametrize("shift", (1, 7, 8, 15))
@pytest.mark.parametrize("name", ("frame cut", "full segment stored"))
def test_an_output_off_the_16_byte_grid_gives_the_same_bytes(name, shift, large):
    """d_out as a raw address 1 ... 15 bytes behind an aligned one: fragment 0's first destination word is cut too, and the sentinels
    in front of d_out stay (Buffers.read).  The header asks alignment of the scratch alone."""
    import torch
    import relativisticraytracer_amd as rrt
    data, d_src, stream_bytes = large[name]
    b = Buffers(torch, rrt, len(data), stream_bytes, shift=shift)
    b.fill()
    out, tab, scratch = b.views()
    assert out.data_ptr() % 16 == shift and scratch.data_ptr() % 16 == 0
    rrt.launch_deflate(out.data_ptr(), tab.data_ptr(), scratch.data_ptr(), d_src.data_ptr(), len(data), stream_bytes, True)
    got, sizes = b.read()
    _check(got, sizes, name, data, stream_bytes, 1, note=shift)


def test_a_large_input_off_the_16_byte_grid_gives_the_same_bytes(large):
    """`frame cut` 1 and 15 bytes off the grid: its streams start off the grid anyway, so hundreds of workgroups stage shifted segments"""
    import torch
    import relativisticraytracer_amd as rrt
    data, d_src, stream_bytes = large["frame cut"]
    holder = torch.full((len(data) + 48,), SENTINEL, dtype=torch.uint8, device="cuda")
    for shift in (1, 15):
        at = (-holder.data_ptr()) % 16 + shift
        moved = holder[at:at + len(data)]
        moved.copy_(d_src)
        assert moved.data_ptr() % 16 == shift
        geometry = rrt.deflate_launch_geometry(len(data), stream_bytes, moved.data_ptr())
        assert geometry["head_bytes"] == 16 - shift
        _, (got, sizes) = _launch(torch, rrt, moved, len(data), stream_bytes, 1)
        _check(got, sizes, "frame cut", data, stream_bytes, 1, note=shift)


def test_a_captured_large_launch_replays_the_same_bytes(large):
    import torch
    import relativisticraytracer_amd as rrt
    data, d_src, stream_bytes = large["frame cut"]
    b = Buffers(torch, rrt, len(data), stream_bytes)
    out, tab, scratch = b.views()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_deflate(out, tab, scratch, d_src, len(data), stream_bytes, 1)
    for replay in range(2):
        b.fill()
        graph.replay()
        got, sizes = b.read()
        _check(got, sizes, "frame cut", data, stream_bytes, 1, note=f"replay {replay}")


# ---- the drivers

W, H, FRAMES = 64, 48, 2
BASE = ["--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--spin", "0.9", "--path", "0", "--no-noise-table"]


def _drive(driver, args, base=None):
    if driver == "cpp":
        from relativisticraytracer_amd import build
        cmd = [build.build_headless()]
    else:
        cmd = [sys.executable, "-m", "relativisticraytracer_amd.headless"]
    r = subprocess.run(cmd + (BASE if base is None else base) + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def driver_files(tmp_path_factory):
    """both drivers at depth 8 and at depth 16 (--exposure 1), once with --png-deflate host and once with device:
    {(driver, depth, where): (directory, summary line)}"""
    out = {}
    for driver in ("py", "cpp"):
        for depth in (8, 16):
            for where in ("host", "device"):
                d = tmp_path_factory.mktemp(f"{driver}{depth}{where}")
                extra = ["--png-depth", "16", "--exposure", "1"] if depth == 16 else []
                line = _drive(driver, ["--png", str(d / "f.%04d.png"), "--png-deflate", where] + extra)
                assert sorted(os.listdir(d)) == ["f.0001.png", "f.0002.png"]
                out[(driver, depth, where)] = (d, line)
    return out


@pytest.mark.parametrize("depth", (8, 16))
@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_device_files_hold_the_host_files_frames(driver, depth, driver_files):
    (dev_dir, dev_line), (host_dir, host_line) = driver_files[(driver, depth, "device")], driver_files[(driver, depth, "host")]
    assert sorted(dev_line) == sorted(host_line)                                    # the summary line's fields are unchanged
    for key in ("frames", "width", "height", "n_gpus"):
        assert dev_line[key] == host_line[key], key
    frames = []
    for k in range(1, FRAMES + 1):
        a, b = (dev_dir / f"f.{k:04d}.png").read_bytes(), (host_dir / f"f.{k:04d}.png").read_bytes()
        back, ref = pr.read_file(a), pr.read_file(b)
        assert (back["width"], back["height"], back["depth"]) == (W, H, depth)
        assert back["chunks"] == ref["chunks"]
        assert np.array_equal(back["samples"], ref["samples"]) and np.array_equal(back["types"], ref["types"]), (driver, depth, k)
        assert a != b                                                               # another deflate made them
        frames.append(back["samples"])
    assert not np.array_equal(frames[0], frames[1])                                 # the camera moves: a stale frame would show


def test_both_drivers_device_files_are_the_same_bytes(driver_files):
    """the payloads are equal (tests/test_gpu_png.py) and the definition has no freedom left"""
    for depth in (8, 16):
        for k in range(1, FRAMES + 1):
            a = (driver_files[("py", depth, "device")][0] / f"f.{k:04d}.png").read_bytes()
            b = (driver_files[("cpp", depth, "device")][0] / f"f.{k:04d}.png").read_bytes()
            assert a == b, (depth, k)


# ---- the drivers at a frame of several slices, with more frames than slots: a frame of 768x480 is cut into two slices at depth 8 and
# three at depth 16, each of several segments, and seven frames are more than twice rrt_headless' three slots -- every slot is
# delivered inside the frame loop and its device buffers (streams, scratch, sizes and row sums) are used again, one of them twice

BIG_W, BIG_H, BIG_FRAMES = 768, 480, 7
BIG_BASE = ["--width", str(BIG_W), "--height", str(BIG_H), "--frames", str(BIG_FRAMES), "--spin", "0.9", "--path", "0", "--no-noise-table"]
BIG_NAMES = [f"f.{k:04d}.png" for k in range(1, BIG_FRAMES + 1)]


@pytest.fixture(scope="module")
def big_driver_files(tmp_path_factory):
    """{(driver, depth, where): directory}; where: host | device, and for the C++ driver at depth 8 `device, one in flight`"""
    out = {}
    runs = [(driver, depth, where, []) for driver in ("py", "cpp") for depth in (8, 16) for where in ("host", "device")]
    runs.append(("cpp", 8, "device, one in flight", ["--frames-in-flight", "1"]))
    for driver, depth, where, more in runs:
        d = tmp_path_factory.mktemp(f"big{driver}{depth}{where.replace(', ', '').replace(' ', '')}")
        extra = ["--png-depth", "16", "--exposure", "1"] if depth == 16 else []
        line = _drive(driver, ["--png", str(d / "f.%04d.png"), "--png-deflate", where.split(",")[0]] + extra + more, BIG_BASE)
        assert line["frames"] == BIG_FRAMES and sorted(os.listdir(d)) == BIG_NAMES
        out[(driver, depth, where)] = d
    return out


def _chunks(data):
    """([type, ...], [the contents of every IDAT]) of a PNG file, every CRC checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, kinds, idat = 8, [], []
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        kinds.append(kind.decode())
        if kind == b"IDAT":
            idat.append(body)
        at += 12 + n
    assert at == len(data)
    return kinds, idat


@pytest.mark.parametrize("depth", (8, 16))
@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_device_files_of_several_slices_over_reused_slots(driver, depth, big_driver_files):
    """every frame: the device file has the host file's chunk list (an IDAT per slice) and its payload -- samples and filter types --,
    and its IDATs hold exactly rrt.deflate_host's streams of that payload (frames 1, 4 and 7: the restatement's too)"""
    import relativisticraytracer_amd as rrt
    fmt = rrt.PngFormat(depth, "adaptive")
    n, stride, _ = rrt.png_frame_bytes(fmt, BIG_W, BIG_H, layout=True)
    rows, slices = rrt.png_slices(fmt, BIG_W, BIG_H)
    plan = rrt.deflate_plan(n, rows * stride)
    assert slices > 1 and plan["streams"] == slices and plan["segments"] > 2 * slices      # slices of several segments, the last one short
    assert plan["segments"] % -(-rows * stride // dr.SEGMENT) != 0
    dev_dir, host_dir = big_driver_files[(driver, depth, "device")], big_driver_files[(driver, depth, "host")]
    frames = []
    for k, name in enumerate(BIG_NAMES, 1):
        a, b = (dev_dir / name).read_bytes(), (host_dir / name).read_bytes()
        (kinds, idat), (host_kinds, host_idat) = _chunks(a), _chunks(b)
        assert kinds == host_kinds == ["IHDR", "sRGB", "tEXt"] + ["IDAT"] * slices + ["IEND"], (driver, depth, k)
        assert a[:a.index(b"IDAT") - 4] == b[:b.index(b"IDAT") - 4] and a != b             # the same header; another deflate made the rest
        joined = b"".join(host_idat)
        assert joined[:2] == b"\x78\x01"
        z = zlib.decompressobj(-15)
        payload = z.decompress(joined[2:-4])
        assert z.eof and len(payload) == n and joined[-4:] == struct.pack(">I", zlib.adler32(payload))
        assert zlib.decompress(b"".join(idat)) == payload, (driver, depth, k)       # the same samples and filter types
        streams = list(idat)
        assert streams[0][:2] == b"\x78\x01" and streams[-1][-4:] == joined[-4:]
        streams[0] = streams[0][2:]
        streams[-1] = streams[-1][:-4]
        assert streams == rrt.deflate_host(payload, rows * stride, True), (driver, depth, k, dr.first_difference(streams, payload, rows * stride, 1))
        if k in (1, 4, 7):
            assert streams == dr.deflate(payload, rows * stride, 1), (driver, depth, k, dr.first_difference(streams, payload, rows * stride, 1))
        frames.append(rrt.png_unfilter_host(payload, fmt, BIG_W, BIG_H))
    for i in range(BIG_FRAMES):                                                     # the camera moves: a stale or swapped slot would show
        for j in range(i):
            assert not np.array_equal(frames[i], frames[j]), (driver, depth, i + 1, j + 1)


def test_both_drivers_device_files_of_several_slices_are_the_same_bytes(big_driver_files):
    for depth in (8, 16):
        for name in BIG_NAMES:
            assert (big_driver_files[("py", depth, "device")] / name).read_bytes() == (big_driver_files[("cpp", depth, "device")] / name).read_bytes(), (depth, name)


def test_one_frame_in_flight_writes_the_same_files(big_driver_files):
    """rrt_headless with one slot, used seven times, against its three"""
    for name in BIG_NAMES:
        assert (big_driver_files[("cpp", 8, "device, one in flight")] / name).read_bytes() == (big_driver_files[("cpp", 8, "device")] / name).read_bytes(), name
