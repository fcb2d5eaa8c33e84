"""Device deflate on the device: rrt_launch_deflate against rrt_deflate_host and the Python restatement (tests/deflate_ref.py), stream
bytes byte for byte and stream sizes word for word, on every fixture the host tests use (tests/test_deflate_geometry.py keeps them on
their branches), with guard bytes behind the output, the size table and the scratch, off the 16-byte grid, launched twice, and
captured into a graph; and both headless drivers' --png-deflate device files against their --png-deflate host files."""
import json
import os
import subprocess
import sys

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
    """output, size table and scratch of one plan, each in the middle of sentinels"""

    def __init__(self, torch, rrt, n, stream_bytes):
        self.plan = rrt.deflate_plan(n, stream_bytes)
        self.torch = torch
        self.bytes = (self.plan["out_bound"], 4 * self.plan["streams"], self.plan["scratch_bytes"])
        self.bufs = [torch.empty(GUARD + b + GUARD + 16, dtype=torch.uint8, device="cuda") for b in self.bytes]
        self.at = [(-b.data_ptr()) % 16 + GUARD for b in self.bufs]      # 16-byte aligned starts

    def fill(self):
        for b in self.bufs:
            b.fill_(SENTINEL)

    def views(self):
        return [b[a:] for b, a in zip(self.bufs, self.at)]

    def read(self):
        """(streams, sizes) after checking that nothing outside the three buffers, and nothing of d_out beyond the total, was written"""
        self.torch.cuda.synchronize()
        host = [b.cpu().numpy() for b in self.bufs]
        for h, a, n in zip(host, self.at, self.bytes):
            assert (h[:a] == SENTINEL).all() and (h[a + n:] == SENTINEL).all()
        sizes = host[1][self.at[1]:self.at[1] + self.bytes[1]].view(np.uint32)
        total = int(sizes.sum())
        out = host[0][self.at[0]:self.at[0] + self.bytes[0]]
        assert total <= self.bytes[0] and (out[total:] == SENTINEL).all()
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


# ---- the drivers

W, H, FRAMES = 64, 48, 2
BASE = ["--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--spin", "0.9", "--path", "0", "--no-noise-table"]


def _drive(driver, args):
    if driver == "cpp":
        from relativisticraytracer_amd import build
        cmd = [build.build_headless()]
    else:
        cmd = [sys.executable, "-m", "relativisticraytracer_amd.headless"]
    r = subprocess.run(cmd + BASE + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
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
