"""Y4M output on the device: the two launches of include/rrt_yuv.h against the numpy restatement (tests/yuv_ref.py) byte for byte, at
sizes of both launch paths, a rendered frame through both inputs, and both headless drivers' --y4m files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import yuv_ref as yr

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32
IDS = dict(ids=lambda f: f"{f[0]}-{'full' if f[1] else 'limited'}-{f[2]}" if isinstance(f, tuple) and len(f) == 3 else None)
SENTINEL, BEFORE, AFTER = 0xA5, 16, 64


def _fmt(rrt, fmt):
    return rrt.YuvFormat(fmt[0], "full" if fmt[1] else "limited", fmt[2])


@pytest.fixture(scope="module")
def inputs():
    """one random RGBA8 frame and one HDR frame per size, shared by the formats and left unchanged: {(w, h): (rgba, hdr)}"""
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(2020)
    out = {}
    for w, h in yr.sizes(rrt.yuv_launch_geometry(None, 64, 48)):
        out[(w, h)] = (rng.integers(0, 256, (h, w, 4), dtype=np.uint8), yr.hdr_frame(rng, w, h))
    return out


@pytest.fixture(scope="module")
def hdr_q(inputs, po):
    """the HDR frames' sixteen-bit components by the oracle's tone map, once"""
    return {size: yr.q_from_hdr(po, hdr) for size, (_, hdr) in inputs.items()}


def _launch_checked(torch, launch, src, w, h, f, n):
    """the launch into the middle of a larger buffer of sentinels; returns the frame's bytes after checking both margins"""
    buf = torch.full((BEFORE + n + AFTER + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + BEFORE                  # 16-byte aligned, with at least BEFORE bytes in front
    launch(buf[start:], src, w, h, f)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[start - BEFORE:start] == SENTINEL).all() and (got[start + n:start + n + AFTER] == SENTINEL).all(), (w, h)
    return got[start:start + n]


@pytest.mark.parametrize("fmt", yr.FORMATS, **IDS)
def test_launches_equal_the_restatement(fmt, inputs, hdr_q):
    import torch
    import relativisticraytracer_amd as rrt
    f = _fmt(rrt, fmt)
    paths = set()
    for (w, h), (rgba, hdr) in inputs.items():
        paths.add(rrt.yuv_launch_geometry(f, w, h)["wide"])
        n = rrt.yuv_frame_bytes(f, w, h)
        d_rgba, d_hdr = torch.from_numpy(rgba).cuda(), torch.from_numpy(hdr).cuda()
        want8, want16 = yr.frame_from_rgba8(rgba, fmt), yr.pack(yr.planes(hdr_q[(w, h)], fmt), fmt[2])
        for launch, src, want in ((rrt.launch_yuv_from_rgba8, d_rgba, want8), (rrt.launch_yuv_from_hdr, d_hdr, want16)):
            got = _launch_checked(torch, launch, src, w, h, f, n)
            assert np.array_equal(got, want), (launch.__name__, w, h, int((got != want).sum()))
            again = _launch_checked(torch, launch, src, w, h, f, n)
            assert np.array_equal(again, got), (launch.__name__, w, h)
        assert np.array_equal(d_rgba.cpu().numpy(), rgba)                            # the inputs are only read
    assert paths == {True, False}, "the size list must hold sizes of both launch paths"


def test_raw_addresses_and_a_side_stream(inputs):
    """the launches take raw device addresses and an explicit stream: same bytes as with tensors on the current stream"""
    import torch
    import relativisticraytracer_amd as rrt
    w, h = 64, 48
    rgba, _ = inputs[(w, h)]
    d = torch.from_numpy(rgba).cuda()
    n = rrt.yuv_frame_bytes(None, w, h)
    out = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rrt.launch_yuv_from_rgba8(out.data_ptr(), d.data_ptr(), w, h, None, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), yr.frame_from_rgba8(rgba, (420, False, 8)))


def test_an_rgba8_frame_off_the_16_byte_grid_gives_the_same_bytes(inputs):
    """d_rgba8 need only be 4-byte aligned: at a size of the wide path such a frame cannot be loaded 16 bytes at a time and goes
    through the one-sample kernel -- same bytes"""
    import torch
    import relativisticraytracer_amd as rrt
    w, h = 64, 48
    assert rrt.yuv_launch_geometry(None, w, h)["wide"]
    rgba, _ = inputs[(w, h)]
    flat = torch.from_numpy(rgba).cuda().view(-1)
    for fmt in ((420, False, 8), (444, True, 10)):
        f = _fmt(rrt, fmt)
        want = yr.frame_from_rgba8(rgba, fmt)
        for shift in (4, 8, 12):
            buf = torch.zeros(flat.numel() + 32, dtype=torch.uint8, device="cuda")
            at = (-buf.data_ptr()) % 16 + shift
            buf[at:at + flat.numel()] = flat
            got = _launch_checked(torch, rrt.launch_yuv_from_rgba8, buf[at:], w, h, f, want.size)
            assert np.array_equal(got, want), (fmt, shift)


def test_a_rendered_frame_through_both_inputs(po, sky):
    """64 x 48 at a = 0.9 through launch_raymarch_ss(..., 1, ..., hdr=H): the bytes it wrote and its HDR, each through its launch,
    equal the restatement -- the library's tone map tied to the oracle's on real HDR values"""
    import torch
    import relativisticraytracer_amd as rrt
    w, h = 64, 48
    tex = rrt.SkyTexture(sky)
    B = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    H = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    rrt.launch_raymarch_ss(B, w, h, 1, 1.0, rrt.CameraState.default(), tex, rrt.CameraEffects(), rrt.RenderParams(spin=0.9), hdr=H)
    torch.cuda.synchronize()
    b, lin = B.cpu().numpy().reshape(h, w, 4), H.cpu().numpy().reshape(h, w, 4)
    assert len(np.unique(b[..., :3])) > 50                                       # a picture, not a flat frame
    q = yr.q_from_hdr(po, lin)
    for fmt in ((420, False, 8), (444, True, 10), (420, False, 10)):
        f = _fmt(rrt, fmt)
        out = torch.zeros(rrt.yuv_frame_bytes(f, w, h), dtype=torch.uint8, device="cuda")
        rrt.launch_yuv_from_rgba8(out, B, w, h, f)
        assert np.array_equal(out.cpu().numpy(), yr.frame_from_rgba8(b, fmt)), fmt
        rrt.launch_yuv_from_hdr(out, H, w, h, f)
        assert np.array_equal(out.cpu().numpy(), yr.pack(yr.planes(q, fmt), fmt[2])), fmt
    tex.destroy()


# ---- the drivers

W, H, FRAMES = 64, 48, 2
BASE = ["--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--spin", "0.9", "--path", "0"]


def _drive(driver, args):
    if driver == "cpp":
        from relativisticraytracer_amd import build
        cmd = [build.build_headless()]
    else:
        cmd = [sys.executable, "-m", "relativisticraytracer_amd.headless"]
    r = subprocess.run(cmd + BASE + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _rgba_frames(path):
    data = np.fromfile(path, np.uint8)
    assert data.size == FRAMES * H * W * 4
    return data.reshape(FRAMES, H, W, 4)


def _expected_stream(frames, fmt):
    return yr.header(fmt, W, H) + b"".join(b"FRAME\n" + yr.frame_from_rgba8(f, fmt).tobytes() for f in frames)


@pytest.fixture(scope="module", params=["py", "cpp"])
def default_run(request, tmp_path_factory):
    """one run per driver with --out and --y4m in the default format, shared by the depth-8 tests: (driver, summary, frames, y4m bytes)"""
    d = tmp_path_factory.mktemp("y4m_" + request.param)
    meta = _drive(request.param, ["--out", str(d / "f.rgba"), "--y4m", str(d / "f.y4m")])
    return request.param, meta, _rgba_frames(d / "f.rgba"), (d / "f.y4m").read_bytes()


def test_driver_depth_8(default_run):
    """the .y4m file is the header and, per frame, FRAME + the restatement's planes of that frame of the .rgba file"""
    driver, meta, frames, y4m = default_run
    assert not np.array_equal(frames[0], frames[1])                             # the camera moves: a stale frame would show
    assert y4m == _expected_stream(frames, (420, False, 8))
    assert meta["frames"] == FRAMES and (driver == "cpp" or meta["sink"].endswith("f.rgba"))


def test_driver_depth_8_444_full_range(default_run, tmp_path):
    driver = default_run[0]
    rgba, y4m = tmp_path / "g.rgba", tmp_path / "g.y4m"
    _drive(driver, ["--out", str(rgba), "--y4m", str(y4m), "--y4m-chroma", "444", "--y4m-range", "full"])
    assert y4m.read_bytes() == _expected_stream(_rgba_frames(rgba), (444, True, 8))


def test_driver_y4m_alone_writes_the_same_file(default_run, tmp_path):
    """--y4m without --out: the same file, and no RGBA sink"""
    driver, _, _, y4m = default_run
    alone = tmp_path / "alone.y4m"
    meta = _drive(driver, ["--y4m", str(alone)])
    assert alone.read_bytes() == y4m
    assert driver == "cpp" or meta["sink"] is None
    assert os.listdir(tmp_path) == ["alone.y4m"]


@pytest.mark.parametrize("extra", [[], ["--exposure", "1"]], ids=["plain", "exposure"])
@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_depth_10(driver, extra, tmp_path):
    """10-bit frames come from the frame's linear HDR (with --exposure: the scaled HDR).  A plumbing check: on every pixel
    |Y10 - 4 * Y8| <= 6 with Y8 the restatement's luma of the same run's .rgba -- q_hdr - 257 * byte lies in about [-1, 258), under
    3.5 ten-bit luma codes, and the two final roundings add up to 2.5 more.  A flipped, shifted, stale or wrong-slot frame fails it."""
    rgba, y4m = tmp_path / "f.rgba", tmp_path / "f10.y4m"
    _drive(driver, ["--out", str(rgba), "--y4m", str(y4m), "--y4m-depth", "10"] + extra)
    fmt = (420, False, 10)
    data = y4m.read_bytes()
    n, offs = yr.frame_bytes(fmt, W, H)
    assert len(data) == len(yr.header(fmt, W, H)) + FRAMES * (6 + n)
    head, got = yr.parse_y4m(data, fmt, W, H)
    assert head == yr.header(fmt, W, H) and len(got) == FRAMES
    frames = _rgba_frames(rgba)
    assert not np.array_equal(frames[0], frames[1])
    for frame, g in zip(frames, got):
        y10 = g[:offs[1]].view(np.dtype("<u2")).astype(np.int64).reshape(H, W)
        y8 = yr.planes(yr.q_from_rgba8(frame), (420, False, 8))[0]
        assert y10.max() - y10.min() > 40                                        # a picture
        worst = int(np.abs(y10 - 4 * y8).max())
        print(f"{driver} {extra}: largest |Y10 - 4 Y8| = {worst}")
        assert worst <= 6
