"""EXR output on the device: rrt_launch_exr_from_hdr against the host entry point and the numpy restatement (tests/exr_ref.py) byte
for byte -- every type and compression at sizes of both launch paths, off the 16-byte grid and where the grid's rows wrap; the half
conversion's input list through the kernel; a rendered frame through launch, sink and the restatement's reader; and both headless
drivers' --exr files against the HDR the driver's own passes leave."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exr_ref as xr

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32
SENTINEL, BEFORE, AFTER = 0xA5, 32, 64


@pytest.fixture(scope="module")
def inputs():
    """one HDR frame per size, shared by the formats and left unchanged, on the host and on the device: {(w, h): (hdr, d_hdr)}"""
    import torch
    rng = np.random.default_rng(2024)
    out = {}
    for w, h, _ in xr.GPU_CASES:
        if (w, h) not in out:
            hdr = xr.hdr_frame(rng, w, h)
            out[(w, h)] = (hdr, torch.from_numpy(hdr).cuda())
    return out


def _launch_checked(torch, rrt, d_hdr, w, h, f, n, shift=0):
    """the launch into the middle of a larger buffer of sentinels, `shift` bytes off the 16-byte grid; returns the payload after
    checking the guard bytes on both sides"""
    buf = torch.full((BEFORE + n + AFTER + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + BEFORE + shift
    assert rrt.exr_launch_geometry(f, w, h, (buf.data_ptr() + start) | d_hdr.data_ptr())["wide"] == (w % 8 == 0 and shift % 16 == 0)
    rrt.launch_exr_from_hdr(buf[start:], d_hdr, w, h, f)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:start] == SENTINEL).all() and (got[start + n:] == SENTINEL).all(), (w, h, shift)
    return got[start:start + n]


@pytest.mark.parametrize("fmt", xr.FORMATS, ids="-".join)
def test_launch_equals_the_host_entry_point_and_the_restatement(fmt, inputs):
    import torch
    import relativisticraytracer_amd as rrt
    f = rrt.ExrFormat(*fmt)
    paths = set()
    for w, h, shift in xr.GPU_CASES:
        hdr, d_hdr = inputs[(w, h)]
        g = rrt.exr_launch_geometry(f, w, h, shift)
        paths.add((g["wide"], g["passes"] > 1))
        n = rrt.exr_frame_bytes(f, w, h)
        want = xr.payload(hdr, fmt)
        assert want.size == n
        got = _launch_checked(torch, rrt, d_hdr, w, h, f, n, shift)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (w, h, shift, bad.size, bad[:8].tolist())
        assert np.array_equal(rrt.exr_from_hdr_host(hdr, f), want), (w, h)
        again = _launch_checked(torch, rrt, d_hdr, w, h, f, n, shift)          # nothing is accumulated: a second launch, the same bytes
        assert np.array_equal(again, got), (w, h, shift)
        assert np.array_equal(d_hdr.cpu().numpy().view(np.uint32), hdr.view(np.uint32))      # the input is only read
    assert paths == {(True, False), (False, False), (True, True)}


@pytest.mark.parametrize("half_max", [65504.0, 1024.0])
def test_the_conversion_input_list_through_the_kernels(half_max):
    """every input the half conversion is pinned on (tests/exr_ref.py: conversion_inputs), laid out as a frame, through the wide
    kernel -- plain and filtered -- and, off the 16-byte grid, through the narrow one"""
    import torch
    import relativisticraytracer_amd as rrt
    w = 256
    frame = xr.frame_of(xr.conversion_inputs(), w)
    h = frame.shape[0]
    d = torch.from_numpy(frame).cuda()
    src = np.ascontiguousarray(frame[::-1, :, 2::-1].transpose(0, 2, 1))
    for compression, shift in (("none", 0), ("zip", 0), ("none", 2), ("zips", 6)):
        f = rrt.ExrFormat("half", compression, half_max)
        fmt = ("half", compression, half_max)
        n = rrt.exr_frame_bytes(f, w, h)
        got = _launch_checked(torch, rrt, d, w, h, f, n, shift)
        assert np.array_equal(got, xr.payload(frame, fmt)), (compression, shift)
        assert np.array_equal(got, rrt.exr_from_hdr_host(frame, f)), (compression, shift)
        if compression == "none":       # and against numpy's own conversion, apart from the clamp
            bits = got.view("<u2").reshape(h, 3, w)
            with np.errstate(over="ignore"):
                rounded = src.astype(np.float16)
            plain = np.isfinite(src) & (np.abs(rounded.astype(np.float64)) <= half_max)
            assert np.array_equal(bits[plain], rounded[plain].view(np.uint16))
            assert not np.any((bits & 0x7C00) == 0x7C00) and np.all(bits[np.isnan(src)] == 0)
    g = torch.from_numpy(frame).cuda()
    f = rrt.ExrFormat("float", "zip")
    got = _launch_checked(torch, rrt, g, w, h, f, rrt.exr_frame_bytes(f, w, h))
    assert np.array_equal(got, xr.payload(frame, ("float", "zip")))      # NaNs and infs pass through a float file as they are


def test_raw_addresses_and_a_side_stream(inputs):
    import torch
    import relativisticraytracer_amd as rrt
    w, h = 72, 33
    hdr, d_hdr = inputs[(w, h)]
    out = torch.zeros(rrt.exr_frame_bytes(None, w, h), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rrt.launch_exr_from_hdr(out.data_ptr(), d_hdr.data_ptr(), w, h, None, stream=s)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), xr.payload(hdr, ("half", "zip")))


def _half_channels(hdr):
    s = xr.samples(hdr, "half")
    return {"B": s[:, 0], "G": s[:, 1], "R": s[:, 2]}


def test_a_rendered_frame_into_a_file_and_back(sky, tmp_path):
    """64 x 48 at a = 0.9 with volumetrics through launch_raymarch_ss(..., hdr=H) -> launch_exr_from_hdr -> EXRSink -> the
    restatement's reader: the file holds the half-rounded HDR the launch returned"""
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import sinks
    w, h = 64, 48
    tex = rrt.SkyTexture(sky)
    B = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    H = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    rrt.launch_raymarch_ss(B, w, h, 1, 1.0, rrt.CameraState.default(), tex, rrt.CameraEffects(), rrt.RenderParams(spin=0.9, volumetrics=1), hdr=H)
    torch.cuda.synchronize()
    lin = H.cpu().numpy().reshape(h, w, 4)
    assert len(np.unique(lin[..., :3])) > 500 and np.isfinite(lin).all()         # a picture, not a flat frame
    want = _half_channels(lin)
    for fmt in (("half", "zip"), ("half", "none"), ("float", "zips")):
        f = rrt.ExrFormat(*fmt)
        out = torch.zeros(rrt.exr_frame_bytes(f, w, h), dtype=torch.uint8, device="cuda")
        rrt.launch_exr_from_hdr(out, H, w, h, f)
        payload = out.cpu().numpy()
        assert np.array_equal(payload, xr.payload(lin, fmt)), fmt
        path = tmp_path / ("%s_%s.exr" % fmt)
        sink = sinks.EXRSink(str(path), w, h, 24, f)
        sink.write(payload)
        sink.close()
        data = path.read_bytes()
        assert data == xr.write_file(lin, fmt)
        back = xr.read_file(data)
        assert (back["width"], back["height"], back["type"], back["compression"]) == (w, h) + fmt
        for k, c in enumerate("RGB"):
            if fmt[0] == "half":
                assert np.array_equal(back["channels"][c].view(np.uint16), want[c]), (fmt, c)
            else:
                assert np.array_equal(back["channels"][c].view(np.uint32), lin[::-1, :, k].view(np.uint32)), (fmt, c)
        if fmt[1] != "none":
            assert len(data) < len(xr.header(fmt, w, h)) + 8 * 48 + rrt.exr_frame_bytes(f, w, h)       # deflate shrank it
    tex.destroy()


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
def exposed_hdr():
    """the HDR the drivers' own passes leave for `--auto-exposure` (and without it), frame by frame: headless.py's Renderer, in this
    process -- the launches, the sequence's exposure state and the camera path the driver runs"""
    import torch
    from relativisticraytracer_amd import headless

    def frames(extra):
        ap = headless.build_parser()
        args = ap.parse_args(BASE + ["--exr", "unused.%04d.exr"] + extra)
        pano, use_exposure, dof_k = headless.check_args(ap, args, 1)
        r = headless.Renderer(args, headless.build_settings(ap, args, pano, use_exposure), dof_k, 0, 1, torch.device("cuda", 0))
        out = []
        for k in range(1, FRAMES + 1):
            r.set_frame(k, lambda t: 0)
            r.render_post()
            torch.cuda.synchronize()
            out.append(r.hdr.cpu().numpy().reshape(H, W, 4).copy())
        r.close()
        return out
    return {"exposed": frames(["--auto-exposure"]), "plain": frames([])}


@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_files_hold_the_post_exposure_hdr(driver, exposed_hdr, tmp_path):
    """--frames 2 --exr f.%04d.exr --auto-exposure: two files, each the half-rounded HDR as the exposure pass left it"""
    _drive(driver, ["--exr", str(tmp_path / "f.%04d.exr"), "--auto-exposure"])
    assert sorted(os.listdir(tmp_path)) == ["f.0001.exr", "f.0002.exr"]
    frames = exposed_hdr["exposed"]
    assert not np.array_equal(frames[0], frames[1])                               # the camera moves: a stale frame would show
    assert not np.array_equal(frames[0], exposed_hdr["plain"][0])                 # ... and the exposure scaled the frame
    for k, lin in enumerate(frames, 1):
        data = (tmp_path / f"f.{k:04d}.exr").read_bytes()
        back = xr.read_file(data)
        assert (back["width"], back["height"], back["type"], back["compression"]) == (W, H, "half", "zip")
        want = _half_channels(lin)
        for c in "RGB":
            assert np.array_equal(back["channels"][c].view(np.uint16), want[c]), (driver, k, c)
        assert data == xr.write_file(lin, ("half", "zip"))                        # both drivers deflate alike, at level 4


@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_float_files_next_to_out(driver, exposed_hdr, tmp_path):
    """--exr next to --out, float, one scanline per chunk, no exposure: the files hold the launch's HDR bit for bit"""
    _drive(driver, ["--exr", str(tmp_path / "g.%d.exr"), "--exr-type", "float", "--exr-compression", "zips", "--exr-level", "6",
                    "--out", str(tmp_path / "g.rgba")])
    assert sorted(os.listdir(tmp_path)) == ["g.1.exr", "g.2.exr", "g.rgba"]
    assert os.path.getsize(tmp_path / "g.rgba") == FRAMES * W * H * 4
    for k, lin in enumerate(exposed_hdr["plain"], 1):
        data = (tmp_path / f"g.{k}.exr").read_bytes()
        assert data == xr.write_file(lin, ("float", "zips"), 24, 6)
        back = xr.read_file(data)
        for j, c in enumerate("RGB"):
            assert np.array_equal(back["channels"][c].view(np.uint32), lin[::-1, :, j].view(np.uint32)), (driver, k, c)
