"""PNG output on the device: rrt_launch_png_from_rgba8 / _from_hdr against the host entry points and the numpy restatement
(tests/png_ref.py), payload byte for byte and row sums word for word -- both inputs, all six filter settings, at the smallest frames
that can go wrong (png_ref.gpu_sizes; tests/test_png_geometry.py keeps them on their branches), with guard bytes behind both outputs,
off the 16-byte grid (the narrow path) and launched twice; and both headless drivers' --png files against the frames they hold."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import png_ref as pr

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SENTINEL, BEFORE, AFTER = 0xA5, 32, 64
DEPTHS = (8, 16)


@pytest.fixture(scope="module")
def po():
    from oracle import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def inputs(po):
    """one frame per depth and size, shared by the filters and left unchanged, on the host and on the device, with its raw
    scanlines: {(depth, name): (w, h, frame, tensor, raw)}"""
    import torch
    import relativisticraytracer_amd as rrt
    wide, narrow = rrt.png_launch_geometry(None, 64, 64), rrt.png_launch_geometry(None, 64, 64, 1)
    rng = np.random.default_rng(2025)
    out = {}
    for name, (w, h) in pr.gpu_sizes(wide["rows"], wide["threads"], narrow["threads"]).items():
        f8, f16 = pr.rgba8_frame(rng, w, h), pr.hdr_frame(rng, w, h)
        out[(8, name)] = (w, h, f8, torch.from_numpy(f8).cuda(), pr.raw_from_rgba8(f8))
        out[(16, name)] = (w, h, f16, torch.from_numpy(f16).cuda(), pr.raw_from_hdr(po, f16))
    return out


def _guarded(torch, n, shift):
    """a buffer of sentinels and the start, `shift` bytes off the 16-byte grid, of the n bytes a launch may write"""
    buf = torch.full((BEFORE + n + AFTER + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    return buf, (-buf.data_ptr()) % 16 + BEFORE + shift


def _launch_checked(torch, rrt, depth, d_src, w, h, f, shift=0, expect_wide=None):
    """the launch into the middle of larger buffers of sentinels; returns payload and sums after checking the guard bytes"""
    n, _, table = rrt.png_frame_bytes(f, w, h, layout=True)
    buf, start = _guarded(torch, n, shift)
    tab, t0 = _guarded(torch, table, 0)
    geometry = rrt.png_launch_geometry(f, w, h, (buf.data_ptr() + start) | d_src.data_ptr())
    if expect_wide is not None:
        assert geometry["wide"] == expect_wide
    launch = rrt.launch_png_from_rgba8 if depth == 8 else rrt.launch_png_from_hdr
    launch(buf[start:], tab[t0:], d_src, w, h, f)
    torch.cuda.synchronize()
    got, sums = buf.cpu().numpy(), tab.cpu().numpy()
    assert (got[:start] == SENTINEL).all() and (got[start + n:] == SENTINEL).all(), (w, h, shift)
    assert (sums[:t0] == SENTINEL).all() and (sums[t0 + table:] == SENTINEL).all(), (w, h, shift)
    return got[start:start + n], sums[t0:t0 + table].view(np.uint32)


@pytest.mark.parametrize("filter_name", pr.FILTERS)
@pytest.mark.parametrize("depth", DEPTHS)
def test_launch_equals_the_host_entry_point_and_the_restatement(depth, filter_name, inputs):
    import torch
    import relativisticraytracer_amd as rrt
    f = rrt.PngFormat(depth, filter_name)
    host = rrt.png_from_rgba8_host if depth == 8 else rrt.png_from_hdr_host
    seen = set()
    for (d, name), (w, h, frame, tensor, raw) in inputs.items():
        if d != depth:
            continue
        want, types, want_sums = pr.payload(raw, f.bpp, filter_name)
        seen |= set(types.tolist())
        got, sums = _launch_checked(torch, rrt, depth, tensor, w, h, f, 0, True)
        bad = np.flatnonzero(got != want.ravel())
        assert bad.size == 0, (name, bad.size, bad[:8].tolist(), types.tolist())
        assert np.array_equal(sums.reshape(h, 2), want_sums), name
        host_pay, host_sums = host(frame, f)
        assert np.array_equal(host_pay, got) and np.array_equal(host_sums, sums), name
        again, sums_again = _launch_checked(torch, rrt, depth, tensor, w, h, f, 0, True)      # nothing is accumulated
        assert np.array_equal(again, got) and np.array_equal(sums_again, sums), name
    assert seen == ({0, 1, 2, 3, 4} if filter_name == "adaptive" else {pr.FILTERS.index(filter_name)})


@pytest.mark.parametrize("filter_name", ("adaptive", "paeth"))
@pytest.mark.parametrize("depth", DEPTHS)
def test_off_the_16_byte_grid_the_narrow_path_writes_the_same_bytes(depth, filter_name, inputs):
    """a payload 1 ... 15 bytes off the grid, and an input 4 bytes off it"""
    import torch
    import relativisticraytracer_amd as rrt
    f = rrt.PngFormat(depth, filter_name)
    shift = 0
    for name in pr.NARROW_SIZES:
        w, h, frame, tensor, raw = inputs[(depth, name)]
        want, _, want_sums = pr.payload(raw, f.bpp, filter_name)
        for _ in range(3):
            shift = shift % 15 + 1
            got, sums = _launch_checked(torch, rrt, depth, tensor, w, h, f, shift, False)
            assert np.array_equal(got, want.ravel()) and np.array_equal(sums.reshape(h, 2), want_sums), (name, shift)
    assert shift == 6            # 21 launches: every shift 1 ... 15 was used
    w, h, frame, tensor, raw = inputs[(depth, "two bands plus a row")]
    want, _, want_sums = pr.payload(raw, f.bpp, filter_name)
    flat = tensor.reshape(-1)
    holder = torch.zeros(flat.numel() + 16, dtype=flat.dtype, device="cuda")
    at = ((-holder.data_ptr()) % 16 + 4) // flat.element_size()
    moved = holder[at:at + flat.numel()]
    moved.copy_(flat)
    assert moved.data_ptr() % 16 == 4
    got, sums = _launch_checked(torch, rrt, depth, moved, w, h, f, 0, False)
    assert np.array_equal(got, want.ravel()) and np.array_equal(sums.reshape(h, 2), want_sums)


def test_raw_addresses_and_a_side_stream(inputs):
    import torch
    import relativisticraytracer_amd as rrt
    w, h, frame, tensor, raw = inputs[(8, "two bands plus a row")]
    out = torch.zeros(rrt.png_frame_bytes(None, w, h), dtype=torch.uint8, device="cuda")
    tab = torch.zeros(2 * h, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    rrt.launch_png_from_rgba8(out.data_ptr(), tab.data_ptr(), tensor.data_ptr(), w, h, None, stream=s)
    s.synchronize()
    want, _, sums = pr.payload(raw, 3, "adaptive")
    assert np.array_equal(out.cpu().numpy(), want.ravel()) and np.array_equal(tab.cpu().numpy().view(np.uint32).reshape(h, 2), sums)


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
    """the HDR the Python driver's own passes leave for `--exposure 1`, frame by frame: headless.py's Renderer, in this process"""
    import torch
    from relativisticraytracer_amd import headless
    ap = headless.build_parser()
    args = ap.parse_args(BASE + ["--png", "unused.%04d.png", "--png-depth", "16", "--exposure", "1"])
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


@pytest.fixture(scope="module")
def driver_files(tmp_path_factory):
    """both drivers, each once at depth 8 and once at depth 16 with --exposure 1, --out next to --png: {(driver, depth): directory}"""
    out = {}
    for driver in ("py", "cpp"):
        for depth in DEPTHS:
            d = tmp_path_factory.mktemp(f"{driver}{depth}")
            extra = ["--png-depth", "16", "--exposure", "1"] if depth == 16 else ["--png-filter", "adaptive", "--png-level", "6"]
            _drive(driver, ["--out", str(d / "f.rgba"), "--png", str(d / "f.%04d.png")] + extra)
            assert sorted(os.listdir(d)) == ["f.0001.png", "f.0002.png", "f.rgba"]
            out[(driver, depth)] = d
    return out


@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_8_bit_files_hold_the_out_frames(driver, driver_files):
    d = driver_files[(driver, 8)]
    frames = np.fromfile(d / "f.rgba", np.uint8).reshape(FRAMES, H, W, 4)
    assert not np.array_equal(frames[0], frames[1])                                 # the camera moves: a stale frame would show
    for k in range(FRAMES):
        back = pr.read_file((d / f"f.{k + 1:04d}.png").read_bytes())
        assert (back["width"], back["height"], back["depth"]) == (W, H, 8)
        assert np.array_equal(back["samples"], frames[k, ::-1, :, :3]), (driver, k)
        assert len(set(back["types"].tolist())) > 1                                 # adaptive chose


@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_16_bit_files_hold_q_of_the_exposed_hdr(driver, driver_files, exposed_hdr, po):
    d = driver_files[(driver, 16)]
    for k, lin in enumerate(exposed_hdr):
        back = pr.read_file((d / f"f.{k + 1:04d}.png").read_bytes())
        assert (back["width"], back["height"], back["depth"]) == (W, H, 16)
        want = pr.q_from_hdr(po, lin)
        assert len(np.unique(want)) > 500                                           # a picture, not a flat frame
        assert np.array_equal(back["samples"], want), (driver, k)


def test_both_drivers_files_decode_to_the_same_samples(driver_files):
    for depth in DEPTHS:
        for k in range(1, FRAMES + 1):
            a = pr.read_file((driver_files[("py", depth)] / f"f.{k:04d}.png").read_bytes())
            b = pr.read_file((driver_files[("cpp", depth)] / f"f.{k:04d}.png").read_bytes())
            assert np.array_equal(a["samples"], b["samples"]) and np.array_equal(a["types"], b["types"]), (depth, k)
