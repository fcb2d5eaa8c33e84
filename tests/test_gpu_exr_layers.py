"""EXR data layers on the device: rrt_launch_exr_layers against the host entry point and the numpy restatement
(tests/exr_layers_ref.py) byte for byte -- five kinds of layer set at three compressions, at sizes of both launch paths, off the
16-byte grid and where the grid's rows wrap, between sentinel guards; the conversion lists through the kernels; a side stream; the
{B, G, R} set against rrt_launch_exr_from_hdr on the device; a rendered frame through launch_raymarch_debug into a layered file and
back; and both headless drivers' --exr-layers files against the debug launch's own outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import exr_layers_ref as lr
import exr_ref as xr

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32
SENTINEL, GUARD = 0xA5, 64
SETS = ("bgr_half", "all_half", "all_float", "mixed", "uint")
# (w, h, bytes the payload is moved off the 16-byte grid, the plane moved 4 bytes off it)
CASES = ([(w, h, 0, None) for w, h in lr.WIDE_CASES + lr.NARROW_CASES]
         + [lr.MOVED_CASE + (2, None), lr.MOVED_CASE + (0, "last"), lr.WRAP_CASE + (0, None)])


def _aligned(torch, a, shift=0):
    """the array on the device, 16-byte aligned, or `shift` bytes (a multiple of 4) past that"""
    flat = torch.from_numpy(np.ascontiguousarray(a)).reshape(-1)
    buf = torch.empty(flat.numel() + 8, dtype=flat.dtype, device="cuda")
    start = ((-buf.data_ptr()) % 16 + shift) // 4
    buf[start:start + flat.numel()] = flat.cuda()
    return buf[start:start + flat.numel()]


@pytest.fixture(scope="module")
def inputs():
    """the six planes per size, shared by the layer sets and compressions and left unchanged, on the host and on the device, each
    also 4 bytes off the 16-byte grid: {(w, h): (planes, on, on_moved)}"""
    import torch
    rng = np.random.default_rng(2025)
    out = {}
    for w, h, _, _ in CASES:
        if (w, h) not in out:
            planes = lr.random_planes(rng, w, h)
            on = {k: _aligned(torch, a) for k, (a, _) in planes.items()}
            moved = {k: _aligned(torch, a, 4) for k, (a, _) in planes.items()} if (w, h) == lr.MOVED_CASE else None
            out[(w, h)] = (planes, on, moved)
    return out


def _launch_checked(torch, rrt, L, shift=0, want_wide=None, stream=None):
    """the launch into the middle of a larger buffer of sentinels, `shift` bytes off the 16-byte grid; returns the payload after
    checking the 64-byte guards on both sides"""
    n = rrt.exr_layers_frame_bytes(L)
    buf = torch.full((GUARD + n + GUARD + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + GUARD + shift
    g = rrt.exr_layers_launch_geometry(L, L.address_bits(buf.data_ptr() + start))
    if want_wide is not None:
        assert bool(g["wide"]) == want_wide, (L.w, L.h, shift, g)
    torch.cuda.synchronize()
    rrt.launch_exr_layers(buf[start:], L, stream=stream)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[:start] == SENTINEL).all() and (got[start + n:] == SENTINEL).all(), (L.w, L.h, shift)
    return got[start:start + n], g


@pytest.mark.parametrize("compression", lr.COMPRESSIONS)
@pytest.mark.parametrize("set_name", SETS)
def test_launch_equals_the_host_entry_point_and_the_restatement(set_name, compression, inputs):
    import torch
    import relativisticraytracer_amd as rrt
    channels = lr.LAYER_SETS[set_name]
    paths = set()
    for w, h, shift, moved in CASES:
        planes, on, on_moved = inputs[(w, h)]
        dev = dict(on)
        if moved:       # the plane of the set's last channel, 4 bytes off the grid
            key = lr.ordered(channels)[-1][2]
            dev[key] = on_moved[key]
        L = lr.api_layers(rrt, channels, planes, w, h, compression, on=dev)
        want = lr.payload(channels, planes, compression)
        got, g = _launch_checked(torch, rrt, L, shift, want_wide=(w % 8 == 0 and not shift and not moved))
        paths.add((g["wide"], g["passes"] > 1))
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (w, h, shift, moved, bad.size, bad[:8].tolist())
        assert np.array_equal(rrt.exr_layers_host(lr.api_layers(rrt, channels, planes, w, h, compression)), want), (w, h)
        for k, (a, _) in planes.items():        # the inputs are only read
            assert np.array_equal(dev[k].cpu().numpy().view(np.uint32), np.ascontiguousarray(a).ravel().view(np.uint32)), k
    # widths 8, 24 and 72 are 8 past a multiple of 16: where a filtered layout mixes sample sizes they take the 8-byte stores
    mixed = len({t == "half" for _, t, _, _ in channels}) == 2 and compression != "none"
    assert paths == ({(1, False), (False, False), (2, False), (2, True)} if mixed else {(1, False), (False, False), (1, True)})


def test_a_second_launch_on_a_side_stream_gives_the_same_bytes(inputs):
    import torch
    import relativisticraytracer_amd as rrt
    w, h = 24, 17
    planes, on, _ = inputs[(w, h)]
    for compression in ("zip", "none"):
        L = lr.api_layers(rrt, lr.LAYER_SETS["all_half"], planes, w, h, compression, on=on)
        first, _ = _launch_checked(torch, rrt, L)
        again, _ = _launch_checked(torch, rrt, L, stream=torch.cuda.Stream())
        assert np.array_equal(first, again) and np.array_equal(first, lr.payload(lr.LAYER_SETS["all_half"], planes, compression))


@pytest.mark.parametrize("fmt", xr.FORMATS, ids="-".join)
def test_bgr_layers_equal_the_dedicated_launch_on_the_device(fmt, inputs):
    import torch
    import relativisticraytracer_amd as rrt
    f = rrt.ExrFormat(*fmt)
    for w, h in ((72, 16), (64, 33), (9, 17)):
        planes, on, _ = inputs[(w, h)]
        L = lr.api_layers(rrt, lr.LAYER_SETS["bgr_" + fmt[0]], planes, w, h, fmt[1], on=on)
        out = torch.zeros(rrt.exr_frame_bytes(f, w, h), dtype=torch.uint8, device="cuda")
        rrt.launch_exr_from_hdr(out, on["hdr"], w, h, f)
        got, _ = _launch_checked(torch, rrt, L)
        assert np.array_equal(got, out.cpu().numpy()), (w, h)
        assert np.array_equal(got, xr.payload(planes["hdr"][0], fmt)), (w, h)


@pytest.mark.parametrize("half_max", [65504.0, 1024.0])
def test_the_conversion_lists_through_the_kernels(half_max):
    """every input the half conversion is pinned on, and the integers around every rounding and clamping edge, as 1-word planes
    through the wide kernel -- raw and filtered -- and, off the 16-byte grid, through the narrow one"""
    import torch
    import relativisticraytracer_amd as rrt
    w = 256
    vals = xr.conversion_inputs()
    h = -(-vals.size // w)
    f32 = np.full(h * w, 0.5, F)
    f32[:vals.size] = vals
    edge = np.array([0, 1, -1, 2047, 2048, 2049, 2050, 2051, 4097, 4098, 4099, 65504, 65519, 65520, 65521, 65536, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1,
                     2 ** 24 + 3, 2 ** 31 - 1, 2 ** 31 - 64, 2 ** 31 - 65, -2 ** 31, -2047, -2049, -65520, -2 ** 24 - 1], np.int64)
    i32 = np.resize(np.concatenate([edge, np.arange(-4200, 70000, 7)]), h * w).astype(np.int32)
    planes = {"f": (f32.reshape(h, w), False), "i": (i32.reshape(h, w), True)}
    channels = [("f.half", "half", "f", 0), ("f.float", "float", "f", 0), ("i.half", "half", "i", 0), ("i.float", "float", "i", 0),
                ("i.uint", "uint", "i", 0)]
    on = {k: _aligned(torch, a) for k, (a, _) in planes.items()}
    for compression, shift in (("none", 0), ("zip", 0), ("none", 2), ("zips", 6)):
        L = lr.api_layers(rrt, channels, planes, w, h, compression, half_max, on=on)
        got, _ = _launch_checked(torch, rrt, L, shift, want_wide=shift == 0)
        assert np.array_equal(got, lr.payload(channels, planes, compression, half_max)), (compression, shift)
        assert np.array_equal(got, rrt.exr_layers_host(lr.api_layers(rrt, channels, planes, w, h, compression, half_max))), (compression, shift)


def _debug_frame(torch, rrt, tex, w, h, t, cam, prm):
    """launch_raymarch_debug's outputs on the device, as the planes of a layer set: ({key: tensor}, {key: (array, bottom_up)})"""
    shapes = {"hdr": (F, 4), "rad": (F, 4), "pos": (F, 3), "vel": (F, 3), "steps": (np.int32, 1), "hit": (np.int32, 1)}
    on = {k: torch.zeros(h * w * n, dtype=torch.float32 if d is F else torch.int32, device="cuda") for k, (d, n) in shapes.items()}
    frame = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch_debug(frame, w, h, t, cam, tex, rrt.CameraEffects(), prm, **on)
    torch.cuda.synchronize()
    planes = {k: (v.cpu().numpy().reshape((h, w, shapes[k][1]) if shapes[k][1] > 1 else (h, w)), k == "hdr") for k, v in on.items()}
    return on, planes


def test_a_rendered_frame_into_a_layered_file_and_back(sky, tmp_path):
    """64 x 48 at a = 0.9 with volumetrics through launch_raymarch_debug -> launch_exr_layers -> EXRSink -> the restatement's reader:
    FLOAT and UINT channels hold the debug arrays exactly, HALF channels their half rounding"""
    import torch
    import relativisticraytracer_amd as rrt
    from relativisticraytracer_amd import sinks
    w, h = 64, 48
    tex = rrt.SkyTexture(sky)
    on, planes = _debug_frame(torch, rrt, tex, w, h, 1.0, rrt.CameraState.default(), rrt.RenderParams(spin=0.9, volumetrics=1))
    steps, hit, vel = planes["steps"][0], planes["hit"][0], planes["vel"][0]
    assert len(np.unique(steps)) > 20 and 0 < hit.sum() < hit.size and len(np.unique(planes["rad"][0][..., 3])) > 50      # a picture with a shadow and a medium
    for beauty, compression in (("half", "zip"), ("float", "zips"), ("half", "none")):
        channels = lr.standard_channels(lr.LAYER_NAMES, beauty)
        L = lr.api_layers(rrt, channels, planes, w, h, compression, on=on)
        payload, _ = _launch_checked(torch, rrt, L, want_wide=True)
        assert np.array_equal(payload, lr.payload(channels, planes, compression)), (beauty, compression)
        path = tmp_path / f"{beauty}_{compression}.exr"
        sink = sinks.EXRSink(str(path), w, h, 24, rrt.ExrFormat(beauty, compression), layers=L)
        sink.write(payload)
        sink.close()
        data = path.read_bytes()
        assert data == lr.write_file(channels, planes, compression)
        back = lr.read_file(data)
        ch = back["channels"]
        assert len(back["names"]) == 15 and back["types"]["steps"] == "uint" and back["types"]["horizon"] == "half"
        assert np.array_equal(ch["steps"], steps.astype(np.uint32)) and np.array_equal(ch["horizon"], hit.astype(np.float16))
        for k, axis in enumerate("XYZ"):
            assert np.array_equal(ch["direction." + axis].view(np.uint32), np.ascontiguousarray(vel[..., k]).view(np.uint32)), axis
            assert np.array_equal(ch["position." + axis].view(np.uint32), np.ascontiguousarray(planes["pos"][0][..., k]).view(np.uint32)), axis
        rad, hdr = planes["rad"][0], planes["hdr"][0][::-1]
        for name, src in (("emission.R", rad[..., 0]), ("emission.G", rad[..., 1]), ("emission.B", rad[..., 2]), ("transmittance", rad[..., 3]),
                          ("R", hdr[..., 0]), ("G", hdr[..., 1]), ("B", hdr[..., 2])):
            src = np.ascontiguousarray(src)
            if beauty == "float":
                assert np.array_equal(ch[name].view(np.uint32), src.view(np.uint32)), name
            else:
                assert np.array_equal(ch[name].view(np.uint16), xr.half_bits(src)), name
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
def debug_views():
    """what the Python API's debug launch and exposure pass leave for the driver's views, frame by frame, with `--auto-exposure` and
    without: headless.py's Renderer in this process -- {"exposed" | "plain": [planes per frame]}"""
    import torch
    from relativisticraytracer_amd import headless

    def frames(extra):
        ap = headless.build_parser()
        args = ap.parse_args(BASE + ["--exr", "unused.%04d.exr", "--exr-layers", "all"] + extra)
        pano, use_exposure, dof_k = headless.check_args(ap, args, 1)
        r = headless.Renderer(args, headless.build_settings(ap, args, pano, use_exposure), dof_k, 0, 1, torch.device("cuda", 0))
        shapes = {"hdr": 4, "rad": 4, "pos": 3, "vel": 3, "steps": 1, "hit": 1}
        out = []
        for k in range(1, FRAMES + 1):
            r.set_frame(k, lambda t: 0)
            r.render_post()
            torch.cuda.synchronize()
            on = dict(r.layer_planes, hdr=r.hdr)
            out.append({key: (on[key].cpu().numpy().reshape((H, W, n) if n > 1 else (H, W)).copy(), key == "hdr") for key, n in shapes.items()})
        r.close()
        return out
    return {"exposed": frames(["--auto-exposure"]), "plain": frames([])}


@pytest.mark.parametrize("exposure", ["plain", "exposed"])
@pytest.mark.parametrize("driver", ["py", "cpp"])
def test_driver_files_hold_the_debug_launchs_layers(driver, exposure, debug_views, tmp_path):
    """--frames 2 --exr f.%04d.exr --exr-layers all: each file is the restatement's, built from the debug outputs of the same view;
    its B, G, R are those of the same command without --exr-layers"""
    extra = ["--auto-exposure"] if exposure == "exposed" else []
    os.makedirs(tmp_path / "layers")
    os.makedirs(tmp_path / "beauty")
    _drive(driver, ["--exr", str(tmp_path / "layers" / "f.%04d.exr"), "--exr-layers", "all"] + extra)
    _drive(driver, ["--exr", str(tmp_path / "beauty" / "f.%04d.exr")] + extra)
    assert sorted(os.listdir(tmp_path / "layers")) == sorted(os.listdir(tmp_path / "beauty")) == ["f.0001.exr", "f.0002.exr"]
    views = debug_views[exposure]
    assert not np.array_equal(views[0]["steps"][0], views[1]["steps"][0])                      # the camera moves: a stale plane would show
    assert not np.array_equal(views[0]["hdr"][0], debug_views["plain" if exposure == "exposed" else "exposed"][0]["hdr"][0])
    assert np.array_equal(views[0]["rad"][0], debug_views["plain"][0]["rad"][0])              # the exposure scales B, G, R only
    channels = lr.standard_channels(lr.LAYER_NAMES, "half")
    for k, planes in enumerate(views, 1):
        data = (tmp_path / "layers" / f"f.{k:04d}.exr").read_bytes()
        back = lr.read_file(data)
        assert (back["width"], back["height"], back["compression"], len(back["names"])) == (W, H, "zip", 15)
        for name, _, want in lr.samples(channels, planes):
            assert np.array_equal(back["channels"][name].view(want.dtype), want), (driver, k, name)
        assert data == lr.write_file(channels, planes, "zip")                                  # both drivers deflate alike, at level 4
        beauty = xr.read_file((tmp_path / "beauty" / f"f.{k:04d}.exr").read_bytes())
        for c in "BGR":
            assert np.array_equal(back["channels"][c].view(np.uint16), beauty["channels"][c].view(np.uint16)), (driver, k, c)
