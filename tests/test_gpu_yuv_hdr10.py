"""HDR10 output on the device: rrt_launch_yuv_hdr10_from_hdr against the numpy restatement (tests/hdr10_ref.py) -- the planes byte for
byte and the light-level state word for word -- at sizes of both launch paths and at the shapes where the reduction can go wrong, a
film of three frames eagerly and through a captured graph, a rendered frame, and both headless drivers' --y4m-transfer pq files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hdr10_ref as hr
import yuv_ref as yr

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32
IDS = dict(ids=lambda f: f"{f[0]}-{'full' if f[1] else 'limited'}-{f[2]}" if isinstance(f, tuple) and len(f) == 3 else None)
SENTINEL, BEFORE, AFTER = 0xA5, 16, 64
KNEES = (0.0, 0.5, 1.0)


def _fmt(rrt, fmt):
    return rrt.YuvFormat(fmt[0], "full" if fmt[1] else "limited", fmt[2])


class Light:
    """a light-level state in the middle of a buffer of sentinels, 16-byte aligned"""

    def __init__(self, torch, rrt):
        self.torch = torch
        self.buf = torch.full((16 + 16 + 32 + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.at = (-self.buf.data_ptr()) % 16 + 16
        self.ptr = self.buf.data_ptr() + self.at
        rrt.launch_yuv_hdr10_light_reset(self.ptr)

    def words(self):
        """the state's 32 bytes, after checking the sentinels on both sides"""
        self.torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        assert (got[:self.at] == SENTINEL).all() and (got[self.at + 32:] == SENTINEL).all()
        return got[self.at:self.at + 32].tobytes()


def _launch_checked(torch, rrt, src, w, h, f, settings, light):
    """the launch into the middle of a larger buffer of sentinels; returns the frame's bytes after checking both margins"""
    n = rrt.yuv_frame_bytes(f, w, h)
    buf = torch.full((BEFORE + n + AFTER + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + BEFORE
    rrt.launch_yuv_hdr10_from_hdr(buf[start:], src, w, h, f, settings, light)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[start - BEFORE:start] == SENTINEL).all() and (got[start + n:start + n + AFTER] == SENTINEL).all(), (w, h)
    return got[start:start + n]


@pytest.fixture(scope="module")
def inputs():
    """one HDR frame per size, shared by the formats and left unchanged"""
    import relativisticraytracer_amd as rrt
    rng = np.random.default_rng(2084)
    return {(w, h): yr.hdr_frame(rng, w, h) for w, h in yr.sizes(rrt.yuv_launch_geometry(None, 64, 48))}


@pytest.fixture(scope="module")
def expected(inputs, po):
    """{(size, knee): (q, the state's words after one frame)} by the restatement, once"""
    out = {}
    for size, hdr in inputs.items():
        for knee in KNEES:
            settings = (203.0, 1000.0, knee)
            c = hr.nits(po, hdr, settings)
            out[(size, knee)] = (hr.pq(po, c), hr.state_words(hr.meter(c, hr.new_state())))
    return out


@pytest.mark.parametrize("fmt", hr.FORMATS, **IDS)
def test_launch_equals_the_restatement(fmt, inputs, expected):
    import torch
    import relativisticraytracer_amd as rrt
    f = _fmt(rrt, fmt)
    paths = set()
    for (w, h), hdr in inputs.items():
        paths.add(rrt.yuv_launch_geometry(f, w, h)["wide"])
        d_hdr = torch.from_numpy(hdr).cuda()
        for knee in KNEES:
            settings = rrt.Hdr10Settings(knee=knee)
            q, words = expected[((w, h), knee)]
            want = yr.pack(hr.planes(q, fmt), 10)
            light = Light(torch, rrt)
            got = _launch_checked(torch, rrt, d_hdr, w, h, f, settings, light.ptr)
            assert np.array_equal(got, want), (w, h, knee, int((got != want).sum()))
            assert light.words() == words, (w, h, knee)
            light = Light(torch, rrt)
            again = _launch_checked(torch, rrt, d_hdr, w, h, f, settings, light.ptr)              # a second run: the same bytes
            assert np.array_equal(again, got) and light.words() == words, (w, h, knee)
            # without a state: the same planes, and a state nearby keeps every sentinel
            idle = torch.full((32,), SENTINEL, dtype=torch.uint8, device="cuda")
            bare = _launch_checked(torch, rrt, d_hdr, w, h, f, settings, None)
            assert np.array_equal(bare, got), (w, h, knee)
            assert (idle.cpu().numpy() == SENTINEL).all()
        assert np.array_equal(d_hdr.cpu().numpy().view(np.uint32), hdr.view(np.uint32))           # the input is only read
    assert paths == {True, False}, "the size list must hold sizes of both launch paths"


def _one_bright(w, h, col, row):
    """black but for one pixel at display (col, row)"""
    a = np.zeros((h, w, 4), F)
    a[h - 1 - row, col, :3] = (0.5, 2.0, 1.0)
    return a


def test_the_reductions_shapes(po):
    """the smallest frames at which the wavefront, workgroup and grid stages of the metering can go wrong"""
    import torch
    import relativisticraytracer_amd as rrt
    g = rrt.yuv_launch_geometry(None, 64, 48)
    assert g["threads"] == 256 and (g["strip_w"], g["strip_h"]) == (8, 2)      # the shapes below are worked out for these
    block_w = g["strip_w"] * g["threads"]                                      # one workgroup's strips in one strip row
    rng = np.random.default_rng(861)
    fmt = (420, False, 10)
    f = _fmt(rrt, fmt)
    cases = []
    for w, h in ((1, 1), (64, 4), (512, 2), (block_w - 8, 2), (block_w, 2), (block_w + 8, 2), (block_w - 1, 2), (216, 38)):
        cases.append(((w, h), np.exp2(rng.uniform(-8.0, 3.0, (h, w, 4))).astype(F), hr.DEFAULT))
    w, h = 216, 38                                                             # 27 x 19 = 513 strips: three workgroups, the last holds one
    assert rrt.yuv_launch_geometry(f, w, h)["wide"] and (w // 8) * (h // 2) == 2 * g["threads"] + 1
    for col, row in ((w - 1, 7), (100, h - 1), (9 * 8 + 7, 2 * 2 + 1), (w - 1, h - 1), (0, 0)):      # (79, 5): strip 63, lane 63
        cases.append(((w, h), _one_bright(w, h, col, row), hr.DEFAULT))
    cases.append(((128, 64), np.full((64, 128, 4), np.inf, F), (203.0, 10000.0, 0.5)))             # frame_sum passes 2^32
    for (w, h), hdr, settings in cases:
        state = hr.new_state()
        want = hr.frame(po, hdr, fmt, settings, state)
        light = Light(torch, rrt)
        got = _launch_checked(torch, rrt, torch.from_numpy(hdr).cuda(), w, h, f, rrt.Hdr10Settings(*settings), light.ptr)
        assert np.array_equal(got, want), (w, h)
        assert light.words() == hr.state_words(state), (w, h)
    assert state["max_frame_sum"] == 8192 * 640000 > 1 << 32
    assert rrt.yuv_hdr10_light_levels(np.frombuffer(light.words(), np.uint8), 128, 64) == {"max_cll": 10000, "max_fall": 10000, "frames": 1}


def test_a_film_of_three_frames_eagerly_and_as_a_graph(po):
    """reset, then pack and fold three times: the state and the resolved levels equal the restatement; the same chain -- linear, no
    parallel branch -- captured into a graph and replayed gives the same state and planes"""
    import torch
    import relativisticraytracer_amd as rrt
    w, h, fmt = 64, 48, (420, False, 10)
    f, settings = _fmt(rrt, fmt), rrt.Hdr10Settings()
    rng = np.random.default_rng(3)
    frames = [np.exp2(rng.uniform(-9.0, lift, (h, w, 4))).astype(F) for lift in (1.0, 3.0, -2.0)]
    state, want = hr.new_state(), []
    for hdr in frames:
        want.append(hr.frame(po, hdr, fmt, hr.DEFAULT, state))
    assert state["frames"] == 3
    d_frames = [torch.from_numpy(a).cuda() for a in frames]
    n = rrt.yuv_frame_bytes(f, w, h)
    outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in frames]
    light = Light(torch, rrt)
    for d, o in zip(d_frames, outs):
        rrt.launch_yuv_hdr10_from_hdr(o, d, w, h, f, settings, light.ptr)
    assert light.words() == hr.state_words(state)
    assert all(np.array_equal(o.cpu().numpy(), b) for o, b in zip(outs, want))
    levels = rrt.yuv_hdr10_light_levels(np.frombuffer(light.words(), np.uint8), w, h)
    assert levels == hr.levels(state, w, h) and levels["max_cll"] > levels["max_fall"] > 0
    # captured: the reset is part of the graph, so every replay is a film of its own
    light = Light(torch, rrt)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rrt.launch_yuv_hdr10_light_reset(light.ptr)
        for d, o in zip(d_frames, outs):
            rrt.launch_yuv_hdr10_from_hdr(o, d, w, h, f, settings, light.ptr)
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        assert light.words() == hr.state_words(state)
        assert all(np.array_equal(o.cpu().numpy(), b) for o, b in zip(outs, want))


def test_a_rendered_frame(po, sky):
    """64 x 48 at a = 0.9 through launch_raymarch_ss(..., hdr=H), encoded: the restatement of the same HDR"""
    import torch
    import relativisticraytracer_amd as rrt
    w, h = 64, 48
    tex = rrt.SkyTexture(sky)
    B = torch.zeros(h * w * 4, dtype=torch.uint8, device="cuda")
    H = torch.zeros(h * w * 4, dtype=torch.float32, device="cuda")
    rrt.launch_raymarch_ss(B, w, h, 1, 1.0, rrt.CameraState.default(), tex, rrt.CameraEffects(), rrt.RenderParams(spin=0.9), hdr=H)
    torch.cuda.synchronize()
    lin = H.cpu().numpy().reshape(h, w, 4)
    for fmt in ((420, False, 10), (444, True, 10)):
        f = _fmt(rrt, fmt)
        state = hr.new_state()
        want = hr.frame(po, lin, fmt, hr.DEFAULT, state)
        assert len(np.unique(want)) > 50                                         # a picture, not a flat frame
        light = Light(torch, rrt)
        out = torch.zeros(rrt.yuv_frame_bytes(f, w, h), dtype=torch.uint8, device="cuda")
        rrt.launch_yuv_hdr10_from_hdr(out, H, w, h, f, None, light.ptr)
        assert light.words() == hr.state_words(state)
        assert np.array_equal(out.cpu().numpy(), want), fmt
    tex.destroy()


# ---- the drivers

W, H, FRAMES = 64, 48, 3
BASE = ["--width", str(W), "--height", str(H), "--frames", str(FRAMES), "--spin", "0.9", "--path", "0", "--auto-exposure"]
FMT = (444, True, 10)                   # the format the level check below inverts
Y4M10 = ["--y4m-depth", "10", "--y4m-chroma", "444", "--y4m-range", "full"]


def _drive(driver, args):
    if driver == "cpp":
        from relativisticraytracer_amd import build
        cmd = [build.build_headless()]
    else:
        cmd = [sys.executable, "-m", "relativisticraytracer_amd.headless"]
    r = subprocess.run(cmd + BASE + args, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _nits_of_the_file(frame):
    """the largest channel's light per pixel of a 4:4:4 full-range frame, decoded in float64: BT.2020 inverse matrix, inverse PQ"""
    s = frame.view(np.dtype("<u2")).astype(np.float64).reshape(3, H, W)
    y, cb, cr = s[0] / 1023.0, (s[1] - 512.0) / 1023.0, (s[2] - 512.0) / 1023.0
    r = y + 2.0 * (1.0 - hr.KR) * cr
    b = y + 2.0 * (1.0 - hr.KB) * cb
    g = (y - hr.KR * r - hr.KB * b) / hr.KG
    e = np.clip(np.stack([r, g, b]), 0.0, 1.0) ** (1.0 / 78.84375)
    c = 1.0e4 * (np.maximum(e - 0.8359375, 0.0) / (18.8515625 - 18.6875 * e)) ** (1.0 / 0.1593017578125)
    return c.max(axis=0)


def test_both_drivers_write_the_same_hdr10_film(tmp_path):
    """three frames with --y4m-depth 10 --y4m-transfer pq --auto-exposure: the frames are equal between the drivers and the sidecars
    byte-identical.  The drivers keep no HDR to restate the levels from exactly (the film test above does that); here the sidecar's
    levels are tied to the file: decoded in float64, the file's own MaxCLL and MaxFALL lie within 4 % of the sidecar's plus 1 nit -- a
    code is rounded by up to half a step in each of Y', Cb and Cr, which moves a channel by up to 0.5 + 1.48 * 0.5 = 1.24 codes of
    1023, 0.0012 of the PQ signal, and the PQ curve's slope d ln(nits) / d signal is at most 27 over 1 ... 1000 nits: 3.3 %.
    Without --y4m-transfer the same command lines write what --y4m-transfer sdr writes, and no sidecar."""
    files = {}
    for driver in ("py", "cpp"):
        pq, sdr, plain = (tmp_path / f"{driver}_{k}.y4m" for k in ("pq", "sdr", "plain"))
        _drive(driver, ["--y4m", str(pq)] + Y4M10 + ["--y4m-transfer", "pq"])
        _drive(driver, ["--y4m", str(sdr)] + Y4M10 + ["--y4m-transfer", "sdr"])
        _drive(driver, ["--y4m", str(plain)] + Y4M10)
        assert plain.read_bytes() == sdr.read_bytes() != pq.read_bytes()
        assert not os.path.exists(str(plain) + ".hdr10.json") and not os.path.exists(str(sdr) + ".hdr10.json")
        files[driver] = (pq.read_bytes(), (tmp_path / f"{driver}_pq.y4m.hdr10.json").read_bytes(), plain.read_bytes())
    assert files["py"][0] == files["cpp"][0] and files["py"][1] == files["cpp"][1] and files["py"][2] == files["cpp"][2]
    head, frames = yr.parse_y4m(files["py"][0], FMT, W, H)
    assert head == yr.header(FMT, W, H) and len(frames) == FRAMES
    doc = json.loads(files["py"][1])
    assert (doc["white_nits"], doc["peak_nits"], doc["knee"], doc["frames"]) == (203, 1000, 0.5, FRAMES)
    assert files["py"][1] == hr.sidecar(hr.DEFAULT, doc)
    light = [_nits_of_the_file(f) for f in frames]
    cll, fall = max(m.max() for m in light), max(m.mean() for m in light)
    print(f"sidecar MaxCLL {doc['max_cll']} MaxFALL {doc['max_fall']}; decoded from the file {cll:.2f} {fall:.2f}")
    assert doc["max_cll"] >= doc["max_fall"] > 0
    assert abs(cll - doc["max_cll"]) <= 0.04 * doc["max_cll"] + 1.0 and abs(fall - doc["max_fall"]) <= 0.04 * doc["max_fall"] + 1.0
