"""What the sampled launches' GPU tests share (a plain module, no conftest): how each kind of frame is rendered into host arrays,
the definition its test holds it to (the pairwise tree over the big 1x frame, the portable tone map), the random scenes and the
pinhole probes.  Where two tests need different things under one name, both are here under names of their own: all_fx_pano /
all_fx_stereo (the stereo one sets a vignette intensity and a distortion amount), probe_hdr_pano / probe_hdr_stereo (a direction /
an origin and a direction per probe), check_parity_ss / check_parity_mb.  torch is only the device-memory plumbing."""
import numpy as np

import projection_ref as pr
import stereo_ref as sr
from conftest import same_bits
from gpu_util import _host, _zeros


def render_ss(rrt, tex, w, h, s, t, cam, fx, prm):
    """the supersampled frame: (rgba8, hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    rrt.launch_raymarch_ss(out, w, h, s, t, cam, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def render_1x(rrt, tex, w, h, t, cam, fx, prm):
    """the 1x frame through the debug launch: (rgba8, post-FX hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    rrt.launch_raymarch_debug(out, w, h, t, cam, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def _tree(parts):
    """pairwise sum in natural order: ((p0 + p1) + (p2 + p3)) ..."""
    while len(parts) > 1:
        parts = [parts[k] + parts[k + 1] for k in range(0, len(parts), 2)]
    return parts[0]


def expected_mean(big_hdr, w, h, s):
    """the mean HDR of every s x s block of the (s h) x (s w) frame's HDR (bottom-up in, bottom-up out), in the order of the
    contract: within each sub-row j over i, then over the row sums, then * 1/s^2"""
    td = np.ascontiguousarray(big_hdr[::-1, :, :3], dtype=np.float32)      # top-down: row s y + j, column s x + i
    b = td.reshape(h, s, w, s, 3)
    rows = [_tree([b[:, j, :, i] for i in range(s)]) for j in range(s)]
    mean = _tree(rows) * np.float32(1.0 / (s * s))
    assert mean.dtype == np.float32
    return mean[::-1]


def tone_map(po, mean):
    """(uint8)(int)((1 - exp(-mean * 0.8f)) * 255) with the portable exp (raymarcher.cu:164-173, kExposure = 0.8f)"""
    x = (-mean).astype(np.float32) * np.float32(0.8)
    e = po.math_fn(0, po.MATH_PORTABLE, x.ravel()).reshape(x.shape)
    v = (np.float32(1.0) - e) * np.float32(255.0)
    rgb = (np.trunc(v).astype(np.int64) & 255).astype(np.uint8)
    return np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


def scene(rrt, rng, case, all_fx=False):
    """a tests/scene_gen.py scene made ragged for every s (odd w and h), volumetrics on and off by turns"""
    from scene_gen import random_scene
    sc = random_scene(rng, case)
    sc["w"] |= 1
    sc["h"] |= 1
    sc["vol"] = 0 if case % 3 == 2 else 1
    f = sc["fx"]
    on = lambda k: True if all_fx else bool(f[k])
    fx = rrt.CameraEffects(useBloom=on("use_bloom"), useVignette=on("use_vignette"), useChromaticAberration=on("use_ca"),
                           useLensDistortion=on("use_lens"), bloomThreshold=f["bloom_threshold"], bloomIntensity=f["bloom_intensity"],
                           vignetteIntensity=f["vignette_intensity"], caAmount=f["ca_amount"] if not all_fx else max(f["ca_amount"], 0.004),
                           distortionAmount=f["distortion_amount"])
    a = sc["cam"]
    return sc, rrt.CameraState(a[0], a[1], a[2], a[3]), fx


def check_parity_ss(po, rrt, tex, w, h, s, t, cam, fx, prm, what):
    big8, big_hdr = render_1x(rrt, tex, s * w, s * h, t, cam, fx, prm)
    got8, got_hdr = render_ss(rrt, tex, w, h, s, t, cam, fx, prm)
    mean = expected_mean(big_hdr, w, h, s)
    assert np.isfinite(mean).all(), what
    assert same_bits(got_hdr[..., :3], mean), (what, int((got_hdr[..., :3] != mean).sum()))
    assert np.all(got_hdr[..., 3] == 1.0), what
    want8 = tone_map(po, mean)
    assert np.array_equal(got8, want8), (what, int((got8 != want8).any(-1).sum()))
    return got8, big8


def render_mb(rrt, tex, w, h, s, times, cams, fx, prm):
    """the motion-blurred frame: (rgba8, hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    rrt.launch_raymarch_mb(out, w, h, s, times, cams, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def block_sums(big_hdr, w, h, s):
    """T_k: the sum of every s x s block of the (s h) x (s w) frame's HDR in the supersampled contract's order (bottom-up)"""
    td = np.ascontiguousarray(big_hdr[::-1, :, :3], dtype=np.float32)
    b = td.reshape(h, s, w, s, 3)
    rows = [_tree([b[:, j, :, i] for i in range(s)]) for j in range(s)]
    return _tree(rows)[::-1]


def expected_mean_mb(rrt, tex, w, h, s, times, cams, fx, prm):
    sums = [block_sums(render_1x(rrt, tex, s * w, s * h, t, c, fx, prm)[1], w, h, s) for t, c in zip(times, cams)]
    mean = _tree(sums) * np.float32(1.0 / (s * s * len(times)))
    assert mean.dtype == np.float32
    return mean


def moving_cameras(rrt, sc, n, step=0.35):
    """n cameras sliding along the scene camera's right vector (the same basis, a moved position)"""
    a = sc["cam"]
    out = []
    for k in range(n):
        pos = [a[0][i] + np.float32(step * k) * a[2][i] for i in range(3)]
        out.append(rrt.CameraState(pos, a[1], a[2], a[3]))
    return out


def check_parity_mb(po, rrt, tex, w, h, s, times, cams, fx, prm, what):
    mean = expected_mean_mb(rrt, tex, w, h, s, times, cams, fx, prm)
    got8, got_hdr = render_mb(rrt, tex, w, h, s, times, cams, fx, prm)
    assert np.isfinite(mean).all(), what
    assert same_bits(got_hdr[..., :3], mean), (what, int((got_hdr[..., :3] != mean).sum()))
    assert np.all(got_hdr[..., 3] == 1.0), what
    want8 = tone_map(po, mean)
    assert np.array_equal(got8, want8), (what, int((got8 != want8).any(-1).sum()))
    return got8


def all_fx_pano(rrt, vignette_lens=True):
    return rrt.CameraEffects(useBloom=True, useChromaticAberration=True, caAmount=0.004, useVignette=vignette_lens,
                             useLensDistortion=vignette_lens)


def render_pano(rrt, tex, w, h, s, proj, t, cam, fx, prm, stream=None):
    """(rgba8, hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    rrt.launch_raymarch_pano(out, w, h, s, proj, t, cam, tex, fx, prm, stream=stream, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def probe_hdr_pano(rrt, tex, t, pos, cam, forwards, fx, prm):
    """the post-FX HDR of pixel (1, 1) of a 2x2 pinhole frame looking along each of `forwards` (from `pos`, cam's right and up):
    u = v = 0 there, so its ray is exactly normalize(forward).  All launches first, one synchronisation."""
    import torch
    n = len(forwards)
    out, hdr = _zeros(n * 16, torch.uint8), _zeros(n * 16, torch.float32)
    a = cam.as_array()
    for k, f in enumerate(forwards):
        c = rrt.CameraState(pos, f, a[2], a[3])
        rrt.launch_raymarch_debug(out.data_ptr() + 16 * k, 2, 2, t, c, tex, fx, prm, hdr=hdr.data_ptr() + 64 * k)
    return _host(hdr, (n, 2, 2, 4))[:, 0, 1, :3]        # image row 1 is stored row 0 (bottom-up)


def all_fx_stereo(rrt, vignette_lens=True):
    return rrt.CameraEffects(useBloom=True, useChromaticAberration=True, caAmount=0.004, useVignette=vignette_lens,
                             vignetteIntensity=0.6, useLensDistortion=vignette_lens, distortionAmount=0.2)


def render_stereo(rrt, tex, w, h, s, proj, st, t, cam, fx, prm, stream=None):
    """(rgba8, hdr) of the composite, both (rows, cols, 4) bottom-up"""
    import torch
    cw, ch = st.composite(w, h)
    out, hdr = _zeros(ch * cw * 4, torch.uint8), _zeros(ch * cw * 4, torch.float32)
    rrt.launch_raymarch_stereo(out, w, h, s, proj, st, t, cam, tex, fx, prm, stream=stream, hdr=hdr)
    return _host(out, (ch, cw, 4)), _host(hdr, (ch, cw, 4))


def render_mono(rrt, tex, w, h, s, proj, t, cam, fx, prm):
    """the mono frame an eye's half is defined by: _ss for a pinhole, _pano for equirect"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    if proj.kind == pr.PINHOLE:
        rrt.launch_raymarch_ss(out, w, h, s, t, cam, tex, fx, prm, hdr=hdr)
    else:
        rrt.launch_raymarch_pano(out, w, h, s, proj, t, cam, tex, fx, prm, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))


def stereo_layout(st):
    return sr.TOP_BOTTOM if st.layout == 1 else sr.SIDE_BY_SIDE


def probe_hdr_stereo(rrt, tex, t, cam, rays, fx, prm):
    """the post-FX HDR of pixel (1, 1) of a 2x2 pinhole frame from each (origin, forward) of `rays` (cam's right and up): u = v = 0
    there, so its ray starts at origin and is exactly normalize(forward).  All launches first, one synchronisation."""
    import torch
    n = len(rays)
    out, hdr = _zeros(n * 16, torch.uint8), _zeros(n * 16, torch.float32)
    a = cam.as_array()
    for k, (o, f) in enumerate(rays):
        c = rrt.CameraState(o, f, a[2], a[3])
        rrt.launch_raymarch_debug(out.data_ptr() + 16 * k, 2, 2, t, c, tex, fx, prm, hdr=hdr.data_ptr() + 64 * k)
    return _host(hdr, (n, 2, 2, 4))[:, 0, 1, :3]        # image row 1 is stored row 0 (bottom-up)


def render_dof(rrt, tex, w, h, s, times, cams, lens, focus, fx, prm, stream=None):
    """the depth-of-field frame: (rgba8, hdr), both (h, w, 4) bottom-up"""
    import torch
    out, hdr = _zeros(h * w * 4, torch.uint8), _zeros(h * w * 4, torch.float32)
    if stream is not None:
        torch.cuda.synchronize()                # the buffers were cleared on the default stream
    rrt.launch_raymarch_dof(out, w, h, s, times, cams, lens, focus, tex, fx, prm, stream=stream, hdr=hdr)
    return _host(out, (h, w, 4)), _host(hdr, (h, w, 4))
