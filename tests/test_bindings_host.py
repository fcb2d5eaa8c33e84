"""The Python bindings' calls into the C ABI, pinned on the CPU: every public wrapper of the package, of camera_paths and of
sharding.PathChooser is run against a recording stand-in for the library, and the (symbol, arguments) it sends are compared with
tests/golden/bindings_calls.json.  That record was generated from the package as it stood BEFORE the bindings were put on one call
path (`python tests/test_bindings_host.py --write` at that commit) and has not been touched since: a wrapper that sends another
symbol, another order or another value fails here, where a swapped tile_rows / shard would otherwise only show as a wrong picture
on a GPU.  Needs neither a GPU nor the built library.

Normalisation of an argument: c_void_p -> its value; byref(x) -> x's label if the scenario named x, else ["&Type", contents];
ctypes arrays and structures -> their values; a host address (numpy's .ctypes.data, a typed pointer) -> "<addr>"; numbers and None
stay.  Every integer the scenario hands in is distinct, so no two arguments can swap unnoticed."""
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import pytest

import relativisticraytracer_amd as rrt
from relativisticraytracer_amd import _lib, camera_paths, sharding

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bindings_calls.json")
SIGNATURES = {name: (res, args) for name, res, args in _lib.SYMBOLS}

# out-parameters the stand-in fills (argument index -> value), so that the wrappers get ids to destroy and sizes to loop over
OUTS = {"rrt_sky_create": {3: 7001}, "rrt_workspace_create": {1: 7002}, "rrt_tile_order_create": {0: 7003},
        "rrt_tile_map_create": {4: 7004}, "rrt_noise_table_create_window": {3: 7005}, "rrt_path_chooser_create": {2: 7006},
        "rrt_tile_order_info": {3: 3}, "rrt_glow_weights": {5: 2}, "rrt_path_info": {1: b"orbit", 2: 2, 3: 1.5},
        "rrt_noise_table_fit_window": {3: 4.0, 4: 1, 5: 4096}, "rrt_adaptive_scratch_bytes": {2: 5001},
        "rrt_glow_scratch_bytes": {3: 5002}, "rrt_exposure_scratch_bytes": {0: 5003}}

# include/rrt.h entries that no Python wrapper reaches, and why
UNREACHED = {
    "rrt_status_string": "error path of _lib.check only (the stand-in never fails)",
    "rrt_last_hip_error": "error path of _lib.check only",
    "rrt_path_auto_max_rays": "read by headless.Renderer straight from the library, no wrapper",
    "rrt_sky_create_from_device": "C++ callers only",
    "rrt_noise_table_create": "superseded by _create_window, kept for C callers",
    "rrt_noise_table_plan": "superseded by _plan_window, kept for C callers",
    "rrt_launch_auto_resources": "C++ drop-in entry point's resources; tests call it raw",
    "rrt_launch_auto_resources_info": "as rrt_launch_auto_resources",
    "rrt_launch_raymarch_compat": "the reference-signature entry point; tests/compat calls it from C++",
    "rrt_workspace_read": "test-only read-back; tests call it raw",
}


class Recorder:
    """Stands in for the loaded library: every attribute is a function that records its call and returns 0."""

    def __init__(self):
        self.calls, self.problems, self.labels, self.keep = [], [], {}, []

    def name(self, obj, label):
        self.labels[id(obj)] = label
        self.keep.append(obj)
        return obj

    def norm(self, a):
        if a is None or isinstance(a, (str, bytes)):
            return a.decode() if isinstance(a, bytes) else a
        if isinstance(a, bool):
            return int(a)
        if isinstance(a, int):
            return "<addr>" if a >= 1 << 24 else a
        if isinstance(a, float):
            return a
        if isinstance(a, C.c_void_p):
            return self.norm(a.value)
        if isinstance(a, C.Array):
            return [self.norm(v) for v in a]
        if isinstance(a, C.Structure):
            return {k: self.norm(getattr(a, k)) for k, _ in a._fields_}
        if isinstance(a, C._SimpleCData):
            return self.norm(a.value)
        if hasattr(a, "_obj"):                              # byref(x)
            x = a._obj
            return self.labels.get(id(x)) or ["&" + type(x).__name__, self.norm(x)]
        if isinstance(a, C._Pointer):
            return "<addr>"
        raise TypeError(f"unexpected argument {a!r}")

    def __getattr__(self, sym):
        if not sym.startswith("rrt_"):
            raise AttributeError(sym)

        def call(*args):
            self.calls.append([sym, [self.norm(a) for a in args]])
            if sym not in SIGNATURES:
                self.problems.append(f"{sym}: not in _lib.SYMBOLS")
                return 0
            argtypes = SIGNATURES[sym][1]
            if len(args) != len(argtypes):
                self.problems.append(f"{sym}: {len(args)} arguments for {len(argtypes)} parameters")
            for k, (a, t) in enumerate(zip(args, argtypes)):
                try:
                    t.from_param(a)
                except (TypeError, C.ArgumentError) as e:
                    self.problems.append(f"{sym}: argument {k} {a!r} is no {t.__name__}: {e}")
            for k, v in OUTS.get(sym, {}).items():
                if args[k] is not None:
                    args[k]._obj.value = v
            return 0
        return call


class Tensor:
    """What the wrappers need of a device tensor."""

    def __init__(self, addr, numel=0, element_size=1):
        self.addr, self.n, self.es = addr, numel, element_size

    def data_ptr(self):
        return self.addr

    def numel(self):
        return self.n

    def element_size(self):
        return self.es


def _camera(x):
    c = _lib.rrt_camera()
    c.pos[:] = [x, x + 1, x + 2]
    return c


def run_scenario(rec):
    """Every wrapper once or more; the arguments are distinct integers (devices addresses and handles included)."""
    n = itertools.count(101)
    k = lambda: next(n)
    cam, fx, prm = rec.name(_lib.rrt_camera(), "cam"), rec.name(_lib.rrt_effects(), "fx"), rec.name(_lib.rrt_params(), "prm")
    proj, st = rec.name(_lib.rrt_projection(), "proj"), rec.name(_lib.rrt_stereo(), "stereo")
    glow, ad, ex = rec.name(_lib.rrt_glow(), "glow"), rec.name(_lib.rrt_adaptive(), "adaptive"), rec.name(_lib.rrt_exposure(), "exposure")

    def both(fn, *args, **kw):          # params=None and a structure; fresh integers for the second call's stream
        fn(*args, **kw, stream=k())
        fn(*args, **kw, params=prm, stream=k())

    # ---- structures and settings
    rrt.CameraState.from_angles((1, 2, 3), 4, 5)
    rrt.CameraState.default()
    rrt.CameraEffects(useBloom=True, caAmount=0.5)
    rrt.RenderParams(spin=0.5, max_steps=k())
    rrt.GlowSettings(radius=0.25, lobes=3)
    rrt.AdaptiveSettings()
    rrt.AdaptiveSettings(k())
    rrt.ExposureSettings(mode="auto", ev=1.5)
    rrt.ExposureSettings(mode=0)
    rrt.Projection("fisheye", 170.0)
    rrt.Projection(1, None, 90.0)
    rrt.projection_default("pinhole")
    rrt.Stereo("side-by-side", 0.5, 20.0, (60, 80))
    rrt.stereo_default(1)
    for cls in (rrt.RenderParams, rrt.GlowSettings, rrt.ExposureSettings):
        with pytest.raises(AttributeError):
            cls(no_such_field=1)
    rrt.projection_ray(proj, k(), k(), k(), k(), cam)
    rrt.stereo_ray(proj, st, k(), k(), k(), k(), k(), cam)
    rrt.lens_ray(k(), k(), k(), k(), cam, 0.25, 0.5, 30.0)
    rrt.lens_points(0.75, 4, 0.125)

    # ---- handle owners
    sky = rrt.SkyTexture(np.zeros((4, 8, 4), np.uint8))
    ws = rrt.Workspace(k())
    ws.stats()
    order = rrt.TileOrder()
    order.info()
    order.info(arrays=True)
    order.set_seeding(False)
    order.seeded_launches()
    tm = rrt.TileMap(7, 3, 2, [0, 1, 0])
    tm.shard_rows(1)
    tm.max_shard_rows()
    nt = rrt.NoiseTable(8.0, 2.0, rrt.TABLE_COARSE)
    nt.info()
    rrt.NoiseTable.window(1.0, 3.0).destroy()
    rrt.NoiseTable.plan(6.0, 1.0, rrt.TABLE_COARSEST)
    rrt.NoiseTable.plan_layout(6.0, 1.0, rrt.TABLE_BANDED)
    rrt.NoiseTable.fit(1.0, 9.0, k())
    nw = rrt.NoiseWindows(10.0, k())
    nw.table_id(0.5)
    nw.close()
    pc = sharding.PathChooser(k(), k())
    pc.policy(k())
    pc.report(k(), 2.5)
    pc.stats()

    # ---- host queries and defaults
    rrt.abi_version()
    rrt.device_count()
    rrt.set_launch_defaults(None)
    rrt.set_launch_defaults(prm)
    rrt.get_launch_defaults()
    rrt.march_cache_configure(k(), k())
    rrt.march_cache_configure(k())
    rrt.march_cache_stats(k())
    rrt.march_cache_release(k())
    rrt.tile_shard_rows(k(), k(), k(), k())
    rrt.balance_tiles([3.0, 1.0, 2.0], k(), k())
    rrt.probe_tile_costs(k(), 7, 3, 0.5, cam, fx, stream=k())
    rrt.probe_tile_costs(k(), 7, 3, 0.5, cam, fx, prm, stream=k())
    rrt.clock_probe(k(), k(), stream=k())
    rrt.glow_weights(glow, k(), k())
    rrt.glow_scratch_bytes(k(), k(), glow)
    rrt.adaptive_scratch_bytes(k(), k())
    rrt.adaptive_mask(np.zeros((3, 5, 4), np.uint8))
    rrt.adaptive_mask(np.zeros((3, 5, 4), np.uint8), ad)
    rrt.exposure_scratch_bytes()
    rrt.exposure_bin_ev(k())
    rrt.exposure_adapt(0.04, 0.5)
    rrt.exposure_meter_host(np.zeros((3, 5, 4), np.float32))
    camera_paths.catmull_rom((1, 2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12), 0.25)
    camera_paths.lerp_angle(10.0, 20.0, 0.5)
    path = camera_paths.CameraPath(k())
    path.camera_at(0.75)
    camera_paths.paths()
    camera_paths.recording_clock(k(), k())
    camera_paths.motion_clock(k(), k(), 0.5, 4)

    # ---- the plain launches and the assemblers
    both(rrt.launch_raymarch, k(), k(), k(), 0.5, cam, k(), fx)
    rrt.launch_raymarch(Tensor(k()), k(), k(), 0.5, cam, sky, fx, prm, stream=k())
    both(rrt.launch_raymarch_rows, k(), k(), k(), k(), k(), 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_tiles, k(), k(), k(), k(), k(), k(), 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_tilemap, k(), k(), k(), tm, k(), 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_tilemap, k(), k(), k(), k(), k(), 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_debug, k(), k(), k(), 0.5, cam, k(), fx, hdr=k(), steps=Tensor(k()), lut_oob=None)
    rrt.assemble_tiles(k(), k(), k(), k(), k(), k(), k(), stream=k())
    rrt.assemble_all_tiles(k(), k(), k(), k(), k(), k(), k(), stream=k())
    rrt.assemble_all_tilemap(k(), k(), k(), k(), k(), tm, stream=k())
    rrt.assemble_all_tilemap(k(), k(), k(), k(), k(), k(), stream=k())
    rrt.launch_projection_map(k(), k(), k(), proj, cam, stream=k())

    # ---- the sampled launches, whole (with and without hdr=) and in tiles
    times, cams, xy = [0.25, 0.5], [_camera(1.0), _camera(5.0)], [(0.1, 0.2), (0.3, 0.4)]
    both(rrt.launch_raymarch_ss, k(), k(), k(), k(), 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_ss, k(), k(), k(), k(), 0.5, cam, k(), fx, hdr=k())
    both(rrt.launch_raymarch_ss_tiles, k(), k(), k(), k(), k(), k(), k(), 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_mb, k(), k(), k(), k(), times, cams, k(), fx)
    both(rrt.launch_raymarch_mb, k(), k(), k(), k(), times, cams, k(), fx, hdr=k())
    both(rrt.launch_raymarch_mb_tiles, k(), k(), k(), k(), k(), k(), k(), times, cams, k(), fx)
    both(rrt.launch_raymarch_dof, k(), k(), k(), k(), times, cams, xy, 30.0, k(), fx)
    both(rrt.launch_raymarch_dof, k(), k(), k(), k(), times, cams, xy, 30.0, k(), fx, hdr=k())
    both(rrt.launch_raymarch_dof_tiles, k(), k(), k(), k(), k(), k(), k(), times, cams, xy, 30.0, k(), fx)
    both(rrt.launch_raymarch_pano, k(), k(), k(), k(), proj, 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_pano, k(), k(), k(), k(), proj, 0.5, cam, k(), fx, hdr=k())
    both(rrt.launch_raymarch_pano_tiles, k(), k(), k(), k(), k(), k(), k(), proj, 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_stereo, k(), k(), k(), k(), proj, st, 0.5, cam, k(), fx)
    both(rrt.launch_raymarch_stereo, k(), k(), k(), k(), proj, st, 0.5, cam, k(), fx, hdr=k())
    both(rrt.launch_raymarch_stereo_tiles, k(), k(), k(), k(), k(), k(), k(), proj, st, 0.5, cam, k(), fx)
    with pytest.raises(ValueError):
        rrt.launch_raymarch_mb(k(), k(), k(), k(), times, cams[:1], k(), fx)
    with pytest.raises(ValueError):
        rrt.launch_raymarch_dof(k(), k(), k(), k(), times, cams, xy[:1], 30.0, k(), fx)

    # ---- the scratch-taking launches: an explicit size, a tensor's own, the library's figure (raw pointer, no size)
    both(rrt.launch_raymarch_adaptive, k(), k(), k(), k(), None, ad, 0.5, cam, k(), fx, k(), scratch_bytes=k())
    both(rrt.launch_raymarch_adaptive, k(), k(), k(), k(), proj, ad, 0.5, cam, k(), fx, Tensor(k(), k(), 4), hdr=k())
    rrt.launch_raymarch_adaptive(k(), k(), k(), k(), proj, ad, 0.5, cam, k(), fx, k(), stream=k())
    rrt.launch_glow(k(), k(), k(), k(), glow, k(), stream=k(), scratch_bytes=k())
    rrt.launch_glow(k(), k(), k(), k(), glow, Tensor(k(), k(), 2), stream=k())
    rrt.launch_glow(k(), k(), k(), k(), glow, k(), stream=k())
    rrt.launch_exposure_reset(k(), stream=k(), scratch_bytes=k())
    rrt.launch_exposure_reset(Tensor(k(), k(), 8), stream=k())
    rrt.launch_exposure_reset(k(), stream=k())
    rrt.launch_exposure(k(), k(), k(), k(), k(), ex, stream=k())
    rrt.launch_exposure(None, None, k(), k(), k(), ex, k(), stream=k(), scratch_bytes=k())
    rrt.launch_exposure(k(), None, k(), k(), k(), ex, Tensor(k(), k(), 4), stream=k())
    rrt.launch_exposure(k(), None, k(), k(), k(), ex, k(), stream=k())

    for obj in (sky, ws, order, tm, nt, pc):
        obj.destroy()
    return rec


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder()
    monkeypatch.setattr(_lib, "_lib", rec)
    return rec


def test_every_wrapper_sends_the_recorded_call(recorder):
    run_scenario(recorder)
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(recorder.calls))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"call {k}"
    assert len(got) == len(want)


def test_every_call_fits_its_declared_signature(recorder):
    run_scenario(recorder)
    assert recorder.problems == []


def test_the_record_covers_every_symbol_a_wrapper_reaches(recorder):
    run_scenario(recorder)
    reached = {c[0] for c in recorder.calls}
    assert reached <= set(SIGNATURES)
    assert set(SIGNATURES) - reached == set(UNREACHED), "an entry of rrt.h lost or gained its wrapper: record it, or say why not"


HANDLE_KINDS = [       # (make the object, call one of its methods, the attribute that holds its id)
    (lambda: rrt.SkyTexture(np.zeros((4, 8, 4), np.uint8)), None, "handle"),
    (lambda: rrt.Workspace(1 << 20), lambda o: o.stats(), "id"),
    (lambda: rrt.TileOrder(), lambda o: (o.info(arrays=True), o.set_seeding(True), o.seeded_launches()), "id"),
    (lambda: rrt.TileMap(7, 3, 2, [0, 1, 0]), lambda o: (o.shard_rows(1), o.max_shard_rows()), "id"),
    (lambda: rrt.NoiseTable(8.0), lambda o: o.info(), "id"),
    (lambda: sharding.PathChooser(3), lambda o: (o.policy(1), o.report(1, 2.5), o.stats()), "id"),
]


@pytest.mark.parametrize("make,use,id_attr", HANDLE_KINDS, ids=["sky", "workspace", "tile_order", "tile_map", "noise_table", "path_chooser"])
def test_a_handle_talks_to_the_library_that_made_it(monkeypatch, make, use, id_attr):
    """An object created while library A is current sends its methods and its destroy to A after B has become current; a second
    destroy(), and a destroy() after the id was set to 0, call nothing."""
    a, b = Recorder(), Recorder()
    monkeypatch.setattr(_lib, "_lib", a)
    obj, dropped = make(), make()
    monkeypatch.setattr(_lib, "_lib", b)
    n_created = len(a.calls)
    if use is not None:
        use(obj)
        assert len(a.calls) > n_created
    made_id = getattr(obj, id_attr)
    assert made_id != 0
    obj.destroy()
    assert a.calls[-1] == [type(obj)._destroy, [made_id]] and getattr(obj, id_attr) == 0
    n = len(a.calls)
    obj.destroy()
    setattr(dropped, id_attr, 0)
    dropped.destroy()
    del obj, dropped
    assert len(a.calls) == n and b.calls == [] and a.problems == []


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    rec = Recorder()
    _lib._lib = rec
    run_scenario(rec)
    with open(GOLDEN, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(c) for c in rec.calls) + "\n]\n")
    print(f"{len(rec.calls)} calls of {len({c[0] for c in rec.calls})} symbols -> {GOLDEN}")
