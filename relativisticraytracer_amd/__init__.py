"""relativisticraytracer_amd -- MI355X (gfx950) implementation of the per-pixel
geodesic ray-march hot path of levi2234/RelativisticRayTracer.

Host-side mirror of the reference's interface for this path
(include/raymarcher.h:11-19, include/camera_effects/camera_settings.h:4-17):

    cam = rrt.CameraState.from_angles((0, 10, -60), yaw=0, pitch=-10)
    sky = rrt.SkyTexture(rgba8_numpy)
    out = torch.empty(h * w * 4, dtype=torch.uint8, device="cuda")
    rrt.launch_raymarch(out, w, h, time, cam, sky, rrt.CameraEffects())

Everything goes through the C ABI of librrt_hip.so (include/rrt.h).  torch is
only used for device memory / streams and is optional: any object with a
`data_ptr()` or a plain integer device address is accepted.  There is no CPU
implementation in this package.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import RRTError, rrt_camera, rrt_debug_outputs, rrt_effects, rrt_glow, rrt_params, rrt_projection  # noqa: F401
from ._lib import rrt_adaptive, rrt_exposure, rrt_stereo  # noqa: F401

__all__ = ["CameraState", "CameraEffects", "RenderParams", "SkyTexture", "Workspace", "NoiseTable", "launch_raymarch",
           "set_launch_defaults", "get_launch_defaults",
           "launch_raymarch_rows", "launch_raymarch_tiles", "assemble_tiles", "assemble_all_tiles",
           "launch_raymarch_ss", "launch_raymarch_ss_tiles", "launch_raymarch_mb", "launch_raymarch_mb_tiles",
           "GlowSettings", "glow_weights", "glow_scratch_bytes", "launch_glow",
           "Projection", "projection_default", "projection_ray", "launch_projection_map", "launch_raymarch_pano", "launch_raymarch_pano_tiles",
           "AdaptiveSettings", "adaptive_scratch_bytes", "adaptive_mask", "launch_raymarch_adaptive",
           "Stereo", "stereo_default", "stereo_ray", "launch_raymarch_stereo", "launch_raymarch_stereo_tiles",
           "launch_raymarch_dof", "launch_raymarch_dof_tiles", "lens_ray", "lens_points",
           "ExposureSettings", "exposure_scratch_bytes", "exposure_bin_ev", "exposure_adapt", "exposure_meter_host",
           "launch_exposure_reset", "launch_exposure",
           "tile_shard_rows",
           "launch_raymarch_debug", "RRTError", "device_count", "abi_version", "TileOrder", "TileMap",
           "probe_tile_costs", "balance_tiles", "launch_raymarch_tilemap", "assemble_all_tilemap", "clock_probe", "clock_probe_ghz",
           "march_cache_configure", "march_cache_stats", "march_cache_release"]


def _ptr(x):
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(f"expected a device tensor or an integer device address, got {type(x)}")


def _stream(stream):
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        except Exception:
            pass
        return None
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


_call = _lib.call       # _call("rrt_x", *args): rrt_x of the current library; any status but RRT_OK raises RRTError("rrt_x: ...")


def _ref(x):
    return C.byref(x) if x is not None else None


def _init_settings(self, default, extra, kw):
    """What the keyword settings classes construct with: the library's defaults (`default`(&self, *extra)), then the keywords; an
    unknown name raises AttributeError."""
    _call(default, C.byref(self), *extra)
    for k, v in kw.items():
        if not hasattr(self, k):
            raise AttributeError(k)
        setattr(self, k, v)


class CameraState(rrt_camera):
    """Reference `struct CameraState` (include/raymarcher.h:11-16)."""

    def __init__(self, pos=(0, 0, 0), forward=(0, 0, 1), right=(1, 0, 0), up=(0, 1, 0)):
        super().__init__()
        for name, v in (("pos", pos), ("forward", forward), ("right", right), ("up", up)):
            arr = getattr(self, name)
            for k in range(3):
                arr[k] = float(v[k])

    @classmethod
    def from_angles(cls, pos, yaw, pitch):
        """CameraController::getCUDAStateFrom (src/main.cpp:141-167); degrees."""
        out = cls()
        p = (C.c_float * 3)(*[float(v) for v in pos])
        _call("rrt_camera_from_angles", C.byref(p), float(yaw), float(pitch), C.byref(out))
        return out

    @classmethod
    def default(cls):
        """The reference's start-up camera (src/main.cpp:128-130)."""
        return cls.from_angles((0.0, 10.0, -60.0), 0.0, -10.0)

    def as_array(self):
        return np.array([list(self.pos), list(self.forward), list(self.right), list(self.up)], np.float32)


class CameraEffects(rrt_effects):
    """Reference `struct CameraEffects` with its default member initialisers
    (camera_settings.h:5-16); attribute names follow the reference."""

    _ALIASES = {"useBloom": "use_bloom", "bloomThreshold": "bloom_threshold",
                "bloomIntensity": "bloom_intensity", "useVignette": "use_vignette",
                "vignetteIntensity": "vignette_intensity",
                "useChromaticAberration": "use_chromatic_aberration", "caAmount": "ca_amount",
                "useLensDistortion": "use_lens_distortion", "distortionAmount": "distortion_amount"}

    def __init__(self, **kw):
        super().__init__()
        _call("rrt_effects_default", C.byref(self))
        for k, v in kw.items():
            setattr(self, k, v)

    def __setattr__(self, k, v):
        k = self._ALIASES.get(k, k)
        if k.startswith("use_"):
            v = 1 if v else 0
        super().__setattr__(k, v)

    def __getattr__(self, k):
        alias = type(self)._ALIASES.get(k)
        if alias is None:
            raise AttributeError(k)
        return getattr(self, alias)


class RenderParams(rrt_params):
    """Scene constants of include/config.h as run-time parameters (defaults == config.h)."""

    def __init__(self, **kw):
        super().__init__()
        _init_settings(self, "rrt_params_init", (C.sizeof(rrt_params),), kw)


class GlowSettings(rrt_glow):
    """HDR glow settings (include/rrt.h: rrt_glow): radius (sigma_0 as a fraction of the frame height), lobes (1-4), threshold,
    intensity.  Defaults == rrt_glow_default."""

    def __init__(self, **kw):
        super().__init__()
        _init_settings(self, "rrt_glow_default", (), kw)

    def info(self):
        return {"radius": self.radius, "lobes": self.lobes, "threshold": self.threshold, "intensity": self.intensity}


class AdaptiveSettings(rrt_adaptive):
    """Adaptive supersampling settings (include/rrt.h: rrt_adaptive): threshold T in [0, 255] -- a pixel is refined if it differs
    from a 4-neighbour by more than T in a colour channel of the stored 1x frame.  Default == rrt_adaptive_default (8)."""

    def __init__(self, threshold=None):
        super().__init__()
        _call("rrt_adaptive_default", C.byref(self))
        if threshold is not None:
            self.threshold = int(threshold)

    def info(self):
        return {"threshold": self.threshold}


EXPOSURE_MANUAL, EXPOSURE_AUTO = 0, 1                         # include/rrt.h: RRT_EXPOSURE_*
EXPOSURE_MODES = {"manual": EXPOSURE_MANUAL, "auto": EXPOSURE_AUTO}
EXPOSURE_HIST_OFFSET, EXPOSURE_STATE_OFFSET, EXPOSURE_TABLE_OFFSET = 0, 1024, 1088      # RRT_EXPOSURE_*_OFFSET: the scratch's layout


class ExposureSettings(rrt_exposure):
    """Exposure settings (include/rrt.h: rrt_exposure): mode "manual" | "auto" (or RRT_EXPOSURE_*), ev (the manual EV, or the
    compensation in auto mode), key, low_permille / high_permille (the shares of the metered pixels left out of the average),
    min_ev / max_ev, adapt_up / adapt_down (exposure_adapt makes them from time constants).  Defaults == rrt_exposure_default."""

    def __init__(self, **kw):
        super().__init__()
        if "mode" in kw:
            kw["mode"] = EXPOSURE_MODES.get(kw["mode"], kw["mode"])
        _init_settings(self, "rrt_exposure_default", (), kw)

    def info(self):
        return {"mode": "auto" if self.mode == EXPOSURE_AUTO else "manual", "ev": self.ev, "key": self.key,
                "low_permille": self.low_permille, "high_permille": self.high_permille, "min_ev": self.min_ev, "max_ev": self.max_ev,
                "adapt_up": self.adapt_up, "adapt_down": self.adapt_down}


PROJ_PINHOLE, PROJ_EQUIRECT, PROJ_FISHEYE = 0, 1, 2          # include/rrt.h: RRT_PROJ_*
PROJECTION_KINDS = {"pinhole": PROJ_PINHOLE, "equirect": PROJ_EQUIRECT, "fisheye": PROJ_FISHEYE}


class Projection(rrt_projection):
    """The camera of a panorama (include/rrt.h: rrt_projection): kind "pinhole" | "equirect" | "fisheye" (or RRT_PROJ_*), fov_deg
    (equirect: horizontal span, default 360; fisheye: aperture, default 180) and vfov_deg (equirect: vertical span, default 180).
    Defaults == rrt_projection_default(kind); the spans are checked by the calls that use them."""

    def __init__(self, kind="equirect", fov_deg=None, vfov_deg=None):
        super().__init__()
        k = PROJECTION_KINDS.get(kind, kind)
        if not isinstance(k, int):
            raise ValueError(f"projection kind: one of {sorted(PROJECTION_KINDS)}, got {kind!r}")
        _call("rrt_projection_default", k, C.byref(self))
        if fov_deg is not None:
            self.fov_deg = float(fov_deg)
        if vfov_deg is not None:
            self.vfov_deg = float(vfov_deg)

    @property
    def name(self):
        return {v: k for k, v in PROJECTION_KINDS.items()}.get(self.kind, str(self.kind))

    def info(self):
        return {"kind": self.name, "fov_deg": self.fov_deg, "vfov_deg": self.vfov_deg}


def projection_default(kind):
    """rrt_projection_default: the documented defaults of a kind ("pinhole" | "equirect" | "fisheye" or RRT_PROJ_*)"""
    return Projection(kind)


def projection_ray(projection, w, h, x, y, cam):
    """(unit direction as float32[3], inside) of virtual pixel (x, y) of a w x h frame (rrt_projection_ray, host only): the
    primary ray before any nudge, from the source the panorama kernel runs; a fisheye pixel outside the disc is (0, 0, 0), False"""
    d, inside = (C.c_float * 3)(), C.c_int(0)
    _call("rrt_projection_ray", C.byref(projection), w, h, x, y, C.byref(cam), C.byref(d), C.byref(inside))
    return np.array(d[:], np.float32), bool(inside.value)


STEREO_TOP_BOTTOM, STEREO_SIDE_BY_SIDE = 1, 2            # include/rrt.h: RRT_STEREO_*
STEREO_LAYOUTS = {"top-bottom": STEREO_TOP_BOTTOM, "side-by-side": STEREO_SIDE_BY_SIDE}
EYE_LEFT, EYE_RIGHT = 0, 1                                # RRT_EYE_*


class Stereo(rrt_stereo):
    """A stereo pair (include/rrt.h: rrt_stereo): layout "top-bottom" | "side-by-side" (or RRT_STEREO_*), base (interaxial
    distance in scene units), convergence (pinhole: the zero-parallax distance, 0 = parallel axes) and pole_merge = (from, to) in
    degrees of latitude (equirect: the eye separation fades to 0 between them; (90, 90) = no fade).  Defaults ==
    rrt_stereo_default(layout); the values are checked by the calls that use them.  Width and height stay PER EYE everywhere."""

    def __init__(self, layout="top-bottom", base=None, convergence=None, pole_merge=None):
        super().__init__()
        k = STEREO_LAYOUTS.get(layout, layout)
        if not isinstance(k, int):
            raise ValueError(f"stereo layout: one of {sorted(STEREO_LAYOUTS)}, got {layout!r}")
        _call("rrt_stereo_default", k, C.byref(self))
        if base is not None:
            self.base = float(base)
        if convergence is not None:
            self.convergence = float(convergence)
        if pole_merge is not None:
            self.pole_merge_from_deg, self.pole_merge_to_deg = (float(v) for v in pole_merge)

    @property
    def name(self):
        return {v: k for k, v in STEREO_LAYOUTS.items()}.get(self.layout, str(self.layout))

    def composite(self, w, h):
        """(width, height) of the composite frame of w x h eyes"""
        return (2 * w, h) if self.layout == STEREO_SIDE_BY_SIDE else (w, 2 * h)

    def info(self):
        return {"layout": self.name, "base": self.base, "convergence": self.convergence,
                "pole_merge_deg": [self.pole_merge_from_deg, self.pole_merge_to_deg]}


def stereo_default(layout):
    """rrt_stereo_default: base 1, convergence 0, pole merge (90, 90) for a layout ("top-bottom" | "side-by-side" or RRT_STEREO_*)"""
    return Stereo(layout)


def stereo_ray(projection, stereo, w, h, eye, x, y, cam):
    """(origin, unit direction, inside) as float32[3], float32[3], bool of eye `eye`'s (0 left, 1 right) virtual pixel (x, y) of a
    w x h eye frame (rrt_stereo_ray, host only): the primary ray before any nudge, from the source the stereo kernel runs; the
    pinhole's direction without the lens"""
    o, d, inside = (C.c_float * 3)(), (C.c_float * 3)(), C.c_int(0)
    _call("rrt_stereo_ray", C.byref(projection), C.byref(stereo), w, h, eye, x, y, C.byref(cam), C.byref(o), C.byref(d), C.byref(inside))
    return np.array(o[:], np.float32), np.array(d[:], np.float32), bool(inside.value)


class SkyTexture(_lib.Handle):
    """Device-resident RGBA8 equirectangular sky; stands in for the reference's
    cudaTextureObject_t (src/main.cpp:237-266)."""
    _destroy, _id = "rrt_sky_destroy", "handle"

    def __init__(self, rgba8):
        arr = np.ascontiguousarray(rgba8, dtype=np.uint8)
        if arr.ndim != 3 or arr.shape[2] != 4:
            raise ValueError("sky must be an (H, W, 4) uint8 array")
        self.height, self.width = arr.shape[:2]
        h = C.c_ulonglong(0)
        self._create("rrt_sky_create", arr.ctypes.data_as(C.c_void_p), self.width, self.height, C.byref(h))
        self.handle = h.value


class Workspace(_lib.Handle):
    """Caller-owned HBM pool for the three-pass path (RenderParams.workspace = ws.id)."""
    _destroy = "rrt_workspace_destroy"

    def __init__(self, nbytes):
        i = C.c_int(0)
        self._create("rrt_workspace_create", int(nbytes), C.byref(i))
        self.id, self.nbytes = i.value, int(nbytes)

    def stats(self):
        """Of the last launch (synchronous): rows pooled over all its rounds, wavefronts still suspended after the last
        round (finished in line), rounds enqueued / with work, rows of the fullest round, rows the pool holds at most."""
        rows, ovf = C.c_uint(0), C.c_uint(0)
        self._call("rrt_workspace_stats", self.id, C.byref(rows), C.byref(ovf))
        a, b, c, d = C.c_uint(0), C.c_uint(0), C.c_uint(0), C.c_uint(0)
        self._call("rrt_workspace_rounds", self.id, C.byref(a), C.byref(b), C.byref(c), C.byref(d))
        return {"rows_used": rows.value, "overflow_waves": ovf.value, "rounds_enqueued": a.value, "rounds_with_work": b.value,
                "peak_rows": c.value, "pool_rows": d.value}


class TileOrder(_lib.Handle):
    """Cost-ordered dispatch (RenderParams.tile_order = order.id): a launch through the object records what every 8x8-pixel
    wave tile cost, and the next launch with the same geometry dispatches longest-first.  Same pixels; removes the drain
    of views whose long rays are not in the middle of the frame.  Launches through one object are serialised on the
    device: frames that should overlap need one each."""
    # the object must be destroyed under the device that owns it (include/rrt.h); a refused destroy frees nothing and keeps the
    # handle valid, so the status is NOT ignored here: the wrapper keeps its id and the caller hears of it
    _destroy, _destroy_checked = "rrt_tile_order_destroy", True

    def __init__(self):
        i = C.c_int(0)
        self._create("rrt_tile_order_create", C.byref(i))
        self.id = i.value

    def info(self, arrays=False):
        """{"launches", "ordered_launches", "n_tiles"}; with arrays=True also "perm" (the order the next matching launch
        will use) and "cost" (shader clocks / 16 per wave tile of the last launch) as numpy arrays (synchronises)."""
        a, b, n = C.c_ulonglong(0), C.c_ulonglong(0), C.c_uint(0)
        self._call("rrt_tile_order_info", self.id, C.byref(a), C.byref(b), C.byref(n), None, None, 0)
        out = {"launches": a.value, "ordered_launches": b.value, "n_tiles": n.value}
        if arrays and n.value:
            perm = np.empty(n.value, np.uint32); cost = np.empty(n.value, np.uint32)
            self._call("rrt_tile_order_info", self.id, None, None, None, perm.ctypes.data, cost.ctypes.data, n.value)
            out["perm"], out["cost"] = perm, cost
        return out

    def set_seeding(self, on):
        """on (default): a launch without history for its geometry takes its order from a coarse probe of the view."""
        self._call("rrt_tile_order_set_seeding", self.id, 1 if on else 0)

    def seeded_launches(self):
        n = C.c_ulonglong(0)
        self._call("rrt_tile_order_seeded", self.id, C.byref(n))
        return n.value


class TileMap(_lib.Handle):
    """Explicit tile -> shard assignment (cost-weighted instead of t mod n_shards).  shard_of_tile[t] for
    every row tile t of `tile_rows` image rows; device-resident, tied to the current device."""
    _destroy, _destroy_checked = "rrt_tile_map_destroy", True       # as TileOrder

    def __init__(self, height, tile_rows, n_shards, shard_of_tile):
        m = np.ascontiguousarray(shard_of_tile, dtype=np.int32)
        if m.shape != ((height + tile_rows - 1) // tile_rows,):
            raise ValueError("shard_of_tile must have one entry per row tile")
        i = C.c_int(0)
        self._create("rrt_tile_map_create", height, tile_rows, n_shards, m.ctypes.data, C.byref(i))
        self.id, self.height, self.tile_rows, self.n_shards, self.shard_of_tile = i.value, height, tile_rows, n_shards, m

    def shard_rows(self, shard):
        r = C.c_int(0)
        self._call("rrt_tile_map_shard_rows", self.id, shard, C.byref(r), None)
        return r.value

    def max_shard_rows(self):
        r = C.c_int(0)
        self._call("rrt_tile_map_shard_rows", self.id, 0, None, C.byref(r))
        return r.value


def probe_tile_costs(w, h, tile_rows, time, cam, effects, params=None, stream=None):
    """Estimated cost of every row tile from the coarse march-only probe of the view (synchronous; float32 array)."""
    n = (h + tile_rows - 1) // tile_rows
    out = np.zeros(n, np.float32)
    _call("rrt_probe_tile_costs", w, h, tile_rows, float(time), C.byref(cam), C.byref(effects), _ref(params),
          out.ctypes.data, n, _stream(stream))
    return out


def balance_tiles(tile_cost, n_shards, max_tiles_per_shard=0):
    """rrt_tile_map_balance: tiles dealt longest-first to the least loaded shard (deterministic host arithmetic)."""
    c = np.ascontiguousarray(tile_cost, dtype=np.float32)
    out = np.zeros(len(c), np.int32)
    _call("rrt_tile_map_balance", len(c), c.ctypes.data, n_shards, max_tiles_per_shard, out.ctypes.data)
    return out


def clock_probe(d_counters2, duration_us, stream=None):
    """rrt_clock_probe, asynchronous: one wavefront sleeps `duration_us` on `stream` and leaves the shader-clock and
    100 MHz counter deltas in d_counters2 (two int64): d[0] / d[1] * 0.1 = GHz held over that time."""
    _call("rrt_clock_probe", _ptr(d_counters2), int(duration_us), _stream(stream))


def clock_probe_ghz(duration_us=20000, stream=None):
    """The shader clock the chip holds right now (GHz): rrt_clock_probe on `stream` (default: a side stream, so that it
    runs BESIDE whatever the current stream is busy with), synchronous."""
    import torch
    buf = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = stream if stream is not None else torch.cuda.Stream()
    clock_probe(buf, duration_us, st)
    st.synchronize()
    c = buf.cpu().numpy()
    return float(c[0]) / max(float(c[1]), 1.0) * 0.1


TABLE_FULL, TABLE_COARSE, TABLE_COARSEST = 0, 1, 2      # rrt.h: which noise call families a table serves
TABLE_BANDED, TABLE_DENSE = 16, 32                        # ... ORed in: force a layout of the dust families (default: automatic)


class NoiseTable(_lib.Handle):
    """Caller-owned lattice-hash tables for the volumetric noise (RenderParams.noise_table = nt.id): hash31 of every
    lattice point the table-served noise3D calls can reach for t0 <= time <= t1 (NoiseTable(t_max) = [0, t_max]).
    A launch whose time lies outside the window renders with the arithmetic kernels: same bytes, slower."""
    _destroy = "rrt_noise_table_destroy"

    def __init__(self, t_max=32.0, t0=0.0, coverage=TABLE_FULL):
        i = C.c_int(0)
        self._create("rrt_noise_table_create_window", float(t0), float(t_max), int(coverage), C.byref(i))
        self.id, self.t0, self.t1, self.t_max, self.coverage = i.value, float(t0), float(t_max), float(t_max), int(coverage)

    @classmethod
    def window(cls, t0, t1, coverage=TABLE_FULL):
        return cls(t_max=t1, t0=t0, coverage=coverage)

    def covers(self, time):
        return self.t0 <= time <= self.t1

    def info(self):
        t, b, box = C.c_float(0), C.c_size_t(0), (C.c_int * 12)()
        self._call("rrt_noise_table_info", self.id, C.byref(t), C.byref(b), C.byref(box))
        t0, t1, cov, dev = C.c_float(0), C.c_float(0), C.c_int(0), C.c_int(0)
        self._call("rrt_noise_table_window", self.id, C.byref(t0), C.byref(t1), C.byref(cov), C.byref(dev))
        return {"t_max": t.value, "t0": t0.value, "t1": t1.value, "coverage": cov.value, "device": dev.value,
                "bytes": b.value, "accretion_box": list(box[:6]), "dust_box": list(box[6:])}

    @staticmethod
    def plan(t_max, t0=0.0, coverage=TABLE_FULL):
        """Host arithmetic only: size and boxes of such a table; raises RRTError(INVALID_ARGUMENT) for a box that
        create would refuse as well."""
        b, box = C.c_size_t(0), (C.c_int * 12)()
        _call("rrt_noise_table_plan_window", float(t0), float(t_max), int(coverage), C.byref(b), C.byref(box))
        return {"t_max": float(t_max), "t0": float(t0), "coverage": int(coverage), "bytes": b.value,
                "accretion_box": list(box[:6]), "dust_box": list(box[6:])}

    @staticmethod
    def plan_layout(t_max, t0=0.0, coverage=TABLE_FULL):
        """Host arithmetic only: {"banded": bool} and, for a banded table, "n_bands", "w_min", "w_scale", "band_boxes"
        (3, n_bands, 6) -- ridge octave 1, ridge octave 2, detail octave -- and "acc_octave_boxes" (4, 6)."""
        banded, nb, w0, ws = C.c_int(0), C.c_int(0), C.c_float(0), C.c_float(0)
        boxes = np.zeros((3, 64, 6), np.int32); acc = np.zeros((4, 6), np.int32)
        _call("rrt_noise_table_plan_layout", float(t0), float(t_max), int(coverage), C.byref(banded), C.byref(nb), C.byref(w0),
              C.byref(ws), boxes.ctypes.data, 64, acc.ctypes.data)
        if not banded.value:
            return {"banded": False}
        return {"banded": True, "n_bands": nb.value, "w_min": w0.value, "w_scale": ws.value,
                "band_boxes": boxes[:, :nb.value].copy(), "acc_octave_boxes": acc}

    @staticmethod
    def fit(t_from, t_until, budget_bytes):
        """The frame drivers' policy (rrt_noise_table_fit_window): longest window from t_from, richest coverage,
        within the byte budget -> (t1, coverage, bytes); bytes == 0: nothing fits."""
        t1, cov, b = C.c_float(0), C.c_int(0), C.c_size_t(0)
        _call("rrt_noise_table_fit_window", float(t_from), float(t_until), int(budget_bytes), C.byref(t1), C.byref(cov), C.byref(b))
        return t1.value, cov.value, b.value


class NoiseWindows:
    """What a frame loop does about the noise tables as the clock runs (src/main.cpp:515 lets simTime grow without
    bound): keeps ONE table whose window holds the current frame time, within a byte budget; when the clock leaves
    the window it builds the next one (a few milliseconds) -- after `sync()`, since frames in flight may still read
    the old table.  `table_id(t)` is what goes into RenderParams.noise_table (0: this frame hashes arithmetically;
    counted in `arith_frames`, never silent)."""

    def __init__(self, t_end, budget_bytes, sync=None, enabled=True):
        self.t_end, self.budget, self.sync, self.enabled = float(t_end), int(budget_bytes), sync, enabled
        self.table = None
        self.failed = None          # (t0, t1) of a window that could not be built: frames in it hash arithmetically, no retry
        self.retry_after = 5.0
        self.builds, self.table_frames, self.arith_frames, self.coarsest = 0, 0, 0, TABLE_FULL
        self.peak_bytes = 0

    def table_id(self, t):
        if not self.enabled:
            return 0
        # a window that could not be built (nothing fits the budget; out of memory) is REMEMBERED: no new fit, no device
        # synchronise and no retry until the clock has left it -- retrying every frame serialised the frames in flight for
        # the rest of the run
        if self.failed is not None and self.failed[0] <= t <= self.failed[1]:
            self.arith_frames += 1
            return 0
        if self.table is None or not self.table.covers(t):
            t1, cov, nbytes = NoiseTable.fit(t, max(t, self.t_end), self.budget)
            if self.sync:
                self.sync()
            if self.table is not None:
                self.table.destroy()
                self.table = None
            self.failed = None
            if nbytes:
                try:
                    self.table = NoiseTable.window(t, t1, cov)
                    self.builds += 1
                    self.coarsest = max(self.coarsest, cov)
                    self.peak_bytes = max(self.peak_bytes, nbytes)
                except _lib.RRTError as e:          # e.g. out of memory: warn once, carry on without
                    self.failed = (t, t1)
                    if not getattr(self, "_warned", False):
                        print(f"noise table [{t:g}, {t1:g}] not built ({e}); hashing arithmetically", flush=True)
                        self._warned = True
            else:
                self.failed = (t, t + self.retry_after)      # nothing fits: look again after retry_after seconds of sim time
        if self.table is not None and self.table.covers(t):
            self.table_frames += 1
            return self.table.id
        self.arith_frames += 1
        return 0

    def summary(self):
        return {"builds": self.builds, "table_frames": self.table_frames, "arith_frames": self.arith_frames,
                "coarsest_coverage": self.coarsest, "peak_bytes": self.peak_bytes, "budget_bytes": self.budget}

    def close(self):
        if self.table is not None:
            self.table.destroy()
            self.table = None


def set_launch_defaults(params):
    """Parameters of the reference-signature C++ entry point launch_raymarch() (None: config.h defaults)."""
    _call("rrt_set_launch_defaults", _ref(params))


def get_launch_defaults():
    out = RenderParams()
    _call("rrt_get_launch_defaults_sized", C.byref(out), C.sizeof(rrt_params))
    return out


def march_cache_configure(max_bytes, device=-1):
    """Byte budget of a device's march cache (retained geodesics of a still camera, include/rrt.h); 0 switches it off.
    device -1: the current one."""
    _call("rrt_march_cache_configure", int(device), int(max_bytes))


_MARCH_CACHE_STATES = ("none", "seen", "fill-pending", "refill", "ready", "uncacheable")
_MARCH_CACHE_WHY = ("", "budget", "overflow", "allocation")


def march_cache_stats(device=-1):
    """Counters of a device's march cache: which path its launches took (fills / hits / drops / misses / uncacheable), memory."""
    info = _lib.rrt_march_cache_info()
    _call("rrt_march_cache_stats", int(device), C.byref(info))
    d = {k: int(getattr(info, k)) for k, _ in info._fields_}
    d["state"] = _MARCH_CACHE_STATES[info.state] if 0 <= info.state < len(_MARCH_CACHE_STATES) else str(info.state)
    d["why"] = _MARCH_CACHE_WHY[info.why] if 0 <= info.why < len(_MARCH_CACHE_WHY) else str(info.why)
    return d


def march_cache_release(device=-1):
    """Free a device's march cache and forget its key (counters and budget stay)."""
    _call("rrt_march_cache_release", int(device))


def _sky_handle(sky):
    return sky.handle if isinstance(sky, SkyTexture) else int(sky)


def _scene(skyboxTex, effects, params, stream):
    """the arguments every ray launch ends with: sky handle, effects, parameters (may be None), stream"""
    return _sky_handle(skyboxTex), C.byref(effects), _ref(params), _stream(stream)


def abi_version():
    return _lib.load().rrt_abi_version()


def device_count():
    n = C.c_int(0)
    _lib.load().rrt_device_count(C.byref(n))
    return n.value


def launch_raymarch(d_out, w, h, time, cam, skyboxTex, effects, params=None, stream=None):
    """Drop-in for the reference's launch_raymarch (include/raymarcher.h:19): asynchronous,
    writes w*h RGBA8 pixels (bottom-up rows, alpha 255) to the device buffer `d_out`."""
    _call("rrt_launch_raymarch", _ptr(d_out), w, h, float(time), C.byref(cam), *_scene(skyboxTex, effects, params, stream))


def launch_raymarch_rows(d_out_rows, w, h, y0, y1, time, cam, skyboxTex, effects, params=None, stream=None):
    _call("rrt_launch_raymarch_rows", _ptr(d_out_rows), w, h, y0, y1, float(time), C.byref(cam),
          *_scene(skyboxTex, effects, params, stream))


def launch_raymarch_tiles(d_out_tiles, w, h, tile_rows, shard, n_shards, time, cam, skyboxTex, effects,
                          params=None, stream=None):
    _call("rrt_launch_raymarch_tiles", _ptr(d_out_tiles), w, h, tile_rows, shard, n_shards, float(time), C.byref(cam),
          *_scene(skyboxTex, effects, params, stream))


# ---- the sampled launches: five kinds (ss, mb, dof, pano, stereo), each as a whole frame and as one shard's row tiles.  An entry
# point is rrt_launch_raymarch_<kind><suffix>(front..., middle..., sky, effects, params, stream): the front says where the pixels go
# (_whole or _tiles, which also give the suffix), the middle is the kind's own description of what is rendered.
def _whole(d_out, hdr, w, h, samples):
    return "", (_ptr(d_out), _ptr(hdr), w, h, samples)


def _tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards):
    return "_tiles", (_ptr(d_out_tiles), w, h, samples, tile_rows, shard, n_shards)


def _launch_sampled(kind, front, middle, skyboxTex, effects, params, stream):
    suffix, front = front
    _call(f"rrt_launch_raymarch_{kind}{suffix}", *front, *middle, *_scene(skyboxTex, effects, params, stream))


def _sub_frames(times, cams):
    """host arrays of the sub-frames' times (float32) and cameras (rrt_camera), for the _mb entry points"""
    times, cams = list(times), list(cams)
    if len(times) != len(cams):
        raise ValueError(f"{len(times)} times but {len(cams)} cameras")
    return (C.c_float * len(times))(*[float(t) for t in times]), (rrt_camera * len(cams))(*cams), len(times)


def _lens_samples(times, cams, lens_xy):
    """_sub_frames plus the host array of the samples' lens points (2 floats each), for the _dof entry points"""
    t, c, n = _sub_frames(times, cams)
    xy = np.ascontiguousarray(lens_xy, dtype=np.float32).reshape(-1)
    if xy.size != 2 * n:
        raise ValueError(f"{n} samples but {xy.size} lens coordinates")
    return t, c, (C.c_float * xy.size)(*xy.tolist()), n


def _mb_middle(times, cams):
    t, c, n = _sub_frames(times, cams)
    return n, t, c


def _dof_middle(times, cams, lens_xy, focus):
    t, c, xy, n = _lens_samples(times, cams, lens_xy)
    return n, t, c, xy, float(focus)


def launch_raymarch_ss(d_out, w, h, samples, time, cam, skyboxTex, effects, params=None, stream=None, hdr=None):
    """samples x samples supersampled w x h frame (include/rrt.h: rrt_launch_raymarch_ss): every pixel is the mean of the
    post-FX HDR of the samples^2 pixels it covers in the (samples w) x (samples h) frame, tone-mapped once; RGBA8, bottom-up.
    `hdr` (optional): a device buffer of w*h*4 float32 that receives the mean HDR, indexed like the frame.  samples in
    {1, 2, 4, 8}; the params' workspace, path_policy, pool_rounds, pass_chains and tile_order are ignored."""
    _launch_sampled("ss", _whole(d_out, hdr, w, h, samples), (float(time), C.byref(cam)), skyboxTex, effects, params, stream)


def launch_raymarch_ss_tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards, time, cam, skyboxTex, effects,
                             params=None, stream=None):
    """The row tiles of `shard` of launch_raymarch_ss's frame, in launch_raymarch_tiles' buffer layout (assemble_tiles /
    assemble_all_tiles serve it unchanged)."""
    _launch_sampled("ss", _tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards), (float(time), C.byref(cam)),
                    skyboxTex, effects, params, stream)


def launch_raymarch_pano(d_out, w, h, samples, projection, time, cam, skyboxTex, effects, params=None, stream=None, hdr=None):
    """samples x samples supersampled w x h panorama (include/rrt.h: rrt_launch_raymarch_pano): launch_raymarch_ss's frame with the
    projection's primary ray (equirect or fisheye; "pinhole" is launch_raymarch_ss itself).  Lens distortion and vignette are
    ignored; a fisheye pixel outside the disc is black.  `hdr` (optional): w*h*4 float32 that receives the mean HDR."""
    _launch_sampled("pano", _whole(d_out, hdr, w, h, samples), (C.byref(projection), float(time), C.byref(cam)),
                    skyboxTex, effects, params, stream)


def launch_raymarch_pano_tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards, projection, time, cam, skyboxTex, effects,
                               params=None, stream=None):
    """The row tiles of `shard` of launch_raymarch_pano's frame, in launch_raymarch_tiles' buffer layout (assemble_tiles /
    assemble_all_tiles serve it unchanged)."""
    _launch_sampled("pano", _tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards),
                    (C.byref(projection), float(time), C.byref(cam)), skyboxTex, effects, params, stream)


def launch_raymarch_stereo(d_out, w, h, samples, projection, stereo, time, cam, skyboxTex, effects, params=None, stream=None,
                           hdr=None):
    """samples x samples supersampled stereo composite of two w x h eyes (include/rrt.h: rrt_launch_raymarch_stereo): top-bottom
    w x 2h (left eye on top as displayed: the upper stored rows) or side-by-side 2w x h (left eye on the left).  projection
    "pinhole" (off-axis pair: launch_raymarch_ss's eyes) or "equirect" (omni-directional stereo: launch_raymarch_pano's eyes).
    `hdr` (optional): the composite's mean HDR, 4 float32 per pixel."""
    _launch_sampled("stereo", _whole(d_out, hdr, w, h, samples), (C.byref(projection), C.byref(stereo), float(time), C.byref(cam)),
                    skyboxTex, effects, params, stream)


def launch_raymarch_stereo_tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards, projection, stereo, time, cam, skyboxTex,
                                 effects, params=None, stream=None):
    """The row tiles of `shard` of launch_raymarch_stereo's composite (tiles of the COMPOSITE's rows), in launch_raymarch_tiles'
    buffer layout: tile_shard_rows / assemble_tiles / assemble_all_tiles serve it given the composite's size."""
    _launch_sampled("stereo", _tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards),
                    (C.byref(projection), C.byref(stereo), float(time), C.byref(cam)), skyboxTex, effects, params, stream)


def launch_raymarch_mb(d_out, w, h, samples, times, cams, skyboxTex, effects, params=None, stream=None, hdr=None):
    """Motion-blurred w x h frame (include/rrt.h: rrt_launch_raymarch_mb): len(times) in {1, 2, 4, 8, 16} sub-frames, sub-frame k
    the samples x samples supersampled frame at (times[k], cams[k]); the pixel is the mean of all their sub-samples' post-FX HDR,
    summed in a fixed pairwise order and tone-mapped once; RGBA8, bottom-up.  `hdr` (optional): w*h*4 float32 for the mean HDR.
    The params' workspace, path_policy, pool_rounds, pass_chains and tile_order are ignored."""
    _launch_sampled("mb", _whole(d_out, hdr, w, h, samples), _mb_middle(times, cams), skyboxTex, effects, params, stream)


def launch_raymarch_mb_tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards, times, cams, skyboxTex, effects,
                             params=None, stream=None):
    """The row tiles of `shard` of launch_raymarch_mb's frame, in launch_raymarch_tiles' buffer layout (assemble_tiles /
    assemble_all_tiles serve it unchanged)."""
    _launch_sampled("mb", _tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards), _mb_middle(times, cams),
                    skyboxTex, effects, params, stream)


def launch_raymarch_dof(d_out, w, h, samples, times, cams, lens_xy, focus, skyboxTex, effects, params=None, stream=None, hdr=None):
    """Depth-of-field w x h frame (include/rrt.h: rrt_launch_raymarch_dof): len(times) in {1, 2, 4, 8, 16} samples, sample k the
    samples x samples supersampled frame at (times[k], cams[k]) seen through the point lens_xy[k] = (lx, ly) of a thin lens
    focused `focus` units along forward (scene units along the camera's right and up; lens_points gives a disc of them); the pixel
    is the mean of all their sub-samples' post-FX HDR, summed in launch_raymarch_mb's order and tone-mapped once; RGBA8, bottom-up.
    All lens points (0, 0) give launch_raymarch_mb's frame.  `hdr` (optional): w*h*4 float32 for the mean HDR.  The params'
    workspace, path_policy, pool_rounds, pass_chains and tile_order are ignored."""
    _launch_sampled("dof", _whole(d_out, hdr, w, h, samples), _dof_middle(times, cams, lens_xy, focus),
                    skyboxTex, effects, params, stream)


def launch_raymarch_dof_tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards, times, cams, lens_xy, focus, skyboxTex,
                              effects, params=None, stream=None):
    """The row tiles of `shard` of launch_raymarch_dof's frame, in launch_raymarch_tiles' buffer layout (assemble_tiles /
    assemble_all_tiles serve it unchanged)."""
    _launch_sampled("dof", _tiles(d_out_tiles, w, h, samples, tile_rows, shard, n_shards), _dof_middle(times, cams, lens_xy, focus),
                    skyboxTex, effects, params, stream)


def _scratch_size(scratch, scratch_bytes, default):
    """bytes of a launch's scratch: an explicit scratch_bytes, else a tensor's own size, else the library's figure (default())"""
    if scratch_bytes is not None:
        return scratch_bytes
    if scratch is None:
        return 0
    return scratch.numel() * scratch.element_size() if hasattr(scratch, "element_size") else default()


def adaptive_scratch_bytes(w, h):
    """bytes of the scratch launch_raymarch_adaptive needs for a w x h frame (rrt_adaptive_scratch_bytes)"""
    n = C.c_size_t(0)
    _call("rrt_adaptive_scratch_bytes", w, h, C.byref(n))
    return n.value


def adaptive_mask(rgba8, adaptive=None):
    """(mask, count) of a stored RGBA8 frame on the host (rrt_adaptive_mask): rgba8 is an (h, w, 4) uint8 array in the frame's
    layout, mask an (h, w) uint8 array of 0 / 1 in the same layout -- from the source the device's mask pass runs."""
    a = np.ascontiguousarray(rgba8, np.uint8)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an (h, w, 4) uint8 frame, got {a.shape}")
    h, w = a.shape[:2]
    ad = adaptive if adaptive is not None else AdaptiveSettings()
    mask, n = np.zeros((h, w), np.uint8), C.c_uint32(0)
    _call("rrt_adaptive_mask", a.ctypes.data_as(C.c_void_p), w, h, C.byref(ad), mask.ctypes.data_as(C.c_void_p), C.byref(n))
    return mask, n.value


def launch_raymarch_adaptive(d_out, w, h, samples, projection, adaptive, time, cam, skyboxTex, effects, scratch, params=None,
                             stream=None, hdr=None, scratch_bytes=None):
    """Adaptively supersampled w x h frame (include/rrt.h: rrt_launch_raymarch_adaptive): launch_raymarch_ss's 1x frame (projection
    None or "pinhole") or launch_raymarch_pano's, with the pixels that differ from a 4-neighbour by more than adaptive.threshold
    replaced by their samples x samples values -- out = where(mask, ss, base), bit for bit.  `scratch`: device memory of
    adaptive_scratch_bytes(w, h) bytes or more (its size is a tensor's own, or scratch_bytes for a raw pointer); after the launch
    its first uint32 is the number of refined pixels and their frame indices follow from byte 16 on.  `hdr` (optional): w*h*4
    float32 that receives the frame's HDR.  Nothing synchronises."""
    nbytes = _scratch_size(scratch, scratch_bytes, lambda: adaptive_scratch_bytes(w, h))
    _call("rrt_launch_raymarch_adaptive", _ptr(d_out), _ptr(hdr), w, h, samples, _ref(projection), C.byref(adaptive), float(time),
          C.byref(cam), _sky_handle(skyboxTex), C.byref(effects), _ref(params), _ptr(scratch), nbytes, _stream(stream))


def launch_projection_map(d_dirs, w, h, projection, cam, stream=None):
    """every pixel's primary ray on the device (rrt_launch_projection_map): d_dirs (w*h*4 float32, 16-byte aligned) receives
    (dir, 1 inside / 0 outside the fisheye disc) per pixel in the frame's bottom-up layout -- projection_ray's bits"""
    _call("rrt_launch_projection_map", _ptr(d_dirs), w, h, C.byref(projection), C.byref(cam), _stream(stream))


def lens_ray(w, h, x, y, cam, lx, ly, focus):
    """(origin, unit direction) as float32[3] each of virtual pixel (x, y) of a w x h frame through the lens point (lx, ly) of a
    thin lens focused at `focus` (rrt_lens_ray, host only): the primary ray before any nudge and without the lens distortion, from
    the source the depth-of-field kernel runs"""
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    _call("rrt_lens_ray", w, h, x, y, C.byref(cam), float(lx), float(ly), float(focus), C.byref(o), C.byref(d))
    return np.array(o[:], np.float32), np.array(d[:], np.float32)


def lens_points(aperture, n_samples, rotation=0.0):
    """(n_samples, 2) float32 lens points on a disc of radius `aperture` (rrt_lens_points, host only): (0, 0) for one sample,
    otherwise Vogel's spiral turned by `rotation` radians"""
    out = np.zeros((max(int(n_samples), 1), 2), np.float32)
    _call("rrt_lens_points", float(aperture), int(n_samples), float(rotation), out.ctypes.data_as(C.POINTER(C.c_float)))
    return out


def glow_weights(glow, height, lobe):
    """lobe `lobe`'s taps for a frame `height` rows high (rrt_glow_weights): float32 array of 2 R + 1 weights, tap k at [k + R]"""
    r = C.c_int(0)
    _call("rrt_glow_weights", C.byref(glow), height, lobe, None, 0, C.byref(r))
    out = np.zeros(2 * r.value + 1, np.float32)
    _call("rrt_glow_weights", C.byref(glow), height, lobe, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(r))
    return out


def glow_scratch_bytes(w, h, glow):
    n = C.c_size_t(0)
    _call("rrt_glow_scratch_bytes", w, h, C.byref(glow), C.byref(n))
    return n.value


def launch_glow(d_out, hdr, w, h, glow, scratch, stream=None, scratch_bytes=None):
    """The glowed RGBA8 frame (include/rrt.h: rrt_launch_glow) of `hdr` (w*h*4 float32 on the device, the layout launch_raymarch_ss
    / launch_raymarch_mb write) into d_out (w*h*4 uint8).  `scratch`: device memory of glow_scratch_bytes(w, h, glow) bytes or
    more -- its size is a tensor's own, or scratch_bytes for a raw pointer."""
    nbytes = _scratch_size(scratch, scratch_bytes, lambda: glow_scratch_bytes(w, h, glow))
    _call("rrt_launch_glow", _ptr(d_out), _ptr(hdr), w, h, C.byref(glow), _ptr(scratch), nbytes, _stream(stream))


def exposure_scratch_bytes():
    """bytes of the scratch an auto launch_exposure needs (rrt_exposure_scratch_bytes): the histogram at EXPOSURE_HIST_OFFSET, the
    state (float ev, uint32 frames, float scale, float target, uint64 N, double m) at EXPOSURE_STATE_OFFSET, the bin centres at
    EXPOSURE_TABLE_OFFSET"""
    n = C.c_size_t(0)
    _call("rrt_exposure_scratch_bytes", C.byref(n))
    return n.value


def exposure_bin_ev(b):
    """bin b's centre in log2 units, a Python float (rrt_exposure_bin_ev, host only)"""
    v = C.c_double(0.0)
    _call("rrt_exposure_bin_ev", int(b), C.byref(v))
    return v.value


def exposure_adapt(dt, tau):
    """the adapt factor (float32) of a time constant tau at a frame interval dt: (float)(1 - exp(-dt / tau)), 1 for tau == 0
    (rrt_exposure_adapt, host only)"""
    a = C.c_float(0.0)
    _call("rrt_exposure_adapt", float(dt), float(tau), C.byref(a))
    return np.float32(a.value)


def exposure_meter_host(hdr):
    """the 256-bin log-luminance histogram (uint32) of an (h, w, 4) float32 frame on the host (rrt_exposure_meter_host): from the
    source the device's meter pass runs"""
    a = np.ascontiguousarray(hdr, np.float32)
    if a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"expected an (h, w, 4) float32 frame, got {a.shape}")
    hist = np.zeros(256, np.uint32)
    _call("rrt_exposure_meter_host", a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0], hist.ctypes.data_as(C.c_void_p))
    return hist


def launch_exposure_reset(scratch, stream=None, scratch_bytes=None):
    """zero the exposure state in `scratch` (device memory of exposure_scratch_bytes() bytes or more) and load the bin centres
    (rrt_launch_exposure_reset): once before the first auto launch_exposure, and again to start a sequence over"""
    _call("rrt_launch_exposure_reset", _ptr(scratch), _scratch_size(scratch, scratch_bytes, exposure_scratch_bytes), _stream(stream))


def launch_exposure(d_out, hdr_out, hdr_in, w, h, exposure, scratch=None, stream=None, scratch_bytes=None):
    """The exposed frame of `hdr_in` (include/rrt.h: rrt_launch_exposure; w*h*4 float32 on the device, as the sampled launches write
    it): hdr_in.rgb * 2^ev tone-mapped into d_out (w*h*4 uint8, may be None) and / or as linear HDR into hdr_out (may be None, may
    be hdr_in: in place -- launch_glow's input).  Manual mode takes the EV from the settings; auto mode meters the frame and adapts
    the EV kept in `scratch` (launch_exposure_reset first), all on the device.  Nothing synchronises."""
    _call("rrt_launch_exposure", _ptr(d_out), _ptr(hdr_out), _ptr(hdr_in), w, h, C.byref(exposure), _ptr(scratch),
          _scratch_size(scratch, scratch_bytes, exposure_scratch_bytes), _stream(stream))


def tile_shard_rows(h, tile_rows, shard, n_shards):
    rows = C.c_int(0)
    _call("rrt_tile_shard_rows", h, tile_rows, shard, n_shards, C.byref(rows))
    return rows.value


def assemble_tiles(d_frame, d_tiles, w, h, tile_rows, shard, n_shards, stream=None):
    _call("rrt_assemble_tiles", _ptr(d_frame), _ptr(d_tiles), w, h, tile_rows, shard, n_shards, _stream(stream))


def assemble_all_tiles(d_frame, d_tiles_all, shard_stride_bytes, w, h, tile_rows, n_shards, stream=None):
    _call("rrt_assemble_all_tiles", _ptr(d_frame), _ptr(d_tiles_all), shard_stride_bytes, w, h, tile_rows, n_shards, _stream(stream))


def _tile_map_id(tile_map):
    return tile_map.id if isinstance(tile_map, TileMap) else int(tile_map)


def launch_raymarch_tilemap(d_out_tiles, w, h, tile_map, shard, time, cam, skyboxTex, effects, params=None, stream=None):
    _call("rrt_launch_raymarch_tilemap", _ptr(d_out_tiles), w, h, _tile_map_id(tile_map), shard, float(time), C.byref(cam),
          *_scene(skyboxTex, effects, params, stream))


def assemble_all_tilemap(d_frame, d_tiles_all, shard_stride_bytes, w, h, tile_map, stream=None):
    _call("rrt_assemble_all_tilemap", _ptr(d_frame), _ptr(d_tiles_all), shard_stride_bytes, w, h, _tile_map_id(tile_map),
          _stream(stream))


def launch_raymarch_debug(d_out, w, h, time, cam, skyboxTex, effects, params=None, stream=None, **outs):
    """Full-frame launch that also fills per-ray outputs: ldr, hdr, steps, hit, pos, vel, rad (+ lut_oob, one
    uint32 counter of out-of-box noise-table reads)."""
    dbg = rrt_debug_outputs()
    for k, v in outs.items():
        setattr(dbg, "d_" + k, _ptr(v).value if v is not None else None)
    _call("rrt_launch_raymarch_ex", _ptr(d_out), w, h, float(time), C.byref(cam), _sky_handle(skyboxTex), C.byref(effects),
          _ref(params), C.byref(dbg), _stream(stream))


# Y'CbCr packing for Y4M output: a library of its own (include/rrt_yuv.h, librrt_yuv.so), loaded on first use
from . import yuv  # noqa: E402
from .yuv import (YuvFormat, launch_yuv_from_hdr, launch_yuv_from_rgba8, y4m_header, yuv_coefficients,  # noqa: E402,F401
                  yuv_frame_bytes, yuv_from_hdr_host, yuv_from_rgba8_host, yuv_launch_geometry)
from .yuv import (Hdr10Settings, launch_yuv_hdr10_from_hdr, launch_yuv_hdr10_light_reset, y4m_hdr10_sidecar,  # noqa: E402,F401
                  yuv_hdr10_coefficients, yuv_hdr10_from_hdr_host, yuv_hdr10_light_bytes, yuv_hdr10_light_levels)

__all__ += yuv.__all__

# OpenEXR chunk packing for scene-linear output: a library of its own (include/rrt_exr.h, librrt_exr.so), loaded on first use
from . import exr  # noqa: E402
from .exr import (ExrFormat, exr_chunks, exr_frame_bytes, exr_from_hdr_host, exr_header, exr_launch_geometry,  # noqa: E402,F401
                  exr_unfilter_host, launch_exr_from_hdr)
from .exr import (ExrLayers, exr_layers_chunks, exr_layers_frame_bytes, exr_layers_header, exr_layers_host,  # noqa: E402,F401
                  exr_layers_launch_geometry, launch_exr_layers)

__all__ += exr.__all__
# PNG scanline filtering for still-image output: a library of its own (include/rrt_png.h, librrt_png.so), loaded on first use
from . import png  # noqa: E402
from .png import (PngFormat, launch_png_from_hdr, launch_png_from_rgba8, png_adler32, png_frame_bytes, png_from_hdr_host,  # noqa: E402,F401
                  png_from_rgba8_host, png_header, png_launch_geometry, png_slices, png_unfilter_host)
__all__ += png.__all__

# deflate streams made on the device: a library of its own (include/rrt_deflate.h, librrt_deflate.so), loaded on first use
from . import deflate  # noqa: E402
from .deflate import deflate_code_lengths, deflate_host, deflate_launch_geometry, deflate_plan, launch_deflate  # noqa: E402,F401
__all__ += deflate.__all__
