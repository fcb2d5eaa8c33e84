"""Headless frame driver: the reference's main loop (src/main.cpp:505-529) without a window.

    python -m relativisticraytracer_amd.headless --width 1920 --height 1080 --spin 0.9 \\
           --path 0 --frames 300 [--out frames.rgba | --out ppm_dir/] [--all-effects] [--supersample 2] [--motion-blur 4 --shutter 0.5]
           [--glow 0.25 [--glow-radius 0.004] [--glow-threshold 1.0] [--glow-lobes 4]]
           [--projection pinhole|equirect|fisheye [--fov DEG] [--vfov DEG]]
           [--stereo top-bottom|side-by-side [--stereo-base B] [--convergence Z] [--pole-merge FROM TO]]
           [--supersample 2 --adaptive [T]]
           [--dof APERTURE [--focus Z|hole] [--dof-samples K]]
           [--exposure EV | --auto-exposure [KEY]] [--exposure-speed UP DOWN] [--exposure-range MIN MAX] [--exposure-percentiles LOW HIGH]
           [--y4m x.y4m [--y4m-chroma 420|444] [--y4m-range limited|full] [--y4m-depth 8|10]
                   [--y4m-transfer sdr|pq [--hdr-white NITS] [--hdr-peak NITS] [--hdr-knee F]]]
           [--exr f.%04d.exr [--exr-type half|float] [--exr-compression none|zips|zip] [--exr-level 1..9]
                   [--exr-layers steps,horizon,transmittance,emission,direction,position|all]]
           [--png f.%04d.png [--png-depth 8|16] [--png-filter adaptive|none|sub|up|average|paeth] [--png-level 1..9] [--png-deflate host|device]]
    python -m torch.distributed.run --nproc-per-node 8 -m relativisticraytracer_amd.headless ...

Per frame k = 1..N it does what `main()` does while recording: advance the fixed 1/24 s clock
(float accumulators, main.cpp:511-516), take the camera from the active path
(getInterpolatedState, :176-203) or the fixed start-up camera, render (launch_raymarch, :467),
hand the pixels to the sink (captureFrame, :85-97).  With several ranks every frame is
row-tile sharded and gathered to rank 0 (sharding.FrameSharder).  Prints one JSON line of metrics.
"""
import argparse
import json
import math
import os
import sys
import time

import relativisticraytracer_amd as rrt


def _threshold(text):
    """--adaptive's T: a whole number in 0 ... 255, and one message for whatever is not (rrt_headless.cpp's)"""
    try:
        v = int(text)
    except ValueError:
        v = -1
    if not 0 <= v <= 255:
        raise argparse.ArgumentTypeError("a threshold in 0 ... 255 (default 8)")
    return v


def _focus(text):
    """--focus' Z: a finite distance > 0, or `hole` (None: the frame's camera's distance to the origin)"""
    if text == "hole":
        return None
    try:
        v = float(text)
    except ValueError:
        v = 0.0
    if not (math.isfinite(v) and v > 0.0):
        raise argparse.ArgumentTypeError("a distance > 0 along forward, or `hole`")
    return v


def bit_reverse(m, n):
    """m's log2(n) bits in reverse order (n a power of two): the lens point of sample m"""
    r = 0
    while n > 1:
        r, m, n = (r << 1) | (m & 1), m >> 1, n >> 1
    return r


def hole_distance(cam):
    """--focus hole: the camera position's distance to the origin, the double root of the sum of the exact squares in x, y, z
    order, rounded to float (rrt_headless.cpp's)"""
    import numpy as np
    x, y, z = (float(v) for v in cam.as_array()[0])
    return float(np.float32(math.sqrt(x * x + y * y + z * z)))


def build_parser():
    ap = argparse.ArgumentParser(prog="relativisticraytracer_amd.headless")
    ap.add_argument("--width", type=int, default=1000)          # WINDOW_WIDTH, config.h:7
    ap.add_argument("--height", type=int, default=700)          # WINDOW_HEIGHT, config.h:8
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--fps", type=int, default=24)              # RECORDING_FPS, config.h:9
    ap.add_argument("--spin", type=float, default=0.0)          # SPIN_A, config.h:21
    ap.add_argument("--path", type=int, default=-1, help="built-in camera path 0..2; -1 = fixed start-up camera")
    ap.add_argument("--no-volumetrics", action="store_true")
    ap.add_argument("--fast", action="store_true", help="RRT_ARITH_FAST (not the parity path); = --arith fast")
    ap.add_argument("--arith", choices=("strict", "fmad", "fast"), default=None,
                    help="arithmetic of the RK4 step: strict (default; bit-identical to the oracle), fmad (multiply-adds fused, roots and "
                         "divisions correctly rounded: the class of the reference's nvcc-default build), fast (also 1-ulp rsq)")
    ap.add_argument("--path-window", type=int, default=0,
                    help="several frames in flight, a share under the three-pass threshold: frames per window of the per-rank path choice "
                         "(rrt_path_chooser; 0 = 48); -1: no choice, the three-pass path throughout")
    ap.add_argument("--all-effects", action="store_true", help="also enable chromatic aberration (key C)")
    ap.add_argument("--sky", default=None, help="equirectangular image file; default: synthetic sky, seed 1")
    ap.add_argument("--tile-rows", type=int, default=16)
    ap.add_argument("--frames-in-flight", type=int, default=3,
                    help="several ranks: frames rendered / gathered / assembled concurrently per rank (>= 2)")
    ap.add_argument("--workspace-gib", type=int, default=8,
                    help="per-rank pool for the three-pass path, used by launches of <= 1.5 M rays (0 = single kernel only)")
    ap.add_argument("--tile-order", choices=("auto", "on", "off"), default="auto",
                    help="cost-ordered dispatch (rrt_tile_order): every frame's wave tiles go out longest-first by the costs the "
                         "previous frame (of the same slot) measured.  auto: on when frames are rendered one at a time, off when "
                         "several are in flight (their drains already overlap)")
    ap.add_argument("--no-noise-table", action="store_true",
                    help="hash every noise3D corner arithmetically (default: lattice-hash tables over a sliding window of the clock)")
    ap.add_argument("--noise-table-gib", type=float, default=2.0,
                    help="per-GPU byte budget of the noise tables: the window of sim time one table covers (and, for long "
                         "sequences, its coverage) is chosen to fit; the table is rebuilt when the clock leaves the window")
    ap.add_argument("--supersample", type=int, choices=(1, 2, 4, 8), default=1,
                    help="S x S sub-samples per pixel, averaged in HDR before the tone map (rrt_launch_raymarch_ss*; 1 = one ray per "
                         "pixel).  S > 1 always renders with the single kernel in the static order: no pool, path choice or tile order")
    ap.add_argument("--motion-blur", type=int, choices=(1, 2, 4, 8, 16), default=1,
                    help="K sub-frames over the shutter interval, averaged in HDR before the tone map (rrt_launch_raymarch_mb*; 1 = "
                         "one instant per frame).  K > 1 always renders with the single kernel in the static order, as --supersample")
    ap.add_argument("--shutter", type=float, default=0.5,
                    help="with --motion-blur K > 1: the fraction of the frame interval the shutter is open, ending at the frame's "
                         "time (rrt_motion_clock; 0.5 = 180 degrees)")
    ap.add_argument("--glow", type=float, default=None, metavar="INTENSITY",
                    help="HDR glow (rrt_launch_glow) of this intensity on every frame: the frame renders through "
                         "rrt_launch_raymarch_ss / _mb into an HDR buffer, the glow writes its RGBA8.  One GPU only; single kernel, no pool")
    ap.add_argument("--glow-radius", type=float, default=0.004, help="with --glow: the first lobe's sigma as a fraction of the height")
    ap.add_argument("--glow-threshold", type=float, default=1.0, help="with --glow: the bright pass' luma threshold (a soft knee)")
    ap.add_argument("--glow-lobes", type=int, choices=(1, 2, 3, 4), default=4, help="with --glow: Gaussian lobes, each twice as wide")
    ap.add_argument("--projection", choices=("pinhole", "equirect", "fisheye"), default="pinhole",
                    help="the camera: pinhole (the reference's), equirect (360-degree panorama) or fisheye (angular dome master), "
                         "rrt_launch_raymarch_pano*.  A panorama always renders with the single kernel in the static order; not with "
                         "--motion-blur > 1, and an equirect frame not with --glow (the glow does not wrap at the seam)")
    ap.add_argument("--fov", type=float, default=None, metavar="DEG",
                    help="equirect: horizontal span in (0, 360], default 360; fisheye: aperture in (0, 360], default 180")
    ap.add_argument("--vfov", type=float, default=None, metavar="DEG", help="equirect: vertical span in (0, 180], default 180")
    ap.add_argument("--stereo", choices=("top-bottom", "side-by-side"), default=None,
                    help="a stereo pair per frame (rrt_launch_raymarch_stereo*): --width / --height per eye, written as one composite "
                         "(top-bottom: width x 2 height, left eye on top; side-by-side: 2 width x height, left eye on the left).  "
                         "pinhole: off-axis pair; equirect: omni-directional stereo.  Single kernel, static order; not with fisheye, "
                         "--motion-blur > 1 or --glow")
    ap.add_argument("--stereo-base", type=float, default=None, metavar="B",
                    help="with --stereo: the interaxial distance in scene units, >= 0 (default 1)")
    ap.add_argument("--convergence", type=float, default=None, metavar="Z",
                    help="with --stereo, pinhole only: the zero-parallax distance along forward, >= 0 (default 0: parallel axes)")
    ap.add_argument("--pole-merge", type=float, nargs=2, default=None, metavar=("FROM", "TO"),
                    help="with --stereo, equirect only: the eye separation fades to 0 between these latitudes in degrees, "
                         "0 <= FROM <= TO <= 90 (default 90 90: no fade)")
    ap.add_argument("--adaptive", type=_threshold, nargs="?", const=8, default=None, metavar="T",
                    help="with --supersample S > 1: adaptive supersampling (rrt_launch_raymarch_adaptive) -- the 1x frame, and only the "
                         "pixels that differ from a 4-neighbour by more than T (0 ... 255, default 8) in a colour channel are rendered "
                         "S x S.  One GPU only; not with --motion-blur > 1 or --stereo; combines with --projection and --glow")
    ap.add_argument("--dof", type=float, default=None, metavar="APERTURE",
                    help="depth of field (rrt_launch_raymarch_dof*): every frame through K points of a thin lens of this radius in "
                         "scene units (rrt_lens_points), sample m through lens point bitrev_K(m).  Single kernel, static order; "
                         "combines with --supersample, --motion-blur (the K samples are the shutter's sub-frames), --glow and several "
                         "GPUs; pinhole only, not with --stereo or --adaptive")
    ap.add_argument("--focus", type=_focus, default=None, metavar="Z|hole",
                    help="with --dof: the distance of the plane in focus along forward, > 0, or `hole` (default): the distance from "
                         "the frame's camera position to the origin")
    ap.add_argument("--dof-samples", type=int, choices=(1, 2, 4, 8, 16), default=None, metavar="K",
                    help="with --dof: lens samples per sub-sample (default 8); with --motion-blur M > 1 the samples are shared: K = M")
    ap.add_argument("--exposure", type=float, default=None, metavar="EV",
                    help="exposure control (rrt_launch_exposure): the frame renders into an HDR buffer as with --glow and is scaled by "
                         "2^EV before the tone map; with --auto-exposure EV is the compensation.  One GPU only; single kernel, no pool; "
                         "with every frame kind; with --glow the exposure scales the HDR in place and the glow follows")
    ap.add_argument("--auto-exposure", type=float, nargs="?", const=0.5, default=None, metavar="KEY",
                    help="meter every frame's log-luminance histogram on the device and adapt the EV so that the retained pixels' "
                         "log-average lands on KEY (> 0, default 0.5)")
    ap.add_argument("--exposure-speed", type=float, nargs=2, default=None, metavar=("UP", "DOWN"),
                    help="with --auto-exposure: time constants in seconds towards a higher / lower EV, turned into per-frame factors "
                         "with 1 / fps (rrt_exposure_adapt; default 0 0: no smoothing)")
    ap.add_argument("--exposure-range", type=float, nargs=2, default=None, metavar=("MIN", "MAX"),
                    help="with --auto-exposure: the metered EV's range (default -8 8)")
    ap.add_argument("--exposure-percentiles", type=int, nargs=2, default=None, metavar=("LOW", "HIGH"),
                    help="with --auto-exposure: the darkest / brightest share of the metered pixels left out of the average, in per "
                         "mille (default 400 20)")
    ap.add_argument("--out", default=None, help="x.rgba (raw, bottom-up) | dir/ (PPM per frame) | x.mp4 (needs ffmpeg)")
    ap.add_argument("--y4m", default=None, metavar="PATH",
                    help="also (or, without --out, only) write the sequence as a YUV4MPEG2 file: BT.709 Y'CbCr packed on the device "
                         "(include/rrt_yuv.h), top-down, playable as it is")
    # the three below are checked in check_args, not by argparse's `choices`: both drivers word their refusals alike
    ap.add_argument("--y4m-chroma", default=None, metavar="420|444", help="with --y4m: chroma subsampling (default 420)")
    ap.add_argument("--y4m-range", default=None, metavar="limited|full", help="with --y4m: code range (default limited)")
    ap.add_argument("--y4m-depth", default=None, metavar="8|10",
                    help="with --y4m: bits per sample (default 8).  8 converts the finished RGBA8 frame, in every mode; 10 converts the "
                         "frame's linear HDR (the whole-frame HDR path of --exposure): one GPU only, not with --glow")
    ap.add_argument("--y4m-transfer", default=None, metavar="sdr|pq",
                    help="with --y4m: sdr (default) tone-maps into BT.709; pq (with --y4m-depth 10) writes HDR10 -- the linear HDR as "
                         "absolute light behind SMPTE ST 2084, BT.2020 -- and PATH.hdr10.json with MaxCLL / MaxFALL and the encoder options")
    ap.add_argument("--hdr-white", type=float, default=None, metavar="NITS", help="with --y4m-transfer pq: the luminance of H = 1 (default 203)")
    ap.add_argument("--hdr-peak", type=float, default=None, metavar="NITS",
                    help="with --y4m-transfer pq: the highlight shoulder's asymptote and the mastering display's peak (default 1000)")
    ap.add_argument("--hdr-knee", type=float, default=None, metavar="F",
                    help="with --y4m-transfer pq: the shoulder starts at F * peak (default 0.5; 1: a hard clip)")
    ap.add_argument("--exr", default=None, metavar="PATTERN",
                    help="also (or only) write every frame as a scene-linear OpenEXR file (include/rrt_exr.h): the frame's linear HDR -- "
                         "after --exposure / --auto-exposure, before any tone map -- as B, G, R scanlines packed on the device.  "
                         "PATTERN holds one frame field (f.%%04d.exr); a plain name serves --frames 1.  The whole-frame HDR path of "
                         "--exposure: one GPU only, not with --glow")
    # checked in check_exr, not by argparse's `choices` or `type`: both drivers word their refusals alike
    ap.add_argument("--exr-type", default=None, metavar="half|float", help="with --exr: the samples (default half, clamped to +-65504)")
    ap.add_argument("--exr-compression", default=None, metavar="none|zips|zip",
                    help="with --exr: none, or deflate of 1 (zips) or 16 (zip, the default) scanlines per chunk")
    ap.add_argument("--exr-level", default=None, metavar="1..9", help="with --exr: the deflate level (default 4)")
    ap.add_argument("--exr-layers", default=None, metavar="LIST",
                    help="with --exr: per-ray data layers next to B, G, R in every file -- a comma-separated subset of "
                         "steps,horizon,transmittance,emission,direction,position, or all.  The frame is rendered by the debug launch; "
                         "the layers are stored as the march left them (the exposure scales B, G, R only).  The 1x pinhole frame only")
    ap.add_argument("--png", default=None, metavar="PATTERN",
                    help="also (or only) write every frame as a PNG file (include/rrt_png.h): RGB scanlines filtered, scored and summed "
                         "on the device, deflated in slices on a thread pool.  PATTERN holds one frame field (f.%%04d.png); a plain "
                         "name serves --frames 1")
    # checked in check_png, not by argparse's `choices` or `type`: both drivers word their refusals alike
    ap.add_argument("--png-depth", default=None, metavar="8|16",
                    help="with --png: bits per sample (default 8).  8 converts the finished RGBA8 frame, in every mode; 16 tone-maps the "
                         "frame's linear HDR to 16 bits (the whole-frame HDR path of --exposure): one GPU only, not with --glow")
    ap.add_argument("--png-filter", default=None, metavar="adaptive|none|sub|up|average|paeth",
                    help="with --png: the scanline filter -- adaptive (default) scores all five per row and keeps the best")
    ap.add_argument("--png-level", default=None, metavar="1..9", help="with --png: the deflate level (default 4)")
    ap.add_argument("--png-deflate", default=None, metavar="host|device",
                    help="with --png: where the slices are deflated -- host (default): zlib on a thread pool; device: include/rrt_deflate.h, "
                         "Huffman codes and run lengths in HIP behind the filtering launch, so that only finished streams are copied and "
                         "the host's threads stay free (larger files on noiseless frames; not with --png-level, which is zlib's)")
    ap.add_argument("--init-timeout", type=float, default=300.0,
                    help="several ranks: seconds the process-group bring-up may take before the run exits non-zero with "
                         "the tracebacks of all threads, instead of hanging")
    ap.add_argument("--frame-timeout", type=float, default=120.0, help="the same for any single frame (0: no limit)")
    return ap


def check_args(ap, args, world):
    """every refusal that needs neither torch nor the library, in the order that decides which message a command line gets;
    returns pano, use_exposure, dof_k (lens samples per sub-sample; 0: no --dof)"""
    if not 0.0 <= args.shutter <= 1.0:
        ap.error("--shutter: a fraction of the frame interval in [0, 1]")
    # the glow needs the whole frame's HDR on one GPU (no _tiles form); checked before any device is touched
    if args.glow is not None and world > 1:
        ap.error("--glow: one GPU only (WORLD_SIZE > 1)")
    # exposure control needs the whole frame's HDR on one GPU as well (the meter sees every pixel; no _tiles form)
    use_exposure = args.exposure is not None or args.auto_exposure is not None
    if not use_exposure and (args.exposure_speed is not None or args.exposure_range is not None or args.exposure_percentiles is not None):
        ap.error("--exposure-speed / --exposure-range / --exposure-percentiles need --exposure EV | --auto-exposure [KEY]")
    if use_exposure and world > 1:
        ap.error("--exposure / --auto-exposure: one GPU only (WORLD_SIZE > 1)")
    pano = args.projection != "pinhole"
    if not pano and (args.fov is not None or args.vfov is not None):
        ap.error("--fov / --vfov need --projection equirect | fisheye")
    if args.projection == "fisheye" and args.vfov is not None:
        ap.error("--vfov: equirect only (a fisheye's aperture is --fov)")
    if pano and args.motion_blur > 1:
        ap.error("a panorama renders one instant per frame (--motion-blur 1)")
    if args.projection == "equirect" and args.glow is not None:
        ap.error("--glow clamps at the frame's edge and an equirect frame wraps: not with --projection equirect")
    stereo_opts = args.stereo_base is not None or args.convergence is not None or args.pole_merge is not None
    if args.stereo is None and stereo_opts:
        ap.error("--stereo-base / --convergence / --pole-merge need --stereo top-bottom | side-by-side")
    if args.stereo is not None:
        if args.projection == "fisheye":
            ap.error("--stereo: pinhole or equirect (no stereo fisheye domes)")
        if args.motion_blur > 1:
            ap.error("--stereo renders one instant per frame (--motion-blur 1)")
        if args.glow is not None:
            ap.error("--stereo: not with --glow")
        if args.convergence is not None and args.projection != "pinhole":
            ap.error("--convergence: pinhole only")
        if args.pole_merge is not None and args.projection != "equirect":
            ap.error("--pole-merge: equirect only")

    if args.adaptive is not None:       # the whole frame on one GPU (the mask needs every pixel's neighbours); before any device is touched
        if args.supersample <= 1:
            ap.error("--adaptive needs --supersample 2 | 4 | 8")
        if world > 1:
            ap.error("--adaptive: one GPU only (WORLD_SIZE > 1)")
        if args.motion_blur > 1:
            ap.error("--adaptive renders one instant per frame (--motion-blur 1)")
        if args.stereo is not None:
            ap.error("--adaptive: not with --stereo")

    if args.dof is None and (args.focus is not None or args.dof_samples is not None):
        ap.error("--focus / --dof-samples need --dof APERTURE")
    dof_k = 0
    if args.dof is not None:
        if not (math.isfinite(args.dof) and args.dof >= 0.0):
            ap.error("--dof APERTURE: the lens radius in scene units, >= 0")
        if pano:
            ap.error("--dof: a thin lens in front of a pinhole camera, not with --projection equirect | fisheye")
        if args.stereo is not None:
            ap.error("--dof: not with --stereo")
        if args.adaptive is not None:
            ap.error("--dof: not with --adaptive")
        if args.motion_blur > 1 and args.dof_samples not in (None, args.motion_blur):
            ap.error("--dof-samples: with --motion-blur M > 1 the lens samples are the shutter's sub-frames (K = M)")
        dof_k = args.motion_blur if args.motion_blur > 1 else (args.dof_samples or 8)
    check_y4m(ap, args, world)
    check_exr(ap, args, world)
    check_png(ap, args, world)
    return pano, use_exposure, dof_k


def check_y4m(ap, args, world):
    """--y4m's refusals (rrt_headless.cpp words them alike); leaves args.y4m_format: (chroma, range, bits) or None"""
    args.y4m_format = args.y4m_hdr10 = None
    if args.y4m_transfer not in (None, "sdr", "pq"):
        ap.error("--y4m-transfer sdr | pq")
    pq = args.y4m_transfer == "pq"
    if not pq and (args.hdr_white is not None or args.hdr_peak is not None or args.hdr_knee is not None):
        ap.error("--hdr-white / --hdr-peak / --hdr-knee need --y4m-transfer pq")
    if pq and (args.y4m is None or args.y4m_depth != "10"):
        ap.error("--y4m-transfer pq needs --y4m PATH and --y4m-depth 10")
    for v in (args.hdr_white, args.hdr_peak):
        if v is not None and not (math.isfinite(v) and 0.0 < v <= 10000.0):
            ap.error("--hdr-white / --hdr-peak NITS: in (0, 10000]")
    if args.hdr_knee is not None and not 0.0 <= args.hdr_knee <= 1.0:
        ap.error("--hdr-knee F: in [0, 1]")
    if pq:
        args.y4m_hdr10 = (args.hdr_white, args.hdr_peak, args.hdr_knee)
    if args.y4m is None:
        if args.y4m_transfer is not None:
            ap.error("--y4m-transfer needs --y4m PATH")
        if args.y4m_chroma is not None or args.y4m_range is not None or args.y4m_depth is not None:
            ap.error("--y4m-chroma / --y4m-range / --y4m-depth need --y4m PATH")
        return
    if args.y4m_chroma not in (None, "420", "444"):
        ap.error("--y4m-chroma 420 | 444")
    if args.y4m_range not in (None, "limited", "full"):
        ap.error("--y4m-range limited | full")
    if args.y4m_depth not in (None, "8", "10"):
        ap.error("--y4m-depth 8 | 10")
    bits = int(args.y4m_depth or 8)
    if bits == 10:      # the frame's linear HDR, whole, on one GPU
        if args.glow is not None:
            ap.error("--y4m-depth 10 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow")
        if world > 1:
            ap.error("--y4m-depth 10: one GPU only (WORLD_SIZE > 1)")
    if args.out is not None and os.path.abspath(args.y4m) == os.path.abspath(args.out):
        ap.error("--y4m and --out name the same file")
    args.y4m_format = (int(args.y4m_chroma or 420), args.y4m_range or "limited", bits)


def check_exr(ap, args, world):
    """--exr's refusals (rrt_headless.cpp words them alike); leaves args.exr_format: (type, compression, level) or None"""
    from relativisticraytracer_amd.sinks import frame_fields, frame_name
    args.exr_format, args.exr_layer_names = None, ()
    if args.exr is None:
        if args.exr_type is not None or args.exr_compression is not None or args.exr_level is not None:
            ap.error("--exr-type / --exr-compression / --exr-level need --exr PATTERN")
        if args.exr_layers is not None:
            ap.error("--exr-layers needs --exr PATTERN")
        return
    if args.exr_type not in (None, "half", "float"):
        ap.error("--exr-type half | float")
    if args.exr_compression not in (None, "none", "zips", "zip"):
        ap.error("--exr-compression none | zips | zip")
    if args.exr_level not in (None,) + tuple("123456789"):
        ap.error("--exr-level 1 ... 9")
    if args.glow is not None:
        ap.error("--exr reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow")
    if world > 1:
        ap.error("--exr: one GPU only (WORLD_SIZE > 1)")
    fields = frame_fields(args.exr)
    if fields > 1:
        ap.error("--exr PATTERN: one frame field (%d or %0Nd)")
    if fields == 0 and args.frames > 1:
        ap.error("--exr PATTERN needs a frame field (%04d) when --frames > 1: the frames would overwrite one another")
    for other, flag in ((args.out, "--out"), (args.y4m, "--y4m")):
        if other is not None and any(os.path.abspath(frame_name(args.exr, k)) == os.path.abspath(other) for k in range(1, max(args.frames, 1) + 1)):
            ap.error(f"--exr and {flag} name the same file")
    args.exr_format = (args.exr_type or "half", args.exr_compression or "zip", int(args.exr_level or 4))
    if args.exr_layers is not None:
        names = list(EXR_LAYERS) if args.exr_layers == "all" else args.exr_layers.split(",")
        if any(n not in EXR_LAYERS for n in names):
            ap.error("--exr-layers LIST: a comma-separated subset of " + ",".join(EXR_LAYERS) + ", or all")
        if len(set(names)) != len(names):
            ap.error("--exr-layers LIST names a layer twice")
        for on, what in ((args.adaptive is not None, "--adaptive"), (args.dof is not None, "--dof"), (args.stereo is not None, "--stereo"),
                         (args.projection != "pinhole", "--projection equirect | fisheye"), (args.motion_blur > 1, "--motion-blur > 1"),
                         (args.supersample > 1, "--supersample > 1")):
            if on:
                ap.error("--exr-layers stores per-ray data of the 1x pinhole frame: not with " + what)
        args.exr_layer_names = tuple(n for n in EXR_LAYERS if n in names)


def check_png(ap, args, world):
    """--png's refusals (rrt_headless.cpp words them alike); leaves args.png_format: (depth, filter, level) or None"""
    from relativisticraytracer_amd.sinks import frame_fields, frame_name
    args.png_format = None
    if args.png is None:
        if args.png_depth is not None or args.png_filter is not None or args.png_level is not None:
            ap.error("--png-depth / --png-filter / --png-level need --png PATTERN")
        if args.png_deflate is not None:
            ap.error("--png-deflate needs --png PATTERN")
        return
    if args.png_depth not in (None, "8", "16"):
        ap.error("--png-depth 8 | 16")
    if args.png_filter not in (None, "adaptive", "none", "sub", "up", "average", "paeth"):
        ap.error("--png-filter adaptive | none | sub | up | average | paeth")
    if args.png_level not in (None,) + tuple("123456789"):
        ap.error("--png-level 1 ... 9")
    if args.png_deflate not in (None, "host", "device"):
        ap.error("--png-deflate host | device")
    if args.png_deflate == "device" and args.png_level is not None:
        ap.error("--png-level is the host zlib's level: not with --png-deflate device")
    depth = int(args.png_depth or 8)
    if depth == 16:      # the frame's linear HDR, whole, on one GPU
        if args.glow is not None:
            ap.error("--png-depth 16 reads the frame's linear HDR and the glow tone-maps H + glow without storing it: not with --glow")
        if world > 1:
            ap.error("--png-depth 16: one GPU only (WORLD_SIZE > 1)")
    fields = frame_fields(args.png)
    if fields > 1:
        ap.error("--png PATTERN: one frame field (%d or %0Nd)")
    if fields == 0 and args.frames > 1:
        ap.error("--png PATTERN needs a frame field (%04d) when --frames > 1: the frames would overwrite one another")
    for k in range(1, max(args.frames, 1) + 1):
        name = os.path.abspath(frame_name(args.png, k))
        for other, flag in ((args.out, "--out"), (args.y4m, "--y4m"), (frame_name(args.exr, k) if args.exr is not None else None, "--exr")):
            if other is not None and name == os.path.abspath(other):
                ap.error(f"--png and {flag} name the same file")
    args.png_format = (depth, args.png_filter or "adaptive", int(args.png_level or 4))
    args.png_on_device = args.png_deflate == "device"


# --exr-layers' names, in the order `all` lists them, and each one's channels: (name, type -- None: --exr-type's --, plane, word)
EXR_LAYERS = {"steps": [("steps", "uint", "steps", 0)],
              "horizon": [("horizon", "half", "hit", 0)],
              "transmittance": [("transmittance", None, "rad", 3)],
              "emission": [("emission.B", None, "rad", 2), ("emission.G", None, "rad", 1), ("emission.R", None, "rad", 0)],
              "direction": [("direction.X", "float", "vel", 0), ("direction.Y", "float", "vel", 1), ("direction.Z", "float", "vel", 2)],
              "position": [("position.X", "float", "pos", 0), ("position.Y", "float", "pos", 1), ("position.Z", "float", "pos", 2)]}
EXR_PLANES = {"steps": ("int32", 1), "hit": ("int32", 1), "rad": ("float32", 4), "vel": ("float32", 3), "pos": ("float32", 3)}


def exr_layer_list(names, beauty, hdr, planes):
    """ExrLayers' list for B, G, R of type `beauty` from the bottom-up HDR plane and the named layers from the debug launch's
    top-down planes {"steps" | "hit" | "rad" | "vel" | "pos": tensor}"""
    out = [("B", beauty, hdr, 2, True), ("G", beauty, hdr, 1, True), ("R", beauty, hdr, 0, True)]
    for name in names:
        out += [(ch, type_ or beauty, planes[plane], word, False) for ch, type_, plane, word in EXR_LAYERS[name]]
    return out


def build_settings(ap, args, pano, use_exposure):
    """proj, stereo, glow, exposure (None: not asked for), each checked by the library's own host query: the launches' refusals,
    stated before any device is touched"""
    proj = None
    if pano:                        # the spans' checks are the host query's (rrt_projection_ray): the launch's own refusals
        proj = rrt.Projection(args.projection, args.fov, args.vfov)
        try:
            rrt.projection_ray(proj, 1, 1, 0, 0, rrt.CameraState())
        except rrt.RRTError:
            ap.error("--fov DEG in (0, 360], --vfov DEG in (0, 180]")
    stereo = None
    if args.stereo is not None:     # the values' checks are the host query's (rrt_stereo_ray): the launch's own refusals
        stereo = rrt.Stereo(args.stereo, args.stereo_base, args.convergence, args.pole_merge)
        try:
            rrt.stereo_ray(proj if proj is not None else rrt.Projection("pinhole"), stereo, 1, 1, 0, 0, 0, rrt.CameraState())
        except rrt.RRTError:
            ap.error("--stereo-base B >= 0, --convergence Z >= 0, --pole-merge FROM TO with 0 <= FROM <= TO <= 90")
    glow = None
    if args.glow is not None:       # the settings' checks are host arithmetic (rrt_glow_scratch_bytes)
        glow = rrt.GlowSettings(radius=args.glow_radius, lobes=args.glow_lobes, threshold=args.glow_threshold, intensity=args.glow)
        try:
            rrt.glow_scratch_bytes(args.width, args.height, glow)
        except rrt.RRTError:
            ap.error("--glow INTENSITY >= 0, --glow-radius R > 0 (a fraction of the height; widest lobe <= 1024 px), "
                     "--glow-threshold T >= 0")
    exposure = None
    if use_exposure:                # the settings' ranges are rrt_launch_exposure's own refusals
        up, down = args.exposure_speed or (0.0, 0.0)
        lo_ev, hi_ev = args.exposure_range or (-8.0, 8.0)
        low, high = args.exposure_percentiles or (400, 20)
        key = args.auto_exposure if args.auto_exposure is not None else 0.5
        try:
            alphas = [rrt.exposure_adapt(1.0 / args.fps, tau) for tau in (up, down)]
        except rrt.RRTError:
            alphas = [0.0, 0.0]
        ok = all(math.isfinite(v) for v in (args.exposure or 0.0, key, lo_ev, hi_ev)) and key > 0.0 and lo_ev <= hi_ev
        if not (ok and min(alphas) > 0.0 and low >= 0 and high >= 0 and low + high < 1000):
            ap.error("--exposure EV finite, --auto-exposure KEY > 0, --exposure-speed UP DOWN >= 0 (seconds), --exposure-range MIN MAX with "
                     "MIN <= MAX, --exposure-percentiles LOW HIGH >= 0 with LOW + HIGH < 1000")
        exposure = rrt.ExposureSettings(mode="auto" if args.auto_exposure is not None else "manual", ev=args.exposure or 0.0, key=key,
                                        low_permille=low, high_permille=high, min_ev=lo_ev, max_ev=hi_ev,
                                        adapt_up=float(alphas[0]), adapt_down=float(alphas[1]))
    return proj, stereo, glow, exposure


class Renderer:
    """One rank's frames.  What the command line fixes -- sizes, settings, launch parameters per slot, buffers -- is set once in
    __init__; `set_frame` sets the frame that the render methods launch: k, t, cam, table, and times / cams / focus for the kinds
    that sample the shutter or the lens."""

    def __init__(self, args, settings, dof_k, rank, world, dev):
        import torch
        from relativisticraytracer_amd import camera_paths, sharding
        from relativisticraytracer_amd.sky import load_sky, synthetic_sky
        self.args, self.rank, self.world, self.dof_k = args, rank, world, dof_k
        self.proj, self.stereo, self.glow, self.exposure = settings
        proj, stereo, glow, exposure = settings
        self.ew, self.eh = ew, eh = args.width, args.height     # the launch's frame: one eye's with --stereo
        self.w, self.h = w, h = stereo.composite(ew, eh) if stereo is not None else (ew, eh)     # the frame that is sharded, gathered and written
        self.ss, self.mb = ss, mb = args.supersample, args.motion_blur
        self.sampled = proj is not None or mb > 1 or ss > 1 or stereo is not None or dof_k > 0      # launch_sampled's kinds
        self.y4m10 = args.y4m_format is not None and args.y4m_format[2] == 10     # the Y4M frames come from the HDR: its whole-frame path
        self.exr = args.exr_format is not None        # the EXR frames are the HDR itself: the same path
        self.png16 = args.png_format is not None and args.png_format[0] == 16      # the 16-bit PNG frames are tone-mapped from the HDR: the same path
        self.post = glow is not None or exposure is not None or self.y4m10 or self.exr or self.png16
        # supersampled, blurred, glowed, panorama, stereo: single kernel, static order, no pool
        single = self.sampled or self.post
        # sample m looks through lens point bitrev_K(m): the spiral's radius grows with its index, the shutter's times with m
        self.dof_points = rrt.lens_points(args.dof, dof_k)[[bit_reverse(m, dof_k) for m in range(dof_k)]] if dof_k else None
        self.tex = rrt.SkyTexture(load_sky(args.sky) if args.sky else synthetic_sky())
        self.fx = rrt.CameraEffects(useChromaticAberration=bool(args.all_effects))
        # with several ranks --frames-in-flight frames are in flight (FrameSharder pipeline mode), each with its own
        # share of the pool
        self.n_slots = n_slots = max(2, args.frames_in_flight) if world > 1 else 1
        self.pools = pools = ([rrt.Workspace((args.workspace_gib << 30) // n_slots) for _ in range(n_slots)]
                              if args.workspace_gib > 0 and not single else [])
        # cost-ordered dispatch pays on single-kernel launches whose frames do not overlap; on the three-pass path (small launches
        # with a pool) it piles the expensive tiles into the first of the two chains and was measured slower: auto leaves it off there
        my_rays = w * sharding.shard_rows(h, args.tile_rows, rank, world)
        three_pass_likely = bool(pools) and my_rays <= rrt._lib.load().rrt_path_auto_max_rays()      # RRT_PATH_AUTO's own threshold
        use_order = not single and (args.tile_order == "on" or (args.tile_order == "auto" and n_slots == 1 and not three_pass_likely))
        self.orders = orders = [rrt.TileOrder() for _ in range(n_slots)] if use_order else []
        self.arith_name = args.arith or ("fast" if args.fast else "strict")
        arith_mode = {"strict": 0, "fast": 1, "fmad": 2}[self.arith_name]
        # the path of a small share under frames in flight is chosen per window by measurement (sharding.PathChooser; the rule and the
        # numbers behind it: csrc/rrt_path_chooser.cpp); RRT_PATH_POLICY pins it
        self.chooser = (sharding.PathChooser(n_slots, args.path_window)
                        if (args.path_window >= 0 and n_slots >= 2 and three_pass_likely and "RRT_PATH_POLICY" not in os.environ) else None)
        self.ends = {}                 # frame -> the event at the end of its render on this rank
        self.prms = [rrt.RenderParams(spin=args.spin, volumetrics=0 if args.no_volumetrics else 1,
                                      noise_table=0, tile_order=orders[j].id if orders else 0,
                                      arith_mode=arith_mode, workspace=pools[j].id if pools else 0,
                                      # frames in flight fill each other's drains: ONE chain per launch (the second chain's streams only compete with
                                      # the other frames: 2-7 % per frame, profiles/r05_sustained_chains.txt).  Which PATH a small share takes --
                                      # the three-pass path, or the plain single kernel, which is 6-8 % faster unless the share holds a wavefront that
                                      # outlasts the frames in flight -- is chosen per window by measurement (chooser, above; round 6)
                                      pass_chains=1 if n_slots >= 2 else 0,
                                      path_policy=int(os.environ.get("RRT_PATH_POLICY", "0"))) for j in range(n_slots)]
        self.path = camera_paths.CameraPath(args.path) if args.path >= 0 else None
        self.k, self.t, self.cam, self.table = 0, 0.0, rrt.CameraState.default(), 0
        self.times = self.cams = self.focus = None
        if self.post:               # one rank (check_args): the whole frame's HDR, the glow's scratch, the finished frame
            self.hdr = torch.zeros(h * w * 4, dtype=torch.float32, device=dev)
            self.frame = torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
        if glow is not None:
            self.glow_scratch = torch.empty(rrt.glow_scratch_bytes(w, h, glow), dtype=torch.uint8, device=dev)
        # --exr-layers: the frame comes from the debug launch, which leaves the per-ray planes the layers read next to the HDR
        self.layer_planes = {}
        for name in args.exr_layer_names:
            for _, _, plane, _ in EXR_LAYERS[name]:
                if plane not in self.layer_planes:
                    dtype, words = EXR_PLANES[plane]
                    self.layer_planes[plane] = torch.zeros(h * w * words, dtype=getattr(torch, dtype), device=dev)
        self.exposure_scratch = None
        if exposure is not None and exposure.mode == rrt.EXPOSURE_AUTO:     # the state the sequence's frames share
            self.exposure_scratch = torch.empty(rrt.exposure_scratch_bytes(), dtype=torch.uint8, device=dev)
            rrt.launch_exposure_reset(self.exposure_scratch)
        self.adaptive = None
        if args.adaptive is not None:   # one rank (check_args): the whole frame, the list's scratch, every frame's count
            self.adaptive = rrt.AdaptiveSettings(args.adaptive)
            self.ad_frame = self.frame if self.post else torch.zeros(h * w * 4, dtype=torch.uint8, device=dev)
            self.ad_scratch = torch.empty(rrt.adaptive_scratch_bytes(w, h), dtype=torch.uint8, device=dev)
            self.ad_counts = torch.zeros(max(args.frames, 1), dtype=torch.int32, pin_memory=True)

    def set_frame(self, k, table_id):
        """frame k's clock, camera and noise table (table_id: NoiseWindows.table_id), and the shutter's / the lens' samples"""
        from relativisticraytracer_amd import camera_paths
        args, mb = self.args, self.mb
        self.k = k
        self.t, path_t = camera_paths.recording_clock(k, args.fps)
        if mb > 1:
            # the shutter's sub-times; the table's window is fitted from the earliest, so that the later ones fall inside it
            self.times, sub_p = camera_paths.motion_clock(k, args.fps, args.shutter, mb)
            self.cams = [self.path.camera_at(p) for p in sub_p] if self.path is not None else [self.cam] * mb
            self.table = table_id(float(self.times[0]))
        else:
            self.table = table_id(self.t)
        if self.path is not None:
            self.cam = self.path.camera_at(path_t)
        if self.dof_k:
            if mb <= 1:
                self.times, self.cams = [self.t] * self.dof_k, [self.cam] * self.dof_k
            self.focus = args.focus if args.focus is not None else hole_distance(self.cam)

    def launch_sampled(self, buf, prm, hdr=None):
        """the stereo / defocused / panorama / blurred / supersampled launch (_stereo, _dof, _pano, _mb, _ss): the whole frame and its
        HDR when hdr is given, else this rank's tiles"""
        whole = hdr is not None
        tiles = () if whole else (self.args.tile_rows, self.rank, self.world)
        w, h = self.w, self.h
        if self.stereo is not None:
            launch = rrt.launch_raymarch_stereo if whole else rrt.launch_raymarch_stereo_tiles
            w, h = self.ew, self.eh
            when = (self.proj if self.proj is not None else rrt.Projection("pinhole"), self.stereo, self.t, self.cam)
        elif self.dof_k:
            launch = rrt.launch_raymarch_dof if whole else rrt.launch_raymarch_dof_tiles
            when = (self.times, self.cams, self.dof_points, self.focus)
        elif self.proj is not None:
            launch, when = (rrt.launch_raymarch_pano if whole else rrt.launch_raymarch_pano_tiles), (self.proj, self.t, self.cam)
        elif self.mb > 1:
            launch, when = (rrt.launch_raymarch_mb if whole else rrt.launch_raymarch_mb_tiles), (self.times, self.cams)
        else:
            launch, when = (rrt.launch_raymarch_ss if whole else rrt.launch_raymarch_ss_tiles), (self.t, self.cam)
        launch(buf, w, h, self.ss, *tiles, *when, self.tex, self.fx, prm, **({"hdr": hdr} if whole else {}))

    def render_post(self):
        """the frame through launch_sampled into self.hdr, then the post passes into self.frame (bottom-up rows, not the tile layout):
        the exposure writes the bytes -- and, in front of the glow, a 10-bit Y4M conversion or an EXR file, the scaled HDR in place --
        and the glow its own"""
        glow, hdr, frame = self.glow, self.hdr, self.frame
        self.prms[0].noise_table = self.table
        if self.adaptive is not None:
            self.render_adaptive(hdr)
        elif self.layer_planes:     # the 1x pinhole frame (check_exr): its HDR is the debug launch's d_hdr
            rrt.launch_raymarch_debug(frame, self.w, self.h, self.t, self.cam, self.tex, self.fx, self.prms[0], hdr=hdr, **self.layer_planes)
        else:
            self.launch_sampled(frame, self.prms[0], hdr=hdr)
        if self.exposure is not None:
            rrt.launch_exposure(None if glow is not None else frame, hdr if glow is not None or self.y4m10 or self.exr or self.png16 else None, hdr, self.w, self.h,
                                self.exposure, self.exposure_scratch)
        if glow is not None:
            rrt.launch_glow(frame, hdr, self.w, self.h, glow, self.glow_scratch)
        return frame

    def render_adaptive(self, hdr=None):
        """the adaptive frame into ad_frame (bottom-up rows) and, with the glow, its HDR; the count of refined pixels follows in a
        4-byte asynchronous copy, read after the last frame"""
        import torch
        self.prms[0].noise_table = self.table
        rrt.launch_raymarch_adaptive(self.ad_frame, self.w, self.h, self.ss, self.proj, self.adaptive, self.t, self.cam, self.tex, self.fx,
                                     self.ad_scratch, self.prms[0], hdr=hdr)
        self.ad_counts[self.k - 1:self.k].copy_(self.ad_scratch[:4].view(torch.int32), non_blocking=True)
        return self.ad_frame

    def render_tiles(self, buf, slot):
        """this rank's tiles of the frame into buf (FrameSharder's render callback, inside the slot's stream)"""
        import torch
        prm, k, chooser, ends = self.prms[slot], self.k, self.chooser, self.ends
        prm.noise_table = self.table
        if chooser is not None:
            prm.path_policy = chooser.policy(k)
        if self.sampled:
            self.launch_sampled(buf, prm)
        else:
            rrt.launch_raymarch_tiles(buf, self.w, self.h, self.args.tile_rows, self.rank, self.world, self.t, self.cam, self.tex, self.fx, prm)
        if chooser is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()                                        # on the slot's stream
            ends[k] = e
            # sustained time of the frames that have finished since: the interval between consecutive frames' render ends
            for j in sorted(ends):
                if j - 1 in ends and ends[j].query() and ends[j - 1].query():
                    # (a frame that ends BEFORE its predecessor -- the predecessor holds a long wavefront -- reports 0; the
                    # predecessor's own interval is then the long one, which is what the outlier rule looks for)
                    chooser.report(j, max(0.0, ends[j - 1].elapsed_time(ends[j])))
                    del ends[j - 1]

    def assemble(self, frame, buf, shard):
        rrt.assemble_tiles(frame, buf, self.w, self.h, self.args.tile_rows, shard, self.world)

    def assemble_all(self, frame, bufs, stride):
        rrt.assemble_all_tiles(frame, bufs, stride, self.w, self.h, self.args.tile_rows, self.world)

    def summary(self, noise_tables):
        """the summary line's entries from "path" on, in the line's order; noise_tables: NoiseWindows.summary()"""
        args, proj, w, h = self.args, self.proj, self.w, self.h
        exposure_info = None
        if self.exposure is not None:        # the final EV: one 4-byte read of the state, after the last frame
            import torch
            final_ev = self.exposure.ev
            if self.exposure_scratch is not None:
                o = rrt.EXPOSURE_STATE_OFFSET
                final_ev = float(self.exposure_scratch[o:o + 4].view(torch.float32).cpu()[0])
            exposure_info = dict(self.exposure.info(), final_ev=final_ev)
        return {"path": self.path.name if self.path else None, "spin": args.spin,
                "arith_mode": self.arith_name, "sink": args.out,
                "path_choice": self.chooser.stats() if self.chooser else None,
                "noise_tables": noise_tables,
                "tile_order": self.orders[0].info() if self.orders else None, "supersample": self.ss,
                "motion_blur": self.mb, "shutter": args.shutter, "glow": self.glow.info() if self.glow is not None else None,
                "projection": args.projection, "fov_deg": proj.fov_deg if proj is not None else None,
                "vfov_deg": proj.vfov_deg if args.projection == "equirect" else None,
                "stereo": self.stereo.info() if self.stereo is not None else None,
                "dof": ({"aperture": args.dof, "focus": args.focus if args.focus is not None else "hole",
                         "samples": self.dof_k} if self.dof_k else None),
                "adaptive": ({"threshold": self.adaptive.threshold,
                              "refined_fraction": float(self.ad_counts[:args.frames].double().mean()) / (w * h) if args.frames > 0 else 0.0}
                             if self.adaptive is not None else None),
                "exposure": exposure_info,
                "march_cache": rrt.march_cache_stats()}

    def close(self):
        if self.chooser is not None:
            self.chooser.destroy()
        for o in self.orders:
            o.destroy()
        self.tex.destroy()


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    pano, use_exposure, dof_k = check_args(ap, args, world)

    t_start = time.perf_counter()

    def trace(what):        # RRT_HEADLESS_TRACE=1: where the start-up time goes (stderr), as in csrc/rrt_headless.cpp
        dest = os.environ.get("RRT_HEADLESS_TRACE")        # "1": stderr; anything else: a file to append to
        if dest:
            line = f"[headless.py pid {os.getpid()} +{time.perf_counter() - t_start:7.2f}s] {what}"
            if dest == "1":
                print(line, file=sys.stderr, flush=True)
            else:
                with open(dest, "a") as fh:
                    print(line, file=fh)

    trace("importing torch")
    import torch
    trace("torch imported")
    from relativisticraytracer_amd import camera_paths, sharding, sinks
    settings = build_settings(ap, args, pano, use_exposure)

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        sys.exit("the headless driver needs a GPU (no CPU fallback)")
    backend = os.environ.get("RRT_DIST_BACKEND", "nccl")        # "gloo": rehearsal on fewer GPUs than ranks
    if backend == "gloo":
        local_rank %= max(1, torch.cuda.device_count())
    trace("GPU visible")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dog = sharding.Watchdog(f"headless.py rank {rank}")
    if world > 1:
        sharding.single_node_environment()
        lib = sharding.torch_rccl_library() if backend == "nccl" else None
        warm = sharding.warm_library_pages(lib) if lib else None
        dog.arm(args.init_timeout, "process group / communicator bring-up")
        dist = sharding.init_process_group(backend, rank, world, dev, timeout_s=args.init_timeout)
        if warm is not None:
            warm.join()

    trace("process group ready" if world > 1 else "single rank")
    r = Renderer(args, settings, dof_k, rank, world, dev)
    w, h = r.w, r.h
    # lattice-hash tables for the volumetric noise over a sliding window of the recording clock (main.cpp:511-516 lets
    # simTime grow without bound; the table's size grows with it): one table within the byte budget, rebuilt when the
    # clock leaves its window -- never a silent fall-back: frames rendered without a table are counted in the summary
    t_end, _ = camera_paths.recording_clock(max(args.frames, 1), args.fps)
    nwin = rrt.NoiseWindows(float(t_end) + 1.0, int(args.noise_table_gib * (1 << 30)), sync=torch.cuda.synchronize,
                            enabled=not args.no_noise_table and not args.no_volumetrics)
    # with several ranks the next frames render while frame k is gathered and assembled (frames arrive late, in order)
    fs = sharding.FrameSharder(w, h, args.tile_rows, rank, world, dev, r.render_tiles, r.assemble, assemble_all=r.assemble_all,
                               pipeline=r.n_slots if world > 1 else False)
    sink = sinks.open_sink(args.out, w, h, args.fps) if rank == 0 else None
    host = torch.empty(h * w * 4, dtype=torch.uint8, pin_memory=True) if sink else None
    # --y4m: rank 0 packs every finished frame on the device -- the RGBA8 frame, or at 10 bits the HDR render_post left -- and
    # copies the planes out; without --out the RGBA8 frame itself stays on the device
    y4m = None
    if rank == 0 and args.y4m_format is not None:
        fmt = rrt.YuvFormat(*args.y4m_format)
        hdr10 = rrt.Hdr10Settings(*args.y4m_hdr10) if args.y4m_hdr10 is not None else None
        y4m = sinks.Y4MSink(args.y4m, w, h, args.fps, fmt, hdr10)
        if hdr10 is not None:        # the film's light levels: reset once, metered by every frame's launch, copied back after the last
            light = torch.empty(rrt.yuv_hdr10_light_bytes(), dtype=torch.uint8, device=dev)
            rrt.launch_yuv_hdr10_light_reset(light)
        yuv_dev = torch.empty(y4m.frame_bytes, dtype=torch.uint8, device=dev)
        yuv_host = torch.empty(y4m.frame_bytes, dtype=torch.uint8, pin_memory=True)
        trace(f"y4m sink {args.y4m}: {fmt.info()}, {y4m.frame_bytes} bytes per frame")

    # --exr: rank 0 packs the HDR render_post left into the file's chunks on the device, copies them out and deflates them
    exr = None
    if rank == 0 and args.exr_format is not None:
        exr_fmt = rrt.ExrFormat(*args.exr_format[:2])
        exr_layers = None
        if args.exr_layer_names:
            exr_layers = rrt.ExrLayers(exr_fmt, w, h, exr_layer_list(args.exr_layer_names, args.exr_format[0], r.hdr, r.layer_planes))
        exr = sinks.EXRSink(args.exr, w, h, args.fps, exr_fmt, level=args.exr_format[2], layers=exr_layers)
        exr_dev = torch.empty(exr.frame_bytes, dtype=torch.uint8, device=dev)
        exr_host = torch.empty(exr.frame_bytes, dtype=torch.uint8, pin_memory=True)
        trace(f"exr sink {args.exr}: {exr_fmt.info()}, {exr.frame_bytes} bytes per frame, {exr.threads} deflate threads")

    # --png: rank 0 filters the finished frame -- the RGBA8 frame, or at 16 bits the HDR render_post left -- into the file's scanlines
    # on the device; the row sums travel behind the payload in the same copy, and the host is left with deflate
    png = None
    if rank == 0 and args.png_format is not None:
        png_fmt = rrt.PngFormat(*args.png_format[:2])
        png = sinks.PNGSink(args.png, w, h, png_fmt, level=args.png_format[2])
        png_table = (png.frame_bytes + 15) & ~15
        png_dev = torch.empty(png_table + png.row_sum_bytes, dtype=torch.uint8, device=dev)
        png_host = torch.empty(png_table + png.row_sum_bytes, dtype=torch.uint8, pin_memory=True)
        trace(f"png sink {args.png}: {png_fmt.info()}, {png.frame_bytes} bytes per frame in {png.n_slices} slices, {png.threads} deflate threads")
        if args.png_on_device:
            # --png-deflate device: the payload stays on the device.  One small buffer holds the streams' sizes and, on the next 16 bytes,
            # the row sums: it is copied first, then exactly the streams' bytes
            png_cut = png.rows_per_slice * png.stride
            png_plan = rrt.deflate_plan(png.frame_bytes, png_cut)
            png_sizes = (4 * png.n_slices + 15) & ~15
            png_dev = torch.empty(png.frame_bytes, dtype=torch.uint8, device=dev)
            png_meta = torch.empty(png_sizes + png.row_sum_bytes, dtype=torch.uint8, device=dev)
            png_meta_host = torch.empty(png_sizes + png.row_sum_bytes, dtype=torch.uint8, pin_memory=True)
            png_out = torch.empty(png_plan["out_bound"], dtype=torch.uint8, device=dev)
            png_out_host = torch.empty(png_plan["out_bound"], dtype=torch.uint8, pin_memory=True)
            png_scratch = torch.empty(png_plan["scratch_bytes"], dtype=torch.uint8, device=dev)
            trace(f"png deflate on the device: {png_plan['segments']} segments, at most {png_plan['out_bound']} bytes per frame")

    def deliver(frame):
        if png and args.png_on_device:      # filtering, then deflate, on the current stream, behind the frame's last pass
            sums = png_meta[png_sizes:]
            if r.png16:
                rrt.launch_png_from_hdr(png_dev, sums, r.hdr, w, h, png_fmt)
            else:
                rrt.launch_png_from_rgba8(png_dev, sums, frame, w, h, png_fmt)
            rrt.launch_deflate(png_out, png_meta, png_scratch, png_dev, png.frame_bytes, png_cut, True)
            png_meta_host.copy_(png_meta, non_blocking=False)
            meta = png_meta_host.numpy()
            sizes = meta[:4 * png.n_slices].view("uint32").astype("int64")
            total = int(sizes.sum())
            png_out_host[:total].copy_(png_out[:total], non_blocking=False)
            streams, ends = png_out_host.numpy(), sizes.cumsum()
            png.write_streams([streams[e - n:e] for n, e in zip(sizes.tolist(), ends.tolist())], meta[png_sizes:].view("uint32"))
        elif png:       # on the current stream, behind the frame's last pass
            if r.png16:
                rrt.launch_png_from_hdr(png_dev, png_dev[png_table:], r.hdr, w, h, png_fmt)
            else:
                rrt.launch_png_from_rgba8(png_dev, png_dev[png_table:], frame, w, h, png_fmt)
            png_host.copy_(png_dev, non_blocking=False)
            data = png_host.numpy()
            png.write(data[:png.frame_bytes], data[png_table:].view("uint32"))
        if exr:         # on the current stream, behind the frame's last pass
            if exr_layers is not None:
                rrt.launch_exr_layers(exr_dev, exr_layers)
            else:
                rrt.launch_exr_from_hdr(exr_dev, r.hdr, w, h, exr_fmt)
            exr_host.copy_(exr_dev, non_blocking=False)
            exr.write(exr_host.numpy())
        if y4m:         # on the current stream, behind the frame
            if y4m.hdr10 is not None:
                rrt.launch_yuv_hdr10_from_hdr(yuv_dev, r.hdr, w, h, fmt, y4m.hdr10, light)
            elif r.y4m10:
                rrt.launch_yuv_from_hdr(yuv_dev, r.hdr, w, h, fmt)
            else:
                rrt.launch_yuv_from_rgba8(yuv_dev, frame, w, h, fmt)
            yuv_host.copy_(yuv_dev, non_blocking=False)
            y4m.write(yuv_host.numpy())
        if sink:
            host.copy_(frame, non_blocking=False)
            sink.write(host.numpy().reshape(h, w, 4))

    torch.cuda.synchronize()
    trace("sky, pools, sink ready; first frame")
    t0 = time.perf_counter()
    for k in range(1, args.frames + 1):
        dog.arm(args.frame_timeout + (args.init_timeout if k == 1 else 0.0), f"frame {k}")    # frame 1 brings the communicator's channels up
        r.set_frame(k, nwin.table_id)
        frame = r.render_post() if r.post else (r.render_adaptive() if r.adaptive is not None else fs.step())
        if (sink or y4m or exr or png) and frame is not None:
            deliver(frame)
    for frame in fs.drain():                # the frames still in flight, in order
        if sink or y4m or exr or png:
            deliver(frame)
    torch.cuda.synchronize()
    trace("frames done")
    dog.arm(args.frame_timeout, "final barrier")
    if world > 1:
        dist.barrier()
    dog.disarm()
    dt = time.perf_counter() - t0
    if rank == 0:
        if sink:
            sink.close()
        if exr:
            exr.close()
        if png:
            png.close()
        if y4m:
            y4m.close(rrt.yuv_hdr10_light_levels(light.cpu().numpy(), w, h) if y4m.hdr10 is not None else None)
        print(json.dumps({"frames": args.frames, "width": w, "height": h, "n_gpus": world, "seconds": round(dt, 4),
                          "fps": round(args.frames / dt, 3), "Mrays_per_s": round(args.frames * w * h / dt / 1e6, 3), **r.summary(nwin.summary())}),
              flush=True)
    if world > 1:
        dist.destroy_process_group()
    nwin.close()
    r.close()


if __name__ == "__main__":
    main()
