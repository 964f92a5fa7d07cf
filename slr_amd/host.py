"""`python -m slr_amd.host scene.txt [--spectral] [--samples N] [--out DIR]` — the HostProgram of the reference
(HostProgram/main.cpp:20-62: read a scene script, build, render) on the HIP path.

Reads a scene in the reference's scene language (slr_amd/scene_language.py), renders it with the path tracer and leaves
behind what PathTracingRenderer::render leaves behind (PathTracingRenderer.cpp:83-94): "%03u.bmp" after 1, 2, 4, ...
samples with scale brightness / samples, and one stdout line "%u samples: %s, %g[s]" per image, at most 16 images.
A scene that asks for another renderer ("BPT", ...) is rendered with the path tracer and a note on stderr.
`--features DIR` (or a scene whose renderer is "debug") also writes the first-hit feature buffers: the normal images of the
reference's DebugRenderer and features.npz with the raw per-pixel sums.
`--noise-target X` renders to a noise level instead of a sample count: blocks of `--noise-step` passes until the estimated error
of the frame (`--noise-metric rmse`: RMS of the per-pixel standard error of the mean luminance; `relative`: that over the mean
luminance) is at most X or `--max-spp` passes are done; prints the passes reached and the final estimate, writes one image, and
with `--noise-map FILE.npy` the per-pixel variance of the mean.  Every pixel gets the same passes.
`--adaptive T` stops every pixel on its own instead (Context.render_adaptive): `--spp-min` passes, then blocks of `--noise-step`
up to `--max-spp`; after each block the pixels whose standard error of the mean luminance is at most T times that mean (times
`--adaptive-floor` for darker pixels) retire.  The image is written from the mean frame; the samples rendered are printed against
pixels x sample limit.
`--denoise [ITERATIONS]` (default 5, 1 .. 8) also filters the final frame on the device (Context.denoised: the mean frame guided by
the variance of the mean, the shading normals and the camera distance, which are rendered alongside) and writes
"<name>_denoised.bmp" next to the last image.
`--demodulate` (with `--denoise`) writes "<name>_denoised.bmp" from the albedo-demodulated pipeline: the first-hit albedo is rendered
alongside (Context.render_albedo), the frame is divided by it before the filter and multiplied back afterwards, so that texture
detail passes the filter.  `--albedo FILE.npy` writes the mean first-hit albedo [height, width, components].
`--device-tonemap` tone-maps every BMP above on the device (Context.frame_image, slrhip_tonemap): the frame is resolved into device
memory (or is the denoiser's output there) and only the 8-bit rows are copied back, in place of a read-back of the floats and the
host loop of slrhip_tonemap_bgr8.
`--environment FILE.npy [--environment-scale S]` lights the scene with a lat-long image ([H][W][3] linear RGB): it is rounded to
binary16 and handed to the scene with the importance map of slrhip_env_importance (with `--spectral` also as (u, v, s) texels,
slrhip_env_texels_to_uvs), so a scene lit only by its environment renders.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import abi, binding, scene_language

# setRenderer("debug", (outputs = (...))) names (libSLRSceneGraph/API.cpp:1037-1059) -> channel bits
DEBUG_OUTPUTS = {"geometric normal": abi.FEATURE_GEOMETRIC_NORMAL, "shading normal": abi.FEATURE_SHADING_NORMAL,
                 "shading tangent": abi.FEATURE_SHADING_TANGENT, "distance": abi.FEATURE_DISTANCE}


def encode_normals(sums, coverage):
    """DebugRenderer's image of a vector channel (DebugRenderer.cpp:162-185): (uint8)clamp((0.5 n + 0.5) * 255, 0, 255) of the
    per-pixel mean over the hits (0 where nothing was hit), as the [h, w, 3] BGR bottom-up pixels a BMP holds."""
    cov = np.asarray(coverage, np.float32)[:, :, None]
    mean = np.where(cov > 0, np.asarray(sums, np.float32) / np.maximum(cov, np.float32(1)), np.float32(0)).astype(np.float32)
    rgb = np.clip((np.float32(0.5) * mean + np.float32(0.5)) * np.float32(255), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(rgb[::-1, :, ::-1])


def save_bmp(path, bgr_bottom_up):
    """[h, w, 3] uint8 BGR bottom-up pixels through slrhip_save_bmp (rows padded as it expects them)."""
    h, w, _ = bgr_bottom_up.shape
    rows = np.zeros((h, 3 * w + w % 4), np.uint8)
    rows[:, :3 * w] = bgr_bottom_up.reshape(h, 3 * w)
    lib = binding.load_library()
    binding._check(lib, lib.slrhip_save_bmp(path.encode(), rows.ctypes.data, w, h), "slrhip_save_bmp")


def write_features(ctx, spp, out_dir, channels):
    """The feature buffers of `spp` passes next to the beauty frame: geometric_normal.bmp, shading_normal.bmp, shading_tangent.bmp
    (DebugRenderer's file names, DebugRenderer.cpp:112-127) for the vector channels asked for, and features.npz with the raw sums."""
    ctx.render_features(channels | abi.FEATURE_COVERAGE, spp)
    raw = {abi.FEATURE_CHANNELS[c][0]: ctx.features(c) for c in abi.FEATURE_CHANNELS if c & (channels | abi.FEATURE_COVERAGE)}
    for c in (abi.FEATURE_GEOMETRIC_NORMAL, abi.FEATURE_SHADING_NORMAL, abi.FEATURE_SHADING_TANGENT):
        name = abi.FEATURE_CHANNELS[c][0]
        if name in raw:
            save_bmp(os.path.join(out_dir, name + ".bmp"), encode_normals(raw[name], raw["coverage"]))
    np.savez(os.path.join(out_dir, "features.npz"), **raw)


def write_image(ctx, st, scale, path, source, device_tonemap, **denoise):
    """frame -> BMP file.  source: "sum" (the frame of sums), "mean" (of per-pixel means) or "denoised" (Context.denoised(**denoise)).
    The floats are read back and tone-mapped by slrhip_tonemap_bgr8, or with device_tonemap (--device-tonemap) tone-mapped where they
    are and only the image is read back."""
    w, h = st.image_width, st.image_height
    if device_tonemap:
        bmp = ctx.denoised(image=(scale, abi.IMAGE_BGR8_BMP), **denoise) if source == "denoised" else ctx.frame_image(scale, mean=source == "mean")
    else:
        fb = ctx.denoised(**denoise) if source == "denoised" else ctx.read_framebuffer_mean() if source == "mean" else ctx.read_framebuffer()
        bmp = np.zeros((3 * w + w % 4) * h, np.uint8)
        binding._check(ctx.lib, ctx.lib.slrhip_tonemap_bgr8(fb.ctypes.data, w, h, ctx.components, C.c_float(scale), bmp.ctypes.data, bmp.size), "slrhip_tonemap_bgr8")
    binding._check(ctx.lib, ctx.lib.slrhip_save_bmp(path.encode(), bmp.ctypes.data, w, h), "slrhip_save_bmp")


def render_to_noise_target(ctx, st, args, spp, sensitivity):
    """--noise-target: Context.render_until in place of the 1, 2, 4, ... loop; one image ("000.bmp") of the passes reached."""
    start = time.time()
    ctx.statistics_begin()
    metric = abi.NOISE_METRICS[args.noise_metric]
    done, summary = ctx.render_until(metric, args.noise_target, args.noise_step, args.max_spp or spp)
    scale = float(np.float32(np.float32(st.brightness) / np.float32(done)) * np.float32(sensitivity))
    write_image(ctx, st, scale, os.path.join(args.out, "000.bmp"), "sum", args.device_tonemap)
    print("%u samples: 000.bmp, %g[s]" % (done, time.time() - start), flush=True)
    print("noise target %g (%s): reached %g after %u samples%s" % (args.noise_target, args.noise_metric, abi.noise_metric(summary, metric), done,
                                                                  "" if abi.noise_metric(summary, metric) <= args.noise_target else " (sample limit)"), flush=True)
    if args.noise_map:
        np.save(args.noise_map, ctx.statistics(abi.STATISTICS_VARIANCE_OF_MEAN))
    return done


def render_adaptively(ctx, st, args, spp, sensitivity):
    """--adaptive: Context.render_adaptive in place of the 1, 2, 4, ... loop; one image ("000.bmp") from the MEAN frame (the pixels
    hold different numbers of samples), scale brightness x sensitivity in place of brightness / samples x sensitivity."""
    start = time.time()
    ctx.statistics_begin()
    spp_max = max(args.max_spp or spp, args.spp_min)
    done, samples = ctx.render_adaptive(0, args.adaptive, args.adaptive_floor, args.spp_min, args.noise_step, spp_max)
    w, h = st.image_width, st.image_height
    scale = float(np.float32(st.brightness) * np.float32(sensitivity))
    write_image(ctx, st, scale, os.path.join(args.out, "000.bmp"), "mean", args.device_tonemap)
    print("%u samples: 000.bmp, %g[s]" % (done, time.time() - start), flush=True)
    full = w * h * spp_max
    print("adaptive %g (floor %g): %u of %u samples rendered (%.1f %%), %u of %u pixels still active after %u passes"
          % (args.adaptive, args.adaptive_floor, samples, full, 100.0 * samples / full, ctx.adaptive_active(), w * h, done), flush=True)
    if args.noise_map:
        np.save(args.noise_map, ctx.statistics(abi.STATISTICS_VARIANCE_OF_MEAN))
    return done


DENOISE_CHANNELS = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE


def write_denoised(ctx, st, iterations, sensitivity, path, device_tonemap=False, demodulate=False):
    """--denoise: the filtered MEAN frame (scale brightness x sensitivity, as --adaptive writes its image) to `path`."""
    scale = float(np.float32(st.brightness) * np.float32(sensitivity))
    extra = dict(demodulate=True) if demodulate else {}
    write_image(ctx, st, scale, path, "denoised", device_tonemap, iterations=iterations, **extra)
    print("denoised (%u iterations%s): %s" % (iterations, ", albedo-demodulated" if demodulate else "", os.path.basename(path)), flush=True)


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m slr_amd.host")
    ap.add_argument("scene")
    ap.add_argument("--spectral", action="store_true", help="16 wavelength samples per path (the reference's default build)")
    ap.add_argument("--samples", type=int, default=0, help="override the script's sample count")
    ap.add_argument("--out", default=".")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--features", metavar="DIR", default=None,
                    help="also write the first-hit feature buffers (normal BMPs as the reference's DebugRenderer names them, features.npz) to DIR")
    ap.add_argument("--noise-target", type=float, default=None, metavar="X",
                    help="render until the frame's estimated noise is at most X instead of a fixed sample count")
    ap.add_argument("--noise-metric", choices=sorted(abi.NOISE_METRICS), default="rmse",
                    help="rmse: RMS over the pixels of the standard error of the mean luminance; relative: that over the mean luminance")
    ap.add_argument("--noise-step", type=int, default=16, metavar="N", help="passes between two stop checks")
    ap.add_argument("--max-spp", type=int, default=0, metavar="N", help="sample limit of --noise-target (default: the sample count)")
    ap.add_argument("--noise-map", default=None, metavar="FILE.npy", help="with --noise-target: write the per-pixel variance of the mean")
    ap.add_argument("--adaptive", type=float, default=None, metavar="T",
                    help="per-pixel adaptive sampling: a pixel retires once the standard error of its mean luminance is at most T x that mean")
    ap.add_argument("--adaptive-floor", type=float, default=0.05, metavar="F", help="with --adaptive: pixels darker than F are judged relative to F")
    ap.add_argument("--spp-min", type=int, default=16, metavar="N", help="with --adaptive: passes every pixel gets before the first check (>= 2)")
    ap.add_argument("--denoise", type=int, nargs="?", const=5, default=None, metavar="ITERATIONS",
                    help="also write <name>_denoised.bmp: the final frame filtered on the device (a-trous iterations, 1 .. 8; default 5)")
    ap.add_argument("--demodulate", action="store_true",
                    help="with --denoise: divide the frame by the first-hit albedo before the filter and multiply it back afterwards")
    ap.add_argument("--albedo", default=None, metavar="FILE.npy", help="write the mean first-hit albedo [height, width, components]")
    ap.add_argument("--device-tonemap", action="store_true",
                    help="tone-map every BMP on the device and read back only the 8-bit image, not the float frame")
    ap.add_argument("--clamp", type=float, default=None, metavar="L",
                    help="scale a sample whose luminance (un-normalised: brightness and sample count not applied) exceeds L down to L")
    ap.add_argument("--drop-nonfinite", action="store_true", help="replace a sample whose luminance is NaN or infinite by zero")
    ap.add_argument("--clamp-map", default=None, metavar="FILE.npy",
                    help="with --clamp or --drop-nonfinite: write the per-pixel clamp records [4, height, width]: clamped, dropped, removed, largest")
    ap.add_argument("--environment", default=None, metavar="FILE.npy",
                    help="light the scene with this lat-long image: [H][W][3] linear RGB radiance, H and W multiples of 4 (row 0 = +Y)")
    ap.add_argument("--environment-scale", type=float, default=1.0, metavar="S", help="with --environment: the radiance scale")
    return ap


def environment_from_file(path, scale, spectral):
    """--environment: the tuple load_scene(environment=...) takes.  The image is rounded to binary16, as the reference's RGBA16F image
    holds it; the importance map (and, for --spectral, the (u, v, s) texels and their importance map) come from the library's host
    exports slrhip_env_importance / slrhip_env_texels_to_uvs."""
    rgb = np.asarray(np.load(path), np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] % 4 or rgb.shape[1] % 4:
        raise ValueError("--environment: a [height, width, 3] array with height and width multiples of 4 expected, not %r" % (rgb.shape,))
    rgb = rgb.astype(np.float16).astype(np.float32)
    env = (rgb, float(scale), binding.env_importance(rgb, abi.MODE_RGB))
    if spectral:
        uvs = binding.env_texels_to_uvs(rgb)
        env = env + (uvs, binding.env_importance(uvs, abi.MODE_SPECTRAL))
    return env


def clamp_begin(ctx, args):
    """--clamp / --drop-nonfinite: Context.clamp_begin for the render that has just begun.  True if the clamp is on."""
    if args.clamp is None and not args.drop_nonfinite:
        return False
    ctx.clamp_begin(float("inf") if args.clamp is None else args.clamp, args.drop_nonfinite)
    return True


def report_clamp(ctx, args):
    """The clamp's summary line and, with --clamp-map, the four record channels."""
    s = ctx.clamp_summary()
    print("clamp %g%s: %u samples clamped, %u dropped, luminance removed %g, largest clamped sample %g"
          % (float("inf") if args.clamp is None else args.clamp, " (non-finite samples dropped)" if args.drop_nonfinite else "",
             s["clamped"], s["dropped"], s["removed"], s["largest"]), flush=True)
    if args.clamp_map:
        np.save(args.clamp_map, np.stack([ctx.clamp(c) for c in sorted(abi.CLAMP_CHANNELS)]))


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.noise_target is None and args.adaptive is None and (args.noise_map or args.max_spp):
        ap.error("--noise-map and --max-spp go with --noise-target or --adaptive")
    if args.adaptive is not None and (args.noise_target is not None or not args.adaptive >= 0 or not args.adaptive_floor >= 0 or args.spp_min < 2
                                      or args.noise_step < 1 or args.max_spp < 0):
        ap.error("--adaptive takes no --noise-target; it and --adaptive-floor must be >= 0, --spp-min >= 2, --noise-step positive, --max-spp non-negative")
    if args.noise_target is not None and (args.noise_step < 1 or args.max_spp < 0 or args.noise_target != args.noise_target):
        ap.error("--noise-step must be positive, --max-spp non-negative and --noise-target a number")

    if args.denoise is not None and not 1 <= args.denoise <= 8:
        ap.error("--denoise takes 1 .. 8 iterations")
    if args.demodulate and args.denoise is None:
        ap.error("--demodulate goes with --denoise")
    if args.clamp is not None and not args.clamp > 0:
        ap.error("--clamp takes a limit > 0")
    if args.clamp_map and args.clamp is None and not args.drop_nonfinite:
        ap.error("--clamp-map goes with --clamp or --drop-nonfinite")

    if not args.environment_scale >= 0 or args.environment_scale == float("inf"):
        ap.error("--environment-scale must be finite and >= 0")
    try:
        environment = environment_from_file(args.environment, args.environment_scale, args.spectral) if args.environment else None
    except (OSError, ValueError) as e:
        print("failed to read the environment image: %s" % e, file=sys.stderr)
        return -1
    try:
        scene, settings, renderer = scene_language.load_scene(args.scene, environment=environment)
    except scene_language.SceneLanguageError as e:
        print("failed to read the scene: %s" % e, file=sys.stderr)
        return -1                                                            # main.cpp:39-42
    feature_dir, feature_channels = args.features, abi.FEATURE_ALL
    if renderer["method"] == "debug":
        # the beauty frame is rendered as before; the debug renderer's outputs are written next to it
        feature_dir = feature_dir or args.out
        feature_channels = 0
        for name in renderer.get("outputs") or DEBUG_OUTPUTS:
            feature_channels |= DEBUG_OUTPUTS[name]
    elif renderer["method"] != "PT":
        print("note: the scene asks for %r; only the unidirectional path tracer is built, rendering with it" % renderer["method"], file=sys.stderr)
    spp = args.samples or int(renderer["samples"])
    st = abi.RenderSettings(int(settings["width"]), int(settings["height"]), float(settings["timeStart"]), float(settings["timeEnd"]),
                            float(settings["brightness"]), int(settings["rngSeed"]))
    ctx = binding.Context(device=args.device, mode=abi.MODE_SPECTRAL if args.spectral else abi.MODE_RGB)
    ctx.upload_scene(scene)
    ctx.render_begin(st)
    clamped = clamp_begin(ctx, args)                                         # before the first render call, like the statistics
    cam = scene.camera
    sensitivity = cam.sensitivity if cam.sensitivity > 0 else float(np.float32(1.0 / (np.pi * float(np.float32(cam.lens_radius)) ** 2))) if cam.lens_radius > 0 else 1.0
    start = time.time()
    done, export, img = 0, 1, 0
    name = "000.bmp"
    if args.denoise is not None and args.noise_target is None and args.adaptive is None:
        ctx.statistics_begin()                                               # the filter's variance guide; the frame is unchanged in every bit
    if args.noise_target is not None:
        done = spp = render_to_noise_target(ctx, st, args, spp, sensitivity)
    elif args.adaptive is not None:
        done = spp = render_adaptively(ctx, st, args, spp, sensitivity)
    while done < spp and img < 16:
        upto = min(export, spp)
        ctx.render(done, upto - done)
        done = upto
        if done == export:
            name = "%03u.bmp" % img
            scale = float(np.float32(np.float32(st.brightness) / np.float32(done)) * np.float32(sensitivity))
            write_image(ctx, st, scale, os.path.join(args.out, name), "sum", args.device_tonemap)
            print("%u samples: %s, %g[s]" % (export, name, time.time() - start), flush=True)
            img += 1
            export += export
    if clamped:
        report_clamp(ctx, args)
    if feature_dir is not None:
        os.makedirs(feature_dir, exist_ok=True)
        # one channel set per render: with --denoise the guides ride with the channels asked for
        write_features(ctx, spp, feature_dir, feature_channels | (DENOISE_CHANNELS if args.denoise is not None else 0))
    elif args.denoise is not None:
        ctx.render_features(DENOISE_CHANNELS, spp)
    if args.demodulate or args.albedo:
        ctx.render_albedo(spp)
    if args.albedo:
        sums, passes = ctx.albedo()
        np.save(args.albedo, sums / np.float32(passes))
        print("albedo (%u passes): %s" % (passes, os.path.basename(args.albedo)), flush=True)
    if args.denoise is not None:
        write_denoised(ctx, st, args.denoise, sensitivity, os.path.join(args.out, os.path.splitext(name)[0] + "_denoised.bmp"), args.device_tonemap,
                       args.demodulate)
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
