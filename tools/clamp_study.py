"""Does the sample clamp (slrhip_clamp_begin) help the denoiser?  RMSE of a 16-spp frame against an UNCLAMPED 4096-spp render of the
same seed family: as rendered, and clamped at the 99th, 99.9th and 99.99th percentile of the 16-spp samples' luminances (non-finite
samples dropped), each as it is, denoised (Context.denoised) and denoised with albedo demodulation.  Per-pixel means, all components,
over the pixels that are finite in every frame.  With each clamped variant the bias: the luminance the clamp removed over the
luminance the samples came with.  No parameter is tuned; the numbers are printed as they come, one JSON document."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, binding, scenes  # noqa: E402

GUIDES = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE
PERCENTILES = (99.0, 99.9, 99.99)


def sample_luminances(ctx, st, spp):
    """Y of every sample of `spp` passes, from per-pass frames (the sensor's sum of one value from zero is that value)."""
    lib = binding.load_library()
    out = []
    for p in range(spp):
        ctx.render_begin(st)
        ctx.render(p, 1)
        fb = ctx.read_framebuffer().reshape(-1, ctx.components)
        if ctx.components == 3:                            # the expression of slrhip_sample_luminance, on all rows at once
            d = fb.astype(np.float64)
            out.append(((0.222485 * d[:, 0] + 0.716905 * d[:, 1]) + 0.060610 * d[:, 2]).astype(np.float32))
        else:
            out.append(np.array([lib.slrhip_sample_luminance(ctx.components, row.ctypes.data) for row in fb], np.float32))
    return np.concatenate(out)


def variant(ctx, st, spp, iterations, limit):
    ctx.render_begin(st)
    ctx.statistics_begin()
    if limit is not None:
        ctx.clamp_begin(limit, True)
    ctx.render(0, spp)
    ctx.render_features(GUIDES, spp)
    ctx.render_albedo(spp)
    frames = {"noisy": ctx.read_framebuffer_mean(), "denoised": ctx.denoised(iterations=iterations),
              "denoised_demodulated": ctx.denoised(iterations=iterations, demodulate=True)}
    info = {}
    if limit is not None:
        s, received = ctx.clamp_summary(), ctx.statistics(abi.STATISTICS_MEAN).astype(np.float64).sum() * spp
        info = {"limit": float(limit), "clamped": s["clamped"], "dropped": s["dropped"], "removed": s["removed"], "largest": s["largest"],
                "bias": s["removed"] / (s["removed"] + received)}
    return frames, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=["glass", "textured"], default="glass", help="the headline Cornell box with the glass sphere, or cornell_textured")
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=5)
    args = ap.parse_args()
    w, h = args.width, args.height
    sc = scenes.cornell_textured(w / h, 16, 8) if args.scene == "textured" else scenes.cornell_box_spheres(w / h, 16, 8, "glass")
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    ctx = Context()
    ctx.upload_scene(sc)
    ctx.render_begin(st)
    ctx.render(0, args.reference_spp)
    reference = ctx.read_framebuffer().astype(np.float64) / args.reference_spp
    y = sample_luminances(ctx, st, args.spp)
    limits = [None] + [float(np.percentile(y[np.isfinite(y)], q)) for q in PERCENTILES]
    results = [variant(ctx, st, args.spp, args.iterations, limit) for limit in limits]
    ctx.close()
    finite = np.isfinite(reference).all(axis=2)
    for frames, _ in results:
        for frame in frames.values():
            finite &= np.isfinite(frame).all(axis=2)
    out = {"scene": args.scene, "width": w, "height": h, "spp": args.spp, "reference_spp": args.reference_spp, "iterations": args.iterations,
           "reference_mean": float(reference[finite].mean()), "pixels_left_out_as_non_finite": int((~finite).sum()),
           "non_finite_samples": int((~np.isfinite(y)).sum()), "sample_luminance_max": float(y[np.isfinite(y)].max()),
           "sample_luminance_mean": float(y[np.isfinite(y)].mean()), "variants": []}
    for (frames, info), name in zip(results, ["as rendered"] + ["clamped at the %gth percentile" % q for q in PERCENTILES]):
        row = dict(name=name, **info)
        for kind, frame in frames.items():
            row["rmse_" + kind] = float(np.sqrt(((frame.astype(np.float64) - reference) ** 2)[finite].mean()))
        out["variants"].append(row)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
