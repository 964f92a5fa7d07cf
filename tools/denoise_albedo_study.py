"""RMSE of the 16-spp cornell_textured frame against a 4096-spp render of the same seed family: as rendered, denoised
(Context.denoised), and denoised with albedo demodulation (demodulate=True).  Per-pixel means, all components; also over the pixels
whose first hit is a textured material only.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402

GUIDES = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE


def rmse(a, b, mask):
    d = (a.astype(np.float64) - b) ** 2
    return float(np.sqrt(d[mask].mean())) if mask.any() else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--reference-spp", type=int, default=4096)
    ap.add_argument("--iterations", type=int, default=5)
    args = ap.parse_args()
    w, h = args.width, args.height
    sc = scenes.cornell_textured(w / h, 16, 8)
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    ctx = Context()
    ctx.upload_scene(sc)
    ctx.render_begin(st)
    ctx.render(0, args.reference_spp)
    reference = ctx.read_framebuffer().astype(np.float64) / args.reference_spp
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.render(0, args.spp)
    ctx.render_features(GUIDES | abi.FEATURE_IDS, args.spp)
    ctx.render_albedo(args.spp)
    noisy = ctx.read_framebuffer_mean()
    plain = ctx.denoised(iterations=args.iterations)
    demodulated = ctx.denoised(iterations=args.iterations, demodulate=True)
    material = ctx.features(abi.FEATURE_IDS)[:, :, 2]
    ctx.close()
    textured = [i for i, m in enumerate(sc.materials) if int(m["type"]) != abi.MAT_MULTI and int(m["spectrum"][0]) <= -2]
    # a pixel that is not finite in any of the four frames (a NaN sample stays in its pixel) is left out of every figure
    finite = np.isfinite(reference).all(axis=2)
    for frame in (noisy, plain, demodulated):
        finite &= np.isfinite(frame).all(axis=2)
    mask = np.isin(material, textured) & finite
    out = {"scene": "cornell_textured", "width": w, "height": h, "spp": args.spp, "reference_spp": args.reference_spp, "iterations": args.iterations,
           "mean": float(reference[finite].mean()), "non_finite_pixels": int((~finite).sum()), "textured_pixels": int(mask.sum())}
    for name, frame in (("noisy", noisy), ("denoised", plain), ("denoised_demodulated", demodulated)):
        out["rmse_" + name] = rmse(frame, reference, finite)
        out["rmse_" + name + "_textured"] = rmse(frame, reference, mask)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
