"""What the denoiser (slrhip_denoise) costs on the headline Cornell frame (1280x720): the call with every stop on (variance, shading
normals, distance), --iterations a-trous iterations, for 3 components (an RGB context) and 16 (a spectral one).

The inputs are a real render's: --spp passes with statistics on, the three guides rendered alongside, all five buffers resolved into
device memory once.  Each timed call is bracketed by two HIP events on one stream (torch.cuda.Event), after --warmup calls; the
median, the fastest and the slowest of --reps calls are reported, and the same for a one-iteration call (prepare + one filter launch),
so that (t_n - t_1) / (n - 1) is the time of a later iteration.  Against that: the bytes an iteration must move — one read of the
colour record, the 16-byte guide record and the 8-byte {Y, v} record, one write of the colour and the {Y, v} record, per pixel: 64 B
for 3 components (the colour padded to a float4), 160 B for 16 — over the HBM rate DESIGN.md 7.2 measures against.  One JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402

HBM_BYTES_PER_SECOND = 8.0e12          # the peak DESIGN.md 7.2 states its fractions against


def iteration_bytes(pixels, components):
    colour = 16 if components == 3 else 64
    return pixels * (colour + 16 + 8 + colour + 8)


def measure(mode, w, h, spp, iterations, warmup, reps):
    ctx = Context(mode=mode)
    ctx.upload_scene(scenes.cornell_box_spheres(w / h, 48, 24, "matte"))
    ctx.render_begin(abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED))
    ctx.statistics_begin()
    ctx.render(0, spp)
    ctx.render_features(abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE, spp)
    comps = ctx.components
    dev = "cuda:%d" % ctx.device
    buf = {name: torch.empty(n, dtype=torch.float32, device=dev)
           for name, n in (("color", h * w * comps), ("variance", h * w), ("normal", h * w * 3), ("distance", h * w), ("coverage", h * w),
                           ("output", h * w * comps), ("output_variance", h * w))}
    stream = torch.cuda.current_stream(ctx.device)
    ctx.mean_into(buf["color"].data_ptr(), buf["color"].numel(), stream)
    ctx.statistics_into(abi.STATISTICS_VARIANCE_OF_MEAN, buf["variance"].data_ptr(), h * w, stream)
    for name, channel in (("normal", abi.FEATURE_SHADING_NORMAL), ("distance", abi.FEATURE_DISTANCE), ("coverage", abi.FEATURE_COVERAGE)):
        ctx.features_into(channel, buf[name].data_ptr(), buf[name].numel(), stream)
    ptrs = {name: t.data_ptr() for name, t in buf.items()}

    def call(n):
        ctx.denoise_into(w, h, comps, n, stream=stream, **ptrs)

    def timed(n):
        for _ in range(warmup):
            call(n)
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call(n)
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))
    full, one = timed(iterations), timed(1)
    out = dict(components=comps, iterations=iterations, call=full, one_iteration_call=one,
               finite=bool(torch.isfinite(buf["output"]).all().item()), hit_fraction=float((buf["coverage"] > 0).float().mean().item()))
    if iterations > 1:
        per = (full["median_ms"] - one["median_ms"]) / (iterations - 1)
        need = iteration_bytes(w * h, comps)
        out.update(later_iteration_ms=per, iteration_bytes=need, iteration_floor_ms=need / HBM_BYTES_PER_SECOND * 1e3,
                   fraction_of_hbm_rate=need / HBM_BYTES_PER_SECOND / (per * 1e-3))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    out = dict(width=args.width, height=args.height, spp=args.spp, hbm_bytes_per_second=HBM_BYTES_PER_SECOND,
               sigma_luminance=4.0, sigma_distance=abi.DENOISE_SIGMA_DISTANCE, normal_power_log2=7)
    out["rgb"] = measure(abi.MODE_RGB, args.width, args.height, args.spp, args.iterations, args.warmup, args.reps)
    out["spectral"] = measure(abi.MODE_SPECTRAL, args.width, args.height, args.spp, args.iterations, args.warmup, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
