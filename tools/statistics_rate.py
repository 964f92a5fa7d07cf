"""Cost of the per-pixel noise statistics (slrhip_statistics_begin) on whole renders: 1280x720 x 1024 spp RGB and 1280x720 x
256 spp spectral on the Cornell box, with and without statistics, alternating; wall time of slrhip_render, median of --reps
after one warm-up render.  Also the cost of one stop check of slrhip_render_until (slrhip_statistics_summary: two small kernels,
a 48-byte copy and a stream synchronise), in microseconds.  `--only rgb|spectral --statistics on|off --reps 1`: one render,
for a kernel trace of its own (the fold kernel's time).  A build without the statistics (SLRHIP_LIBRARY) runs the `off` half."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, binding, scenes  # noqa: E402


def render_seconds(ctx, st, spp, statistics):
    ctx.render_begin(st)
    if statistics:
        ctx.statistics_begin()
    ctx.synchronize()
    t0 = time.perf_counter()
    ctx.render(0, spp)
    ctx.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["rgb", "spectral"])
    ap.add_argument("--statistics", choices=["on", "off", "both"], default="both")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-warmup", action="store_true")
    args = ap.parse_args()
    w, h = 1280, 720
    sc = scenes.cornell_box_spheres(w / h, 48, 24, "matte")
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    have = hasattr(binding.load_library(), "slrhip_statistics_begin")
    out = {"width": w, "height": h, "library_has_statistics": have}
    for name, mode, spp in (("rgb", abi.MODE_RGB, 1024), ("spectral", abi.MODE_SPECTRAL, 256)):
        if args.only and name != args.only:
            continue
        ctx = Context(mode=mode)
        ctx.upload_scene(sc)
        kinds = [k for k in ("off", "on") if args.statistics in (k, "both") and (k == "off" or have)]
        if not args.no_warmup:
            render_seconds(ctx, st, spp, False)
        runs = {k: [] for k in kinds}
        for _ in range(args.reps):                       # alternating
            for k in kinds:
                runs[k].append(render_seconds(ctx, st, spp, k == "on"))
        out[name] = {"spp": spp}
        for k in kinds:
            out[name]["statistics_%s_s" % k] = float(np.median(runs[k]))
            out[name]["statistics_%s_runs" % k] = [round(t, 4) for t in runs[k]]
        if "on" in kinds:
            if "off" in kinds:
                out[name]["overhead"] = out[name]["statistics_on_s"] / out[name]["statistics_off_s"] - 1.0
            # the state the last render left has statistics on: the stop check on it
            us = []
            for _ in range(50):
                t0 = time.perf_counter()
                s = ctx.statistics_summary()
                us.append((time.perf_counter() - t0) * 1e6)
            out[name]["summary_us_median"] = float(np.median(us[5:]))
            out[name]["noise_rmse"] = abi.noise_metric(s, abi.NOISE_RMSE)
            out[name]["noise_relative"] = abi.noise_metric(s, abi.NOISE_RELATIVE)
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
