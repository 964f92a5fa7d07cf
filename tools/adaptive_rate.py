"""What per-pixel adaptive sampling (slrhip_render_adaptive) buys and costs on the headline Cornell frame (1280x720, RGB) at a fixed
sample limit: wall time, samples rendered and the final RELATIVE noise metric (slrhip_statistics_summary) of

  uniform    slrhip_render_until with target 0 (never reached): every pixel gets --spp-max passes in blocks of --step
  adaptive   slrhip_render_adaptive at --threshold (default: found by bisection over renders to the sample limit, so that about
             half of the pixels have retired by then) in the same blocks, spp_min = --step
  machinery  both with a threshold / target of 0 and blocks of 64 passes: nobody retires (but the pixels whose samples are all
             equal), so the difference is the cost of the select launches, the 4-byte read-back and the indexed fold

alternating, median of --reps after one warm-up render; per block of the adaptive run the active pixels and the samples per second,
which fall once few pixels are left (a small window on a slot count sized for the whole shard).  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402


def begin(ctx, st):
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.synchronize()


def uniform(ctx, st, step, spp_max):
    begin(ctx, st)
    t0 = time.perf_counter()
    done, summary = ctx.render_until(abi.NOISE_RELATIVE, 0.0, step, spp_max)
    ctx.synchronize()
    return dict(seconds=time.perf_counter() - t0, spp_done=done, samples=summary["samples"], relative=abi.noise_metric(summary, abi.NOISE_RELATIVE))


def adaptive(ctx, st, threshold, floor, step, spp_max):
    begin(ctx, st)
    t0 = time.perf_counter()
    done, samples = ctx.render_adaptive(0, threshold, floor, step, step, spp_max)
    ctx.synchronize()
    seconds = time.perf_counter() - t0
    return dict(seconds=seconds, spp_done=done, samples=samples, active=ctx.adaptive_active(),
                relative=abi.noise_metric(ctx.statistics_summary(), abi.NOISE_RELATIVE))


def adaptive_blocks(ctx, st, threshold, floor, step, spp_max):
    """The same render, one call per block (spp_min = spp_max = the block: main refuses limits that leave a block of one pass):
    active pixels before the block, its wall time and its samples per second."""
    begin(ctx, st)
    rows, at = [], 0
    while at < spp_max and ctx.adaptive_active():
        active, n = ctx.adaptive_active(), min(step, spp_max - at)
        t0 = time.perf_counter()
        done, samples = ctx.render_adaptive(at, threshold, floor, n, step, n)
        seconds = time.perf_counter() - t0
        rows.append(dict(spp_begin=at, active=active, samples=samples, seconds=round(seconds, 5), msamples_per_s=round(samples / seconds / 1e6, 1)))
        at += done
    return rows


def find_threshold(ctx, st, floor, step, spp_max, pixels):
    """Bisection (in log2) for the threshold at which about half of the pixels have retired by spp_max."""
    lo, hi = 2.0 ** -16, 1.0
    for _ in range(10):
        mid = float(np.sqrt(lo * hi))
        begin(ctx, st)
        ctx.render_adaptive(0, mid, floor, step, step, spp_max)
        if ctx.adaptive_active() > pixels // 2:
            lo = mid
        else:
            hi = mid
    return float(np.float32(np.sqrt(lo * hi)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp-max", type=int, default=256)
    ap.add_argument("--step", type=int, default=16)
    ap.add_argument("--threshold", type=float, default=None)
    ap.add_argument("--floor", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    args = ap.parse_args()
    if args.step < 2 or args.spp_max < args.step or args.spp_max % args.step == 1:
        ap.error("--step must be at least 2 and --spp-max at least --step, and the last block must not be a single pass (spp_min >= 2)")
    w, h = args.width, args.height
    sc = scenes.cornell_box_spheres(w / h, 48, 24, "matte")
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    ctx = Context(mode=abi.MODE_RGB)
    ctx.upload_scene(sc)
    uniform(ctx, st, 64, 64)                             # warm-up
    threshold = args.threshold if args.threshold is not None else find_threshold(ctx, st, args.floor, args.step, args.spp_max, w * h)
    out = dict(width=w, height=h, spp_max=args.spp_max, step=args.step, threshold=threshold, floor=args.floor, pixels=w * h)
    runs = {"uniform": [], "adaptive": [], "machinery_uniform": [], "machinery_adaptive": []}
    for _ in range(args.reps):                           # alternating
        runs["uniform"].append(uniform(ctx, st, args.step, args.spp_max))
        runs["adaptive"].append(adaptive(ctx, st, threshold, args.floor, args.step, args.spp_max))
        runs["machinery_uniform"].append(uniform(ctx, st, 64, args.spp_max))
        runs["machinery_adaptive"].append(adaptive(ctx, st, 0.0, args.floor, 64, args.spp_max))
    for name, rs in runs.items():
        out[name] = dict(rs[-1], seconds=float(np.median([r["seconds"] for r in rs])), runs=[round(r["seconds"], 4) for r in rs])
        out[name]["msamples_per_s"] = round(out[name]["samples"] / out[name]["seconds"] / 1e6, 1)
    out["adaptive_speedup"] = out["uniform"]["seconds"] / out["adaptive"]["seconds"]
    out["machinery_overhead"] = out["machinery_adaptive"]["seconds"] / out["machinery_uniform"]["seconds"] - 1.0
    out["adaptive_blocks"] = adaptive_blocks(ctx, st, threshold, args.floor, args.step, args.spp_max)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
