"""What repairing the top-level tree on the device costs and buys: slrhip_rebuild_top_level next to slrhip_set_instance_transforms
(the refit alone) and slrhip_upload_scene (the remedy there was before it), from one run.

The instanced BASELINE grid (scenes.instanced_grid: 1 250 placements of an 8 192-triangle patch), 960 x 540, 16 spp.
  (a) four states of the tree — fresh upload; placements permuted among the instances, refit only; the same, refit + rebuild; fresh
      upload of the permuted scene — and for each: milliseconds per render (host clock around slrhip_render, which blocks; one warm-up
      render), nodes visited per closest-hit and per shadow ray (a second context with SLRHIP_FLAG_COUNT_TRAVERSAL, whose rate is
      not reported), and slrhip_top_level_cost.  The frames of the three permuted states are compared bit for bit.
  (b) milliseconds per call: --batch calls back to back on one stream between two HIP events (torch.cuda.Event), divided by the
      batch; one warm-up batch, the median, fastest and slowest of --reps batches — slrhip_rebuild_top_level on the one-workgroup
      path (the BASELINE grid's 1 251 primitives) and on the radix-sort path (an 80 x 64 grid of small patches: 5 121 primitives),
      slrhip_set_instance_transforms of all placements on both, and the host clock around slrhip_upload_scene (which synchronises),
      with the launches of each rebuild call (the refit's included, the radix sort counted as one).
One JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from instance_update_rate import nodes_per_ray, records, render_rate, spread, with_records  # noqa: E402
from oracle import binding as ob  # noqa: E402
from slr_amd import Context, abi, scenes  # noqa: E402


def per_call(stream, batch, reps, call):
    ms = []
    for i in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(batch):
            call()
        b.record(stream)
        b.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b) / batch)
    return spread(ms)


def call_timing(ctx, sc, perm, args):
    """The calls on `sc`: upload, set_instance_transforms of every placement (permuted), rebuild_top_level."""
    out = dict(instances=len(perm))
    upload_ms = []
    for i in range(1 + args.reps):
        t0 = time.perf_counter()
        ctx.upload_scene(sc)
        if i >= 1:
            upload_ms.append((time.perf_counter() - t0) * 1e3)
    out["upload_scene"] = spread(upload_ms)
    stream = torch.cuda.current_stream(ctx.device)
    dev = torch.from_numpy(perm).to("cuda:%d" % ctx.device)
    out["set_instance_transforms"] = per_call(stream, args.batch, args.reps, lambda: ctx.set_instance_transforms(dev, stream=stream))
    assert ctx.instances_status(stream) == 0
    ctx.rebuild_top_level(stream)                      # the first call builds the tables and synchronises: not part of the timing
    out["rebuild_top_level"] = per_call(stream, args.batch, args.reps, lambda: ctx.rebuild_top_level(stream))
    info = ctx.debug_top_level_rebuild()
    out.update(primitives=info["primitives"], path=info["path"], launches=info["launches"], seat_group=info["seat_group"])
    out["upload_over_rebuild"] = out["upload_scene"]["median_ms"] / out["rebuild_top_level"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sc = scenes.instanced_grid(cells=args.cells, aspect=args.width / args.height)
    st = ob.settings(args.width, args.height, seed=11)
    rec = records(sc)
    perm = rec[np.random.default_rng(1).permutation(len(rec))]
    out = dict(reps=args.reps, warmup=1, batch=args.batch, instances=len(rec), triangles_per_instance=int(sc.instances["num_triangles"][0]),
               frame=[args.width, args.height], spp=args.spp)

    ctx, count = Context(), Context(flags=abi.FLAG_COUNT_TRAVERSAL)
    frames = {}

    def state(name):
        frames[name], render = render_rate(ctx, st, args.spp, args.reps)
        out[name] = dict(render=render, nodes_per_ray=nodes_per_ray(count, st, args.spp), top_level_cost=ctx.top_level_cost())
        assert out[name]["top_level_cost"] == count.top_level_cost()

    # (a) the four states
    for c in (ctx, count):
        c.upload_scene(sc)
    state("fresh_upload")
    for c in (ctx, count):
        c.set_instance_transforms(perm)
    state("permuted_refit_only")
    for c in (ctx, count):
        c.rebuild_top_level()
    state("permuted_refit_and_rebuild")
    for c in (ctx, count):
        c.upload_scene(with_records(sc, perm))
    state("permuted_fresh_upload")
    out["permuted_frames_bit_equal"] = bool(np.array_equal(frames["permuted_refit_only"].view(np.uint32), frames["permuted_refit_and_rebuild"].view(np.uint32))
                                            and np.array_equal(frames["permuted_refit_only"].view(np.uint32), frames["permuted_fresh_upload"].view(np.uint32)))
    ms = {k: out[k]["render"]["median_ms"] for k in frames}
    out["render_refit_only_over_upload"] = ms["permuted_refit_only"] / ms["permuted_fresh_upload"]
    out["render_rebuild_over_upload"] = ms["permuted_refit_and_rebuild"] / ms["permuted_fresh_upload"]
    count.close()

    # (b) the calls, on both paths
    out["calls_small_path"] = call_timing(ctx, sc, perm, args)
    wide = scenes.instanced_grid(tiles_x=80, tiles_z=64, cells=2, aspect=args.width / args.height)
    wide_rec = records(wide)
    out["calls_large_path"] = call_timing(ctx, wide, wide_rec[np.random.default_rng(1).permutation(len(wide_rec))], args)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
