"""What moving every placement costs: slrhip_set_instance_transforms (matrices already on the device, the top-level tree refitted
there) next to the only route there was before it, a full slrhip_upload_scene; and what the refitted tree costs the rays.

The instanced BASELINE grid (scenes.instanced_grid: 1 250 placements of an 8 192-triangle patch).
  (a) milliseconds per call of all 1 250 placements: --batch calls back to back on one stream between two HIP events
      (torch.cuda.Event) so that the window is not a single launch gap, divided by the batch; one warm-up batch, the median, fastest
      and slowest of --reps batches.  Beside it what a caller pays without the call: slrhip_counters::build_seconds of an upload of
      the same scene (the host build alone) and the host clock around the whole slrhip_upload_scene (which synchronises).
  (b) Msamples/s (host clock around slrhip_render, which blocks; one warm-up render) and nodes visited per ray (a second context
      with SLRHIP_FLAG_COUNT_TRAVERSAL, whose rate is not reported) after a fresh upload and after an identity update: the tree is
      the same, so the node counts must be equal.
  (c) the same after the placements were permuted among the instances — the picture is the same, the tree's shape is now wrong for
      it, the worst case of a refit — and after a fresh upload of the permuted scene, which is the remedy.
Frames of the refitted and the freshly uploaded context are compared bit for bit.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import binding as ob  # noqa: E402
from slr_amd import Context, abi, scenes  # noqa: E402


def spread(values):
    return dict(median_ms=float(np.median(values)), min_ms=float(min(values)), max_ms=float(max(values)))


def records(sc):
    return np.ascontiguousarray(np.concatenate([sc.instances["local_to_world"], sc.instances["world_to_local"]], axis=1), np.float32)


def with_records(sc, rec):
    inst = sc.instances.copy()
    inst["local_to_world"], inst["world_to_local"] = rec[:, :16], rec[:, 16:]
    return abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, None, sc.name, instances=inst)


def render_rate(ctx, st, spp, reps):
    """(frame, Msamples/s spread as ms per render, samples per render)"""
    ms = []
    for i in range(1 + reps):
        ctx.render_begin(st)
        t0 = time.perf_counter()
        ctx.render(0, spp)
        if i >= 1:
            ms.append((time.perf_counter() - t0) * 1e3)
    samples = int(ctx.counters().samples)
    t = spread(ms)
    t["msamples_per_second"] = samples / (t["median_ms"] * 1e-3) / 1e6
    return ctx.read_framebuffer(), t


def nodes_per_ray(ctx, st, spp):
    ctx.render_begin(st)
    ctx.render(0, spp)
    p = ctx.profile()
    return dict(closest=p.nodes[0] / max(1, p.rays[0]), shadow=p.nodes[1] / max(1, p.rays[1]), nodes=[int(p.nodes[0]), int(p.nodes[1])],
                rays=[int(p.rays[0]), int(p.rays[1])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--cells", type=int, default=64)
    args = ap.parse_args()
    sc = scenes.instanced_grid(cells=args.cells, aspect=args.width / args.height)
    st = ob.settings(args.width, args.height, seed=11)
    rec = records(sc)
    perm = rec[np.random.default_rng(1).permutation(len(rec))]
    out = dict(reps=args.reps, warmup=1, batch=args.batch, instances=len(rec), triangles_per_instance=int(sc.instances["num_triangles"][0]),
               frame=[args.width, args.height], spp=args.spp)

    ctx, count = Context(), Context(flags=abi.FLAG_COUNT_TRAVERSAL)
    upload_ms, build_s = [], []
    for i in range(1 + args.reps):
        t0 = time.perf_counter()
        ctx.upload_scene(sc)
        if i >= 1:
            upload_ms.append((time.perf_counter() - t0) * 1e3)
            build_s.append(float(ctx.counters().build_seconds))
    count.upload_scene(sc)
    top = ctx.debug_top_level()
    out["top_level"] = dict(nodes=int(top["top_nodes"]), level_widths=np.diff(top["levels"]).tolist(), single_workgroup_up_to=top["group_nodes"])
    out["upload_scene"] = dict(spread(upload_ms), build_seconds_median=float(np.median(build_s)))

    # (a) the call
    stream = torch.cuda.current_stream(ctx.device)
    dev = {k: torch.from_numpy(v).to("cuda:%d" % ctx.device) for k, v in (("identity", rec), ("permuted", perm))}
    for which in ("identity", "permuted"):
        ms = []
        for i in range(1 + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.batch):
                ctx.set_instance_transforms(dev[which], stream=stream)
            b.record(stream)
            b.synchronize()
            if i >= 1:
                ms.append(a.elapsed_time(b) / args.batch)
        out["set_instance_transforms_" + which] = spread(ms)
    assert ctx.instances_status(stream) == 0
    out["upload_over_call"] = out["upload_scene"]["median_ms"] / out["set_instance_transforms_permuted"]["median_ms"]

    # (b) fresh upload against identity update
    ctx.upload_scene(sc)
    fresh_frame, out["render_fresh_upload"] = render_rate(ctx, st, args.spp, args.reps)
    out["nodes_per_ray_fresh_upload"] = nodes_per_ray(count, st, args.spp)
    for c in (ctx, count):
        c.set_instance_transforms(dev["identity"], stream=stream)
    stream.synchronize()
    frame, out["render_identity_update"] = render_rate(ctx, st, args.spp, args.reps)
    out["nodes_per_ray_identity_update"] = nodes_per_ray(count, st, args.spp)
    out["identity_frame_bit_equal"] = bool(np.array_equal(frame.view(np.uint32), fresh_frame.view(np.uint32)))
    out["identity_nodes_equal"] = out["nodes_per_ray_identity_update"]["nodes"] == out["nodes_per_ray_fresh_upload"]["nodes"]

    # (c) the permutation: refitted, then rebuilt
    for c in (ctx, count):
        c.set_instance_transforms(dev["permuted"], stream=stream)
    stream.synchronize()
    refit_frame, out["render_permuted_refit"] = render_rate(ctx, st, args.spp, args.reps)
    out["nodes_per_ray_permuted_refit"] = nodes_per_ray(count, st, args.spp)
    moved = with_records(sc, perm)
    for c in (ctx, count):
        c.upload_scene(moved)
    frame, out["render_permuted_upload"] = render_rate(ctx, st, args.spp, args.reps)
    out["nodes_per_ray_permuted_upload"] = nodes_per_ray(count, st, args.spp)
    out["permuted_frame_bit_equal"] = bool(np.array_equal(frame.view(np.uint32), refit_frame.view(np.uint32)))
    out["refit_slowdown_render"] = out["render_permuted_refit"]["median_ms"] / out["render_permuted_upload"]["median_ms"]
    out["refit_nodes_factor_closest"] = out["nodes_per_ray_permuted_refit"]["closest"] / out["nodes_per_ray_permuted_upload"]["closest"]
    ctx.close()
    count.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
