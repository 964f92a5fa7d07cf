"""What moving every vertex costs: slrhip_set_vertices (records already on the device; leaf, shading and light records rewritten and
the tree refitted there) next to the only route there was before it, a full slrhip_upload_scene; and what the refitted tree costs the
rays.

One scene per run (--scene grid: scenes.displaced_grid, 10 M triangles; --scene cornell: the bench scene; --scene instanced:
scenes.instanced_grid, --tiles-x x --tiles-z placements of one patch of 2 x --cells^2 triangles, in a context created with
FLAG_DYNAMIC_INSTANCED as well — the two-level host build, whatever --tree says) with one tree builder (--tree device | host; SLRHIP_BVH is
set before the library loads, so a run measures one builder).
  (a) milliseconds per call on the whole vertex array: --batch calls back to back on one stream between two HIP events
      (torch.cuda.Event) and a stream synchronise, divided by the batch; one warm-up batch, the median, fastest and slowest of --reps
      batches; the launches per call.  Beside it, same box and same run: slrhip_counters::build_seconds of an upload of the same
      scene and the host clock around the whole slrhip_upload_scene (which synchronises).
  (b) traversal nodes per ray (a context with SLRHIP_FLAG_COUNT_TRAVERSAL) as uploaded, after an identity update (the tree is the
      same: the counts must be equal), after `perturb` (every vertex displaced by up to half a cell, seeded) refitted, and after a
      fresh upload of the perturbed scene, which is the remedy.  Frames of the refitted and the freshly uploaded context are compared
      bit for bit.  render_ms is the host clock around that render in the COUNTING context (slower than a plain one; comparable among
      the states of one run only).
Appends one JSON line to <out-dir>/vertex_update_rate.txt (a) and one to <out-dir>/vertex_update_tree_quality.txt (b)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values):
    return dict(median_ms=float(np.median(values)), min_ms=float(min(values)), max_ms=float(max(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="grid", choices=["grid", "cornell", "instanced"])
    ap.add_argument("--tree", default="device", choices=["device", "host"])
    ap.add_argument("--grid-n", type=int, default=2236)
    ap.add_argument("--tiles-x", type=int, default=25)
    ap.add_argument("--tiles-z", type=int, default=50)
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--uploads", type=int, default=2)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    os.environ["SLRHIP_BVH"] = args.tree          # read once, when the first scene is prepared

    import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime
    from oracle import binding as ob
    from slr_amd import Context, abi, scenes

    aspect = args.width / args.height
    if args.scene == "grid":
        sc = scenes.displaced_grid(args.grid_n, aspect)
        reach = 0.5 * 8.0 / args.grid_n           # half a cell of the grid (extent 4)
    elif args.scene == "instanced":
        sc = scenes.instanced_grid(args.tiles_x, args.tiles_z, args.cells, aspect)
        reach = 0.5 * 2.0 / args.cells            # half a cell of the patch (local extent 2)
    else:
        sc = scenes.cornell_box_spheres(aspect, 48, 24, "matte")
        reach = 0.01
    st = ob.settings(args.width, args.height, seed=11)
    flags = abi.FLAG_DYNAMIC_GEOMETRY | (abi.FLAG_BVH_DEVICE_BUILD if args.tree == "device" else 0)
    if args.scene == "instanced":
        flags = abi.FLAG_DYNAMIC_GEOMETRY | abi.FLAG_DYNAMIC_INSTANCED
    n = len(sc.vertices)
    moved = sc.vertices.copy()
    moved["position"] = (moved["position"].astype(np.float64) + np.random.default_rng(5).uniform(-reach, reach, (n, 3))).astype(np.float32)
    sc_moved = abi.Scene(moved, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, None, sc.name + "_perturbed",
                         instances=sc.instances if len(sc.instances) else None)
    head = dict(scene=sc.name, tree=args.tree, vertices=n, triangles=len(sc.triangles), instances=len(sc.instances), reps=args.reps, warmup=1,
                batch=args.batch)

    # (a) the call, next to the upload
    ctx = Context(flags=flags)
    upload_ms, build_s = [], []
    for i in range(1 + args.uploads):
        t0 = time.perf_counter()
        ctx.upload_scene(sc)
        if i >= 1:
            upload_ms.append((time.perf_counter() - t0) * 1e3)
            build_s.append(float(ctx.counters().build_seconds))
    tree = ctx.debug_tree(summary_only=True)
    rate = dict(head, builder=tree["builder_name"], nodes=tree["num_nodes"], depth=tree["depth"], quantized=tree["quantized"],
                upload_scene=dict(spread(upload_ms), build_seconds_median=float(np.median(build_s))))
    stream = torch.cuda.current_stream(ctx.device)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.float32).reshape(-1, 11)).to("cuda:%d" % ctx.device)
           for k, v in (("identity", sc.vertices), ("perturbed", moved))}
    for which in ("identity", "perturbed"):
        ms = []
        for i in range(1 + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            for _ in range(args.batch):
                ctx.set_vertices(dev[which], stream=stream)
            b.record(stream)
            b.synchronize()
            if i >= 1:
                ms.append(a.elapsed_time(b) / args.batch)
        rate["set_vertices_" + which] = spread(ms)
    assert ctx.geometry_status(stream) == 0
    geo_levels = ctx.debug_geometry()
    rate["launches_per_call"] = geo_levels["launches"]
    rate["level_widths"] = np.diff(geo_levels["levels"]).tolist()
    if geo_levels["instanced"]:
        rate["mesh_level_widths"] = np.diff(geo_levels["mesh_levels"]).tolist()
        rate["meshes"] = geo_levels["num_meshes"]
    # the bytes one call must move: the caller's records in and the kept ones out, the indices, and every rewritten record in and out
    nt, nn = len(sc.triangles), tree["num_nodes"]
    rate["bytes_per_call"] = int(n * 88 + nt * (16 * 2 + 48 * 2 + 32 * 2 + 96 * 2 + 3 * 44 * 2) + nn * (128 * 2 + (64 if tree["quantized"] else 0)))
    rate["fraction_of_8TBps"] = rate["bytes_per_call"] / (rate["set_vertices_perturbed"]["median_ms"] * 1e-3) / 8e12
    rate["upload_over_call"] = rate["upload_scene"]["median_ms"] / rate["set_vertices_perturbed"]["median_ms"]
    ctx.close()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "vertex_update_rate.txt"), "a") as f:
        f.write(json.dumps(rate) + "\n")
    print(json.dumps(rate), flush=True)

    # (b) what the refitted tree costs the rays
    def nodes_per_ray(c):
        c.render_begin(st)
        t0 = time.perf_counter()
        c.render(0, args.spp)
        c.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        p = c.profile()
        return dict(render_ms=ms, closest=p.nodes[0] / max(1, p.rays[0]), shadow=p.nodes[1] / max(1, p.rays[1]), nodes=[int(p.nodes[0]), int(p.nodes[1])],
                    rays=[int(p.rays[0]), int(p.rays[1])]), c.read_framebuffer()

    count = Context(flags=flags | abi.FLAG_COUNT_TRAVERSAL)
    count.upload_scene(sc)
    quality = dict(head, frame=[args.width, args.height], spp=args.spp, perturb_reach=reach)
    quality["as_uploaded"], _ = nodes_per_ray(count)
    count.set_vertices(dev["identity"], stream=stream)
    stream.synchronize()
    quality["identity_update"], _ = nodes_per_ray(count)
    quality["identity_nodes_equal"] = quality["identity_update"]["nodes"] == quality["as_uploaded"]["nodes"]
    count.set_vertices(dev["perturbed"], stream=stream)
    stream.synchronize()
    quality["perturbed_refit"], refit_frame = nodes_per_ray(count)
    count.upload_scene(sc_moved)
    quality["perturbed_upload"], fresh_frame = nodes_per_ray(count)
    quality["perturbed_frame_bit_equal"] = bool(np.array_equal(refit_frame.view(np.uint32), fresh_frame.view(np.uint32)))
    quality["refit_nodes_factor_closest"] = quality["perturbed_refit"]["closest"] / quality["perturbed_upload"]["closest"]
    quality["refit_nodes_factor_shadow"] = quality["perturbed_refit"]["shadow"] / max(1e-30, quality["perturbed_upload"]["shadow"])
    count.close()
    with open(os.path.join(args.out_dir, "vertex_update_tree_quality.txt"), "a") as f:
        f.write(json.dumps(quality) + "\n")
    print(json.dumps(quality), flush=True)


if __name__ == "__main__":
    main()
