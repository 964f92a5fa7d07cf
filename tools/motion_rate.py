"""What a motion call costs on the 10 M-triangle grid at the bench resolution, with and without moved vertices.

The scene is bench.py's grid10m (scenes.displaced_grid) in a context created with FLAG_DYNAMIC_GEOMETRY (--tree device | host; SLRHIP_BVH is
set before the library loads).  Every vertex is then displaced by up to half a cell (seed 5: the displacement of DESIGN.md 7.23) with
slrhip_set_vertices, and the camera moves a little, so the previous frame differs in both.  One call of --spp passes (the trace plus the
fold) is bracketed by two HIP events on one stream (torch.cuda.Event), in two forms:
  (a) slrhip_render_motion: vertices taken to stand still (k_motion_fold<false>);
  (b) slrhip_render_motion_vertices with the uploaded vertices as the previous frame's (k_motion_fold<true>).
The first call of each form after render_begin allocates and is not timed; after --warmup further calls the forms alternate, --reps times;
the median, the fastest and the slowest call of each are reported, and (b) / (a).  --forms a measures (a) alone: a library from before
slrhip_render_motion_vertices (SLRHIP_LIBRARY) has no (b).  The kernels' shares come from a run of this script under
`rocprofv3 --kernel-trace --stats` of its own.  Appends one JSON line to <out-dir>/motion_rate.txt."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(values):
    return dict(median_ms=float(np.median(values)), min_ms=float(min(values)), max_ms=float(max(values)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default="device", choices=["device", "host"])
    ap.add_argument("--grid-n", type=int, default=2236)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--forms", default="a,b")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    forms = args.forms.split(",")
    os.environ["SLRHIP_BVH"] = args.tree          # read once, when the first scene is prepared

    import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime
    from oracle import binding as ob
    from slr_amd import Context, abi, scenes

    aspect = args.width / args.height
    sc = scenes.displaced_grid(args.grid_n, aspect)
    reach = 0.5 * 8.0 / args.grid_n               # half a cell of the grid
    n = len(sc.vertices)
    moved = sc.vertices.copy()
    moved["position"] = (moved["position"].astype(np.float64) + np.random.default_rng(5).uniform(-reach, reach, (n, 3))).astype(np.float32)
    ctx = Context(flags=abi.FLAG_DYNAMIC_GEOMETRY | (abi.FLAG_BVH_DEVICE_BUILD if args.tree == "device" else 0))
    ctx.upload_scene(sc)
    dev = "cuda:%d" % ctx.device
    stream = torch.cuda.current_stream(ctx.device)
    previous = torch.from_numpy(np.ascontiguousarray(sc.vertices).view(np.float32).reshape(-1, 11)).to(dev)
    now = torch.from_numpy(np.ascontiguousarray(moved).view(np.float32).reshape(-1, 11)).to(dev)
    ctx.set_vertices(now, stream=stream)
    assert ctx.geometry_status(stream) == 0
    c = sc.camera
    m = np.array(c.local_to_world[:], np.float64).reshape(4, 4).T
    prev_cam = scenes.make_camera(scenes._translate(0.04, 0.02, -0.05) @ m, c.aspect, c.fov_y, c.lens_radius, c.img_plane_distance, c.obj_plane_distance,
                                  c.sensitivity)
    ctx.render_begin(ob.settings(args.width, args.height, seed=11))

    def call(form):
        ctx.render_motion(args.spp, prev_cam, stream=stream, previous_vertices=previous if form == "b" else None)
    ms = {f: [] for f in forms}
    for i in range(1 + args.warmup + args.reps):
        for f in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call(f)
            b.record(stream)
            b.synchronize()
            if i >= 1 + args.warmup:
                ms[f].append(a.elapsed_time(b))
    assert ctx.features_status(stream) == 0
    sums = ctx.motion()
    samples = args.width * args.height * args.spp
    out = dict(label=args.label, scene=sc.name, tree=args.tree, vertices=n, triangles=len(sc.triangles), frame=[args.width, args.height], spp=args.spp,
               warmup=args.warmup, reps=args.reps, perturb_reach=reach, hit_fraction=float((sums[..., 3] > 0).mean()), finite=bool(np.isfinite(sums).all()))
    for f in forms:
        out[f] = dict(spread(ms[f]), ns_per_sample=float(np.median(ms[f])) * 1e6 / samples)
    if "a" in forms and "b" in forms:
        out["b_over_a"] = out["b"]["median_ms"] / out["a"]["median_ms"]
    ctx.close()
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "motion_rate.txt"), "a") as f:
        f.write(json.dumps(out) + "\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
