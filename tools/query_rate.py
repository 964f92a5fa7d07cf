"""Ray-query rates: slrhip_intersect_rays / slrhip_test_visibility (the render's wave-specialised traversal fed from a device ray
array) next to slrhip_trace_rays (the 64-ray batch kernel) on the same rays.

Scenes: the headline Cornell box (float nodes), grid10m (10 M triangles, device LBVH, quantized nodes) and the 1 250-instance grid.
Rays: `camera` = 4 Mi rays from the camera position through a grid over the scene's box in image order (coherent); `secondary` =
4 Mi rays from the camera rays' hit points in uniformly random directions (incoherent), dist_min = 1e-4 x the scene's diagonal.

Query times are device-event times of one call (median of --reps).  slrhip_trace_rays copies through the host and synchronises:
its wall time is printed, and its KERNEL time comes from a run of this script under
    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/query_rate.py
(k_trace_batch vs k_ring_ws<..., WsQueryIO> in the stats file).  One JSON line per (scene, ray set); --out appends them to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402


def bounds(sc):
    pos = sc.vertices["position"].astype(np.float64)
    tri = sc.triangles["v"]
    mesh = np.zeros(len(tri), bool)
    pts = []
    for rec in sc.instances:
        first, num = int(rec["first_triangle"]), int(rec["num_triangles"])
        mesh[first:first + num] = True
        p = pos[tri[first:first + num].reshape(-1)]
        lo, hi = p.min(0), p.max(0)
        c = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        pts.append((c @ np.asarray(rec["local_to_world"], np.float64).reshape(4, 4))[:, :3])     # column-major storage: row vector x M^T
    pts.append(pos[tri[~mesh].reshape(-1)])
    pts = np.concatenate(pts)
    return pts.min(0), pts.max(0)


def camera_rays(sc, n):
    lo, hi = bounds(sc)
    side = int(np.sqrt(n))
    cam = np.array(sc.camera.local_to_world[12:15], np.float64)
    axes = np.argsort(hi - lo)[::-1]
    u, v = np.meshgrid((np.arange(side) + 0.5) / side, (np.arange(side) + 0.5) / side, indexing="xy")
    tgt = np.tile((lo + hi) / 2, (side * side, 1))
    tgt[:, axes[0]] = lo[axes[0]] + (hi - lo)[axes[0]] * u.reshape(-1)
    tgt[:, axes[1]] = lo[axes[1]] + (hi - lo)[axes[1]] * v.reshape(-1)
    d = tgt - cam
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((side * side, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = cam, 0.0, d, np.inf
    return r, float(np.linalg.norm(hi - lo))


def secondary_rays(rows, hits, diag, seed=1):
    rng = np.random.default_rng(seed)
    tri = np.ascontiguousarray(hits[:, 0]).view(np.uint32)
    keep = tri != abi.MISS
    o = rows[keep, 0:3].astype(np.float64) + rows[keep, 4:7].astype(np.float64) * hits[keep, 1:2].astype(np.float64)
    o = np.resize(o, (len(rows), 3))
    d = rng.normal(size=(len(rows), 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((len(rows), 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 1e-4 * diag, d, np.inf
    return r


def timed(torch, fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scenes", default="cornell,grid10m,instanced_grid")
    ap.add_argument("--no-batch", action="store_true", help="skip slrhip_trace_rays")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    makers = {"cornell": (lambda: scenes.cornell_box_spheres(16.0 / 9.0, 48, 24, "glass"), 0),
              "grid10m": (lambda: scenes.displaced_grid(2236, 16.0 / 9.0), abi.FLAG_BVH_DEVICE_BUILD),
              "instanced_grid": (lambda: scenes.instanced_grid(25, 50, 64, 16.0 / 9.0), 0)}
    for name in args.scenes.split(","):
        make, flags = makers[name]
        sc = make()
        ctx = Context(flags=flags)
        ctx.upload_scene(sc)
        cam, diag = camera_rays(sc, args.rays)
        first = ctx.intersect_rays(cam)
        for kind, rows in (("camera", cam), ("secondary", secondary_rays(cam, first, diag))):
            r = torch.from_numpy(rows).cuda()
            ctx.intersect_rays(r), ctx.test_visibility(r)          # warm-up
            torch.cuda.synchronize()
            ms_c = timed(torch, lambda: ctx.intersect_rays(r), args.reps)
            ms_v = timed(torch, lambda: ctx.test_visibility(r), args.reps)
            assert ctx.query_status() == 0
            hits = ctx.intersect_rays(rows)
            rec = {"scene": name, "rays": kind, "n": len(rows), "hit_fraction": float((np.ascontiguousarray(hits[:, 0]).view(np.uint32) != abi.MISS).mean()),
                   "intersect_ms": ms_c, "intersect_grays": len(rows) / ms_c / 1e6,
                   "visibility_ms": ms_v, "visibility_grays": len(rows) / ms_v / 1e6}
            if not args.no_batch:
                t0 = time.perf_counter()
                ctx.trace_rays(rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7])
                rec["trace_rays_wall_ms"] = (time.perf_counter() - t0) * 1e3
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")
        ctx.close()


if __name__ == "__main__":
    main()
