"""Time of the first-hit feature pass (slrhip_render_features) at 1280x720, 16 passes: all channels, IDS | DISTANCE only, and
slrhip_intersect_rays on the very same primary rays (slrhip_camera_rays of each pass, read from HBM) — the cost of traversal
alone.  Device-event times, median of --reps after one warm-up call.  `--rays-from DIR` / `--dump-rays DIR`: load / store the
primary rays as pass_NN.npy, so that a build without the feature pass (SLRHIP_LIBRARY) can run the third measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), [round(m, 3) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="cornell", choices=["cornell", "instanced_grid"])
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=["all_channels", "ids_distance"], help="time one channel set only (for a kernel trace of its own)")
    ap.add_argument("--dump-rays")
    ap.add_argument("--rays-from")
    args = ap.parse_args()
    w, h = 1280, 720
    sc = scenes.cornell_box_spheres(w / h, 48, 24, "matte") if args.scene == "cornell" else scenes.instanced_grid()
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    ctx = Context()
    ctx.upload_scene(sc)
    ctx.render_begin(st)
    out = {"scene": args.scene, "passes": args.passes, "width": w, "height": h}
    s = torch.cuda.current_stream()
    if args.rays_from:
        rays = [torch.from_numpy(np.load(os.path.join(args.rays_from, "pass_%02d.npy" % p))).cuda() for p in range(args.passes)]
    else:
        rays = [ctx.camera_rays(p, device=True)[0] for p in range(args.passes)]
        for name, ch in (("all_channels", abi.FEATURE_ALL), ("ids_distance", abi.FEATURE_IDS | abi.FEATURE_DISTANCE)):
            if args.only and name != args.only:
                continue
            ctx.render_begin(st)          # one channel set per render_begin
            out[name + "_ms"], out[name + "_runs"] = timed(lambda: ctx.render_features(ch, args.passes, 0, stream=s), args.reps)
        out["features_status"] = ctx.features_status(s)
        if args.dump_rays:
            os.makedirs(args.dump_rays, exist_ok=True)
            for p, r in enumerate(rays):
                np.save(os.path.join(args.dump_rays, "pass_%02d.npy" % p), r.cpu().numpy())
    if not args.only:
        out["intersect_rays_ms"], out["intersect_rays_runs"] = timed(lambda: [ctx.intersect_rays(r, stream=s) for r in rays], args.reps)
        out["query_status"] = ctx.query_status(s)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
