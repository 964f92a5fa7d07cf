"""What temporal reprojection (slrhip_reproject) costs at 1280x720: the call with every guide given (variance, ids, normals, the distance
test on), for 3 components (an RGB context) and 16 (a spectral one).

The inputs are a real pair of frames of the instanced Cornell scene: frame 1 at --spp passes, then the instances move by small
translations and the camera a little, frame 2 at --spp passes with its guides and its motion vectors (slrhip_render_motion) rendered
alongside, all buffers resolved into device memory once.  Each timed call is bracketed by two HIP events on one stream
(torch.cuda.Event), after --warmup calls; the median, the fastest and the slowest of --reps calls are reported.  Against that: the
bytes the definition must move per pixel — the current colour, motion (16 B), coverage, variance, two id words, the normal (12 B); the
previous frame's colour, variance, length, distance, coverage, two id words and normal, each pixel of it counted ONCE although up to
four neighbours fetch it; the three outputs: 12 C + 88 B, 124 B for 3 components and 280 B for 16 — over the HBM rate DESIGN.md 7.2
measures against.  One JSON line."""
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


def call_bytes(pixels, components):
    return pixels * (12 * components + 88)


def moved(records, rng):
    """World translations of up to 3 cm after each placement: T(d) L and W T(-d), column-major records [n, 32]."""
    out = records.copy()
    d = rng.uniform(-0.03, 0.03, (len(records), 3)).astype(np.float32)
    for k in range(len(records)):
        l2w, w2l = records[k, :16].reshape(4, 4).T.astype(np.float64), records[k, 16:].reshape(4, 4).T.astype(np.float64)
        t, ti = np.eye(4), np.eye(4)
        t[:3, 3], ti[:3, 3] = d[k], -d[k].astype(np.float64)
        out[k, :16], out[k, 16:] = (t @ l2w).T.reshape(-1), (w2l @ ti).T.reshape(-1)
    return out


def measure(mode, w, h, spp, warmup, reps):
    ctx = Context(mode=mode)
    sc = scenes.cornell_instanced(w / h, 24, 12, copies=24)
    ctx.upload_scene(sc)
    comps = ctx.components
    dev = "cuda:%d" % ctx.device
    stream = torch.cuda.current_stream(ctx.device)
    guides = (("normal", abi.FEATURE_SHADING_NORMAL, 3), ("distance", abi.FEATURE_DISTANCE, 1), ("coverage", abi.FEATURE_COVERAGE, 1),
              ("ids", abi.FEATURE_IDS, 3))
    want = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE | abi.FEATURE_IDS

    def frame(seed, motion_from=None):
        ctx.render_begin(abi.RenderSettings(w, h, 0.0, 0.0, 1.0, seed))
        ctx.statistics_begin()
        ctx.render(0, spp)
        ctx.render_features(want, spp)
        buf = {"color": torch.empty(h * w * comps, dtype=torch.float32, device=dev), "variance": torch.empty(h * w, dtype=torch.float32, device=dev)}
        ctx.mean_into(buf["color"].data_ptr(), buf["color"].numel(), stream)
        ctx.statistics_into(abi.STATISTICS_VARIANCE_OF_MEAN, buf["variance"].data_ptr(), h * w, stream)
        for name, channel, k in guides:
            buf[name] = torch.empty(h * w * k, dtype=torch.int32 if name == "ids" else torch.float32, device=dev)
            ctx.features_into(channel, buf[name].data_ptr(), buf[name].numel(), stream)
        if motion_from is not None:
            ctx.render_motion(spp, *motion_from, stream=stream)
            buf["motion"] = torch.empty(h * w * 4, dtype=torch.float32, device=dev)
            ctx.motion_into(buf["motion"].data_ptr(), buf["motion"].numel(), stream)
        torch.cuda.synchronize()
        return buf
    rec1 = np.concatenate([sc.instances["local_to_world"], sc.instances["world_to_local"]], axis=1).astype(np.float32)
    one = frame(abi.DEFAULT_SEED)
    ctx.set_instance_transforms(moved(rec1, np.random.default_rng(5)))
    c = sc.camera
    m = np.array(c.local_to_world[:], np.float64).reshape(4, 4).T
    ctx.set_camera(scenes.make_camera(scenes._translate(0.04, 0.02, -0.05) @ m, c.aspect, c.fov_y, c.lens_radius, c.img_plane_distance,
                                      c.obj_plane_distance, c.sensitivity))
    two = frame(abi.DEFAULT_SEED + 1, (sc.camera, torch.from_numpy(rec1).to(dev)))
    out = {name: torch.empty(n, dtype=torch.float32, device=dev) for name, n in (("output", h * w * comps), ("output_variance", h * w), ("output_length", h * w))}
    length = torch.ones(h * w, dtype=torch.float32, device=dev)
    args = dict(color=two["color"].data_ptr(), motion=two["motion"].data_ptr(), coverage=two["coverage"].data_ptr(), variance=two["variance"].data_ptr(),
                ids=two["ids"].data_ptr(), normal=two["normal"].data_ptr(), prev_color=one["color"].data_ptr(), prev_variance=one["variance"].data_ptr(),
                prev_length=length.data_ptr(), prev_distance=one["distance"].data_ptr(), prev_coverage=one["coverage"].data_ptr(),
                prev_ids=one["ids"].data_ptr(), prev_normal=one["normal"].data_ptr(), output=out["output"].data_ptr(),
                output_variance=out["output_variance"].data_ptr(), output_length=out["output_length"].data_ptr())

    def call():
        ctx.reproject_into(w, h, comps, stream=stream, **args)
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    need = call_bytes(w * h, comps)
    median = float(np.median(ms))
    res = dict(components=comps, call=dict(median_ms=median, min_ms=float(min(ms)), max_ms=float(max(ms))), call_bytes=need,
               floor_ms=need / HBM_BYTES_PER_SECOND * 1e3, fraction_of_hbm_rate=need / HBM_BYTES_PER_SECOND / (median * 1e-3),
               bytes_per_second=need / (median * 1e-3), finite=bool(torch.isfinite(out["output"]).all().item()),
               hit_fraction=float((two["coverage"] > 0).float().mean().item()), accepted_fraction=float((out["output_length"] > 1).float().mean().item()))
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    out = dict(width=args.width, height=args.height, spp=args.spp, hbm_bytes_per_second=HBM_BYTES_PER_SECOND, max_history=abi.REPROJECT_MAX_HISTORY,
               sigma_distance=abi.REPROJECT_SIGMA_DISTANCE, min_normal_dot=abi.REPROJECT_MIN_NORMAL_DOT)
    out["rgb"] = measure(abi.MODE_RGB, args.width, args.height, args.spp, args.warmup, args.reps)
    out["spectral"] = measure(abi.MODE_SPECTRAL, args.width, args.height, args.spp, args.warmup, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
