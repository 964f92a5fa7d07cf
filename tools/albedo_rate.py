"""Time of the albedo pass (slrhip_render_albedo) against the feature pass of the SAME build on the same scene
(slrhip_render_features(SHADING_NORMAL | DISTANCE | COVERAGE): the same traversal, another fold), and of slrhip_modulate against
slrhip_tonemap, at 1280x720, RGB and spectral.  Device-event times, median of --reps after one warm-up call.  Prints one JSON line
per (scene, mode)."""
import argparse
import json
import os
import sys

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402

GUIDES = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE
SCENES = {"cornell_textured": lambda aspect: scenes.cornell_textured(aspect, 48, 24),
          "cornell_multi": lambda aspect: scenes.cornell_multi(aspect, 48, 24)}


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
    ap.add_argument("--scene", action="append", choices=sorted(SCENES))
    ap.add_argument("--passes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    w, h = 1280, 720
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    s = torch.cuda.current_stream()
    for name in args.scene or sorted(SCENES):
        sc = SCENES[name](w / h)
        for mode, comps in ((abi.MODE_RGB, 3), (abi.MODE_SPECTRAL, 16)):
            ctx = Context(mode=mode)
            ctx.upload_scene(sc)
            out = {"scene": name, "mode": "spectral" if comps == 16 else "rgb", "passes": args.passes, "width": w, "height": h}
            ctx.render_begin(st)
            out["features_ms"], out["features_runs"] = timed(lambda: ctx.render_features(GUIDES, args.passes, 0, stream=s), args.reps)
            ctx.render_begin(st)
            out["albedo_ms"], out["albedo_runs"] = timed(lambda: ctx.render_albedo(args.passes, 0, stream=s), args.reps)
            out["albedo_over_features"] = round(out["albedo_ms"] / out["features_ms"], 3)
            out["features_status"] = ctx.features_status(s)
            albedo = torch.empty((h, w, comps), dtype=torch.float32, device="cuda")
            passes = ctx.albedo_into(albedo.data_ptr(), albedo.numel(), stream=s)
            color = torch.rand((h, w, comps), dtype=torch.float32, device="cuda")
            variance = torch.rand((h, w), dtype=torch.float32, device="cuda")
            image = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            out["modulate_ms"], out["modulate_runs"] = timed(
                lambda: ctx.modulate_into(w, h, comps, abi.MODULATE_DIVIDE, color.data_ptr(), albedo.data_ptr(), passes, color.data_ptr(),
                                          variance.data_ptr(), variance.data_ptr(), stream=s), args.reps)
            # the same call over buffers that do not stay in the 256 MB last-level cache: a ring of sets of more than 1 GiB in all, every
            # call on the set used longest ago; the time is per call
            per_set = 4 * (3 * h * w * comps + h * w)
            sets = [(torch.rand((h, w, comps), dtype=torch.float32, device="cuda"), albedo.clone(), torch.rand((h, w), dtype=torch.float32, device="cuda"),
                     torch.empty((h, w, comps), dtype=torch.float32, device="cuda")) for _ in range((1 << 30) // per_set + 2)]
            ms, runs = timed(lambda: [ctx.modulate_into(w, h, comps, abi.MODULATE_DIVIDE, c.data_ptr(), a.data_ptr(), passes, o.data_ptr(),
                                                        v.data_ptr(), None, stream=s) for c, a, v, o in sets], args.reps)
            out["modulate_cold_ms"], out["modulate_cold_sets"], out["modulate_cold_bytes_per_call"] = ms / len(sets), len(sets), per_set - 4 * h * w
            del sets
            out["tonemap_ms"], out["tonemap_runs"] = timed(
                lambda: ctx.tonemap_into(w, h, comps, color.data_ptr(), image.data_ptr(), image.numel(), 1.0, abi.IMAGE_RGBA8, stream=s), args.reps)
            ctx.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
