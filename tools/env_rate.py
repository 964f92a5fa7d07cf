"""What changing the environment light costs: slrhip_set_environment (texels already on the device, importance map and sampling
tables built there) next to the only route there was before it, a full slrhip_upload_scene with a PRECOMPUTED importance map.

Sizes 2048x1024 and 8192x4096, an RGB and a spectral context.  A: the device call bracketed by two HIP events on one stream
(torch.cuda.Event), one warm-up, the median, fastest and slowest of --reps calls; the warm-up also allocates, so the timed calls
reuse the context's arrays.  Against that: the bytes the kernels must move (12 B read and 12 B written per texel by the store, 12 B
per texel read again by the importance kernel, the map read twice and the four tables written) over the HBM peak DESIGN.md states
its fractions against.  The 8K image (403 MB) exceeds the 256 MiB last-level cache, the 2K one (25 MB) does not: the second's rate
is a cache rate, not an HBM rate, and is labelled so.  B: the host clock around slrhip_upload_scene (which synchronises) of
ibl_test_scene's geometry with the same image and the importance map computed beforehand by slrhip_env_importance (not timed).
The tables of both routes are compared bit for bit.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, binding, scenes  # noqa: E402

HBM_BYTES_PER_SECOND = 8.0e12          # the peak DESIGN.md 7.2 states its fractions against
LAST_LEVEL_CACHE_BYTES = 256 << 20


def spread(values):
    return dict(median_ms=float(np.median(values)), min_ms=float(min(values)), max_ms=float(max(values)))


def image(width, height):
    """A seeded half-valued sky with a sun: values are irrelevant to the time, not to the comparison of the tables."""
    rng = np.random.default_rng(width)
    t = rng.uniform(0.05, 1.5, (height, width, 3)).astype(np.float32)
    t[height // 5:height // 5 + 8, width // 3:width // 3 + 8] = 900.0
    return t.astype(np.float16).astype(np.float32)


def with_env(sc, env):
    return abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, env, sc.name)


def measure(mode, width, height, reps):
    spectral = mode == abi.MODE_SPECTRAL
    rgb = image(width, height)
    texels = binding.env_texels_to_uvs(rgb) if spectral else rgb
    importance = binding.env_importance(texels, mode)                 # precomputed: the upload's route is not charged for it
    base = scenes.ibl_test_scene(1.0, (64, 32), 24, 12)
    env = (rgb, 4.0, importance) if not spectral else (rgb, 4.0, binding.env_importance(rgb, abi.MODE_RGB), texels, importance)
    scene = with_env(base, env)

    ctx = Context(mode=mode)
    ctx.upload_scene(base)
    stream = torch.cuda.current_stream(ctx.device)
    dev = torch.from_numpy(texels).to("cuda:%d" % ctx.device)
    ms = []
    for i in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        ctx.set_environment_into(dev.data_ptr(), width, height, 4.0, 0, stream)
        b.record(stream)
        b.synchronize()
        if i >= 1:
            ms.append(a.elapsed_time(b))
    got = [ctx.debug_environment(w) for w in (0, 2, 3, 4, 5)]
    ctx.close()

    fresh = Context(mode=mode)
    upload_ms = []
    for i in range(1 + reps):
        t0 = time.perf_counter()
        fresh.upload_scene(scene)
        if i >= 1:
            upload_ms.append((time.perf_counter() - t0) * 1e3)
    want = [fresh.debug_environment(w) for w in (0, 2, 3, 4, 5)]
    fresh.close()

    cells = (width // 4) * (height // 4)
    moved = width * height * 36 + cells * 4 * 2 + (2 * cells + height // 4) * 4 * 3      # store r + w, importance r; map w + r twice; CDF w + r + w, PDF w
    t = spread(ms)
    in_cache = width * height * 12 <= LAST_LEVEL_CACHE_BYTES
    return dict(set_environment=t, upload_scene=spread(upload_ms), upload_over_device_call=float(np.median(upload_ms)) / t["median_ms"],
                image_bytes=width * height * 12, bytes_moved=moved, bytes_per_second=moved / (t["median_ms"] * 1e-3),
                fraction_of_hbm_rate=moved / HBM_BYTES_PER_SECOND / (t["median_ms"] * 1e-3),
                rate_is="a cache rate: the image fits the 256 MiB last-level cache" if in_cache else "an HBM rate: the image exceeds the 256 MiB last-level cache",
                tables_bit_equal=bool(all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got, want))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="2048x1024,8192x4096")
    args = ap.parse_args()
    out = dict(reps=args.reps, warmup=1, hbm_bytes_per_second=HBM_BYTES_PER_SECOND)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        out[size] = dict(rgb=measure(abi.MODE_RGB, w, h, args.reps), spectral=measure(abi.MODE_SPECTRAL, w, h, args.reps))
        print("# %s done" % size, file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
