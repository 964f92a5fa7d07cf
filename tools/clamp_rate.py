"""Cost of the sample clamp (slrhip_clamp_begin) in the fold kernel: k_fold per 64-pass window at 1280x720 on the Cornell box,
RGB and spectral, for the variants none (no clamp), clamp and clamp_stats (clamp and statistics).  The fold is not one of the
kernels slrhip_profile times, so its durations come from a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR/<label> -- python tools/clamp_rate.py run --mode rgb --variant clamp
    python tools/clamp_rate.py summarise --dir DIR --out profiles/r12_clamp_rate.json

`run` renders --windows windows of 64 passes (one slrhip_render call each: one fold launch per call); `summarise` takes, per
<label> directory under DIR, the median duration of the k_fold dispatches after the first --skip (warm-up) ones, and relates it to
the bytes the kernel moves: the window (16 B per element and pass) plus the sensor's two arrays read and written (64 B per
element) plus the 16-byte records of each kind per pixel, read and written.  A build from before the clamp (SLRHIP_LIBRARY) runs
the variant none only; name its label accordingly."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT, WINDOW = 1280, 720, 64
HBM_BYTES_PER_SECOND = 8e12


def run(args):
    import torch  # noqa: F401  before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime
    from slr_amd import Context, abi, scenes
    sc = scenes.cornell_box_spheres(WIDTH / HEIGHT, 48, 24, "matte")
    st = abi.RenderSettings(WIDTH, HEIGHT, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    ctx = Context(mode=abi.MODE_SPECTRAL if args.mode == "spectral" else abi.MODE_RGB)
    ctx.upload_scene(sc)
    ctx.render_begin(st)
    if args.variant == "clamp_stats":
        ctx.statistics_begin()
    if args.variant != "none":
        ctx.clamp_begin(args.limit, True)
    for w in range(args.windows):
        ctx.render(w * WINDOW, WINDOW)
    ctx.synchronize()
    out = {"mode": args.mode, "variant": args.variant, "windows": args.windows}
    if args.variant != "none":
        out["summary"] = ctx.clamp_summary()
    ctx.close()
    print(json.dumps(out))


def bytes_moved(mode, label):
    elems = WIDTH * HEIGHT * (4 if mode == "spectral" else 1)
    records = (1 if "clamp" in label else 0) + (1 if "stats" in label else 0)
    return elems * 16 * WINDOW + elems * 16 * 4 + WIDTH * HEIGHT * 16 * 2 * records


def summarise(args):
    out = {"width": WIDTH, "height": HEIGHT, "passes_per_window": WINDOW, "hbm_bytes_per_second": HBM_BYTES_PER_SECOND, "skip": args.skip, "runs": {}}
    for label in sorted(os.listdir(args.dir)):
        files = glob.glob(os.path.join(args.dir, label, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            continue
        per_kernel = {}
        for path in files:
            with open(path, newline="") as f:
                rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
            for r in rows:
                if "k_fold" in r["Kernel_Name"]:
                    per_kernel.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
        mode = "spectral" if "spectral" in label else "rgb"
        for kernel, us in per_kernel.items():
            timed = us[args.skip:]
            med = float(np.median(timed))
            moved = bytes_moved(mode, label)
            out["runs"].setdefault(label, []).append(
                {"kernel": kernel, "dispatches_timed": len(timed), "median_us": round(med, 2), "min_us": round(min(timed), 2), "max_us": round(max(timed), 2),
                 "bytes_moved": moved, "fraction_of_hbm_rate": round(moved / (med * 1e-6) / HBM_BYTES_PER_SECOND, 4)})
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="command", required=True)
    r = sub.add_parser("run")
    r.add_argument("--mode", choices=["rgb", "spectral"], default="rgb")
    r.add_argument("--variant", choices=["none", "clamp", "clamp_stats"], default="none")
    r.add_argument("--windows", type=int, default=24)
    r.add_argument("--limit", type=float, default=0.05, help="in sample luminance; the scene's samples reach about 0.06 at 64 x 48")
    s = sub.add_parser("summarise")
    s.add_argument("--dir", required=True)
    s.add_argument("--out")
    s.add_argument("--skip", type=int, default=4)
    args = ap.parse_args()
    (run if args.command == "run" else summarise)(args)


if __name__ == "__main__":
    main()
