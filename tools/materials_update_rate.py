#!/usr/bin/env python3
"""What a change of the emitting set costs through slrhip_set_materials, next to slrhip_upload_scene of the same scene on the same
context: lattice_grid(400) (320 011 triangles, re-assigned to eight matte materials as i % 8 next to the uploaded light), host and
device builder.  Every timed set_materials call switches material 0 (40 000 triangles) between emitting and not, so each one rebuilds
the light list on the device.  Wall-clock around the call and a device synchronise, the median of 10 runs after 2 warm-up runs (the
first call also allocates the rebuild's scratch); min and max are printed with it.

    python tools/materials_update_rate.py [--out profiles/materials_update_rate.txt]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import abi, scenes  # noqa: E402
from slr_amd.binding import Context  # noqa: E402

RUNS, WARMUP = 10, 2


def classes(sc):
    light = int(np.nonzero(sc.materials["emittance"] >= 0)[0][0])
    mats = np.zeros(9, abi.material_dtype)
    mats[:] = sc.materials[1 - light]
    mats[8] = sc.materials[light]
    tris = sc.triangles.copy()
    was_light = tris["material"] == light
    tris["material"] = np.arange(len(tris)) % 8
    tris["material"][was_light] = 8
    return mats, tris, int(sc.materials["emittance"][light])


def scene_with(sc, mats, tris):
    return abi.Scene(sc.vertices, tris, mats, sc.spectra, sc.spectrum_data, sc.camera, None, sc.name + "_classes")


def timed(ctx, call):
    ctx.synchronize()
    t0 = time.perf_counter()
    call()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "materials_update_rate.txt"))
    args = ap.parse_args()
    base = scenes.lattice_grid(400)
    mats, tris, spectrum = classes(base)
    off = scene_with(base, mats, tris)
    lit = mats.copy()
    lit["emittance"][0] = spectrum
    on = scene_with(base, lit, tris)
    lines = ["materials_update_rate: %s, %d triangles, %d runs after %d warm-up runs, milliseconds (median  min .. max)"
             % (base.name, len(tris), RUNS, WARMUP)]
    for label, flags in (("host builder", 0), ("device builder", abi.FLAG_BVH_DEVICE_BUILD)):
        ctx = Context(device=0, flags=flags | abi.FLAG_DYNAMIC_GEOMETRY)
        try:
            ctx.upload_scene(off)
            builder = ctx.debug_tree(summary_only=True)["builder_name"]
            update, upload = [], []
            for k in range(WARMUP + RUNS):
                update.append(timed(ctx, lambda: ctx.set_materials(on if k % 2 == 0 else off)))
            info = ctx.debug_materials()
            assert info["rebuilt"]
            for k in range(WARMUP + RUNS):
                upload.append(timed(ctx, lambda: ctx.upload_scene(on if k % 2 == 0 else off)))
            update, upload = update[WARMUP:], upload[WARMUP:]
            mu, mp = statistics.median(update), statistics.median(upload)
            lines.append("%-15s (%s): set_materials %8.3f  %8.3f .. %8.3f   upload_scene %9.3f  %9.3f .. %9.3f   ratio %.1f x   launches %d   lights %d"
                         % (label, builder, mu, min(update), max(update), mp, min(upload), max(upload), mp / mu, info["launches"], info["lights"]))
        finally:
            ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
