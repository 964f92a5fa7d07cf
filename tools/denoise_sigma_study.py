"""How the default sigma_distance of the denoiser (abi.DENOISE_SIGMA_DISTANCE) was picked, on scenes.cornell_box_spheres at 8 spp:
the relative change of the camera distance between adjacent pixels of one surface (n.n' > 0.99) and of different surfaces
(n.n' < 0.5), as percentiles, at 64x48 and 1280x720; and, at 64x48, the RMS luminance difference to 1024 spp of the raw mean frame
and of the filtered one for a range of sigma_distance, without the normals, without the variance, and for 1 .. 6 iterations.
Prints one JSON document (profiles/r09_denoise_sigma_distance.json).  Uses the helpers of tests/test_denoise.py."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import test_denoise as t  # noqa: E402
from oracle import binding as ob  # noqa: E402
from slr_amd import Context, abi, scenes  # noqa: E402

out = {}
for (w, h, a, b) in ((64, 48, 16, 8), (1280, 720, 48, 24)):
    for material in ("matte", "glass"):
        c = Context()
        c.upload_scene(scenes.cornell_box_spheres(w / h, a, b, material))
        st = ob.settings(w, h, seed=5)
        inp = t.render_with_guides(c, st, 8)
        cov = inp["coverage"]
        hit = cov > 0
        with np.errstate(all="ignore"):
            z = np.where(hit, inp["distance"] / cov, np.nan)
            n = inp["normal"] / np.linalg.norm(inp["normal"], axis=2, keepdims=True)
        rows = {}
        for name, (zp, zq, np_, nq) in {"dx": (z[:, :-1], z[:, 1:], n[:, :-1], n[:, 1:]), "dy": (z[:-1], z[1:], n[:-1], n[1:])}.items():
            with np.errstate(all="ignore"):
                r = np.abs(zp - zq) / zp
                dot = (np_ * nq).sum(axis=2)
            ok = np.isfinite(r) & np.isfinite(dot)
            same, other = ok & (dot > 0.99), ok & (dot < 0.5)
            rows[name] = dict(same_surface=[float(np.percentile(r[same], q)) for q in (50, 90, 99, 99.9)],
                              other_surface=[float(np.percentile(r[other], q)) for q in (1, 10, 50)] if other.any() else None,
                              pairs=int(same.sum()), pairs_other=int(other.sum()))
        key = "%dx%d %s" % (w, h, material)
        out[key] = dict(relative_change_per_pixel=rows, hit_fraction=float(hit.mean()))
        if (w, h) == (64, 48):
            c.render_begin(st)
            c.render(0, 1024)
            conv = t.luminance(c.read_framebuffer()).astype(np.float64) / 1024.0

            def rms(f):
                return float(np.sqrt(np.mean((t.luminance(f).astype(np.float64) - conv) ** 2)))
            q = {"raw": rms(inp["color"])}
            for sd in (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0):
                q["sigma_distance %g" % sd] = rms(c.denoise(sigma_distance=sd, **inp))
            q["no normals, sigma 0.1"] = rms(c.denoise(**dict(inp, normal=None)))
            q["no variance"] = rms(c.denoise(**dict(inp, variance=None)))
            for it in (1, 2, 3, 4, 6):
                q["iterations %d" % it] = rms(c.denoise(iterations=it, **inp))
            out[key]["rms_vs_1024spp"] = q
        c.close()
print(json.dumps(out, indent=1))
