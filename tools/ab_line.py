#!/usr/bin/env python
"""One line of an A/B table (tools/ab_libs.sh) from bench.py's JSON line on stdin and the frame it dumped.

    python bench.py … --dump-outputs DIR | python tools/ab_line.py NAME DIR STEPS"""
import glob
import hashlib
import json
import sys

name, dump, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
d = json.loads(sys.stdin.read().strip().splitlines()[-1])
k, c = d.get("kernels", {}), d.get("counters", {})
sha = hashlib.sha256()
for path in sorted(glob.glob(dump + "/*.npy")):      # framebuffer.npy, or bench.py's fixed pixel sample of a frame over 64 MB
    sha.update(open(path, "rb").read())
print("%-9s ms/frame %8.2f  kernels ms/frame %s launches/frame %s  samples %d ext %d shadow %d  frame sha256 %s" % (
    name, d["ms_per_step"], {n: round(k[n]["ms_total"] / steps, 2) for n in k}, {n: k[n]["launches"] // steps for n in k},
    c.get("samples", -1), c.get("extension_rays", -1), c.get("shadow_rays", -1), sha.hexdigest()), flush=True)
