"""Ray queries on device memory (slrhip_intersect_rays / slrhip_test_visibility / slrhip_query_status): the render's
wave-specialised traversal fed from a caller's ray array.  CPU: the struct layouts and the argument checks.  GPU (MI355X): hit for
hit against the compiled reference's goldens, against slrhip_trace_rays (the 64-ray batch kernel, an independent traversal) on
every tree kind the upload builds, instance ids, the live compiled reference, streams, graph capture and independence from the
render."""
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import zlib

import numpy as np
import pytest

from helpers import GOLDEN, load_golden, scene_from_golden
from slr_amd import abi, binding, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = abi.MISS

PROBE = r"""
#include <stddef.h>
#include <stdio.h>
#include "slrhip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(slrhip_ray), offsetof(slrhip_ray, org), offsetof(slrhip_ray, dist_min),
         offsetof(slrhip_ray, dir), offsetof(slrhip_ray, dist_max), sizeof(slrhip_hit), offsetof(slrhip_hit, triangle),
         offsetof(slrhip_hit, dist), offsetof(slrhip_hit, b0), offsetof(slrhip_hit, b1));
  return 0;
}
"""


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_ray_and_hit_layouts_match_header():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        open(src, "w").write(PROBE)
        exe = os.path.join(d, "probe")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    R, H = abi.ray_dtype, abi.hit_dtype
    want = [R.itemsize, R.fields["org"][1], R.fields["dist_min"][1], R.fields["dir"][1], R.fields["dist_max"][1],
            H.itemsize, H.fields["triangle"][1], H.fields["dist"][1], H.fields["b0"][1], H.fields["b1"][1]]
    assert got == want
    assert [C.sizeof(abi.Ray), abi.Ray.org.offset, abi.Ray.dist_min.offset, abi.Ray.dir.offset, abi.Ray.dist_max.offset] == want[:5]
    assert [C.sizeof(abi.Hit), abi.Hit.triangle.offset, abi.Hit.dist.offset, abi.Hit.b0.offset, abi.Hit.b1.offset] == want[5:]
    assert got[0] == 32 and got[5] == 16


def test_query_entry_points_reject_null_arguments_without_a_gpu():
    lib = binding.load_library()
    bits = C.c_uint32(7)
    assert lib.slrhip_intersect_rays(None, None, 16, None, None, None) == abi_err_invalid()
    assert lib.slrhip_intersect_rays(None, None, 0, None, None, None) == abi_err_invalid()
    assert lib.slrhip_test_visibility(None, None, 16, None, None) == abi_err_invalid()
    assert lib.slrhip_test_visibility(None, None, 0, None, None) == abi_err_invalid()
    assert lib.slrhip_query_status(None, C.byref(bits), None) == abi_err_invalid()
    assert b"null" in lib.slrhip_last_error_string()


def abi_err_invalid():
    return 1      # SLRHIP_ERR_INVALID_ARGUMENT


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------
def query_rows(org, direction, dist_min, dist_max):
    """[n, 8] float32 slrhip_ray rows."""
    n = len(org)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = org, dist_min, direction, dist_max
    return r


def batch_hits(ctx, rows):
    """slrhip_trace_rays (the batch kernel) on the same rays, as [n, 4] slrhip_hit rows."""
    tri, dist, b0, b1 = ctx.trace_rays(rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7])
    out = np.zeros((len(rows), 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = tri.view(np.float32), dist, b0, b1
    return out


def triangles_of(h):
    return np.ascontiguousarray(h[:, 0]).view(np.uint32)


def assert_same_hits(got, want, what):
    """Bit-equal records; the one allowed difference is an equal-distance tie (the same dist on both sides, another triangle),
    at most one per million rays."""
    diff = (got.view(np.uint32) != want.view(np.uint32)).any(axis=1)
    gt, wt = triangles_of(got), triangles_of(want)
    tie = diff & (gt != MISS) & (wt != MISS) & (gt != wt) & (got[:, 1].view(np.uint32) == want[:, 1].view(np.uint32))
    bad = diff & ~tie
    assert not bad.any(), "%s: %d of %d records differ (first at %d)" % (what, bad.sum(), len(got), int(np.argmax(bad)))
    assert tie.sum() <= max(1, len(got) // 1000000), (what, "equal-distance ties", int(tie.sum()))


def instance_ranges(sc):
    return [(int(r["first_triangle"]), int(r["num_triangles"])) for r in sc.instances]


def instance_matrix(rec):
    return np.asarray(rec["local_to_world"], np.float64).reshape(4, 4).T        # stored column-major


def scene_bounds(sc):
    pos = sc.vertices["position"].astype(np.float64)
    tri = sc.triangles["v"]
    mesh = np.zeros(len(tri), bool)
    for first, num in instance_ranges(sc):
        mesh[first:first + num] = True
    pts = [pos[tri[~mesh].reshape(-1)]]
    for rec in sc.instances:
        first, num = int(rec["first_triangle"]), int(rec["num_triangles"])
        p = pos[tri[first:first + num].reshape(-1)]
        lo, hi = p.min(0), p.max(0)
        corners = np.array([[x, y, z, 1.0] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
        pts.append((corners @ instance_matrix(rec).T)[:, :3])
    pts = np.concatenate(pts)
    return pts.min(0), pts.max(0)


def seeded_rays(sc, n, seed):
    """n rays: 3/8 camera rays in image order (coherent), 3/8 random rays from points inside the scene's box, 1/4 of those with a
    short dist_max."""
    rng = np.random.default_rng(seed)
    lo, hi = scene_bounds(sc)
    diag = float(np.linalg.norm(hi - lo))
    n_cam = 3 * n // 8
    side = int(np.sqrt(n_cam))
    n_cam = side * side
    cam = np.array(sc.camera.local_to_world[12:15], np.float64)
    axes = np.argsort(hi - lo)[::-1]
    u, v = np.meshgrid((np.arange(side) + 0.5) / side, (np.arange(side) + 0.5) / side, indexing="xy")
    tgt = np.tile((lo + hi) / 2, (n_cam, 1))
    tgt[:, axes[0]] = lo[axes[0]] + (hi - lo)[axes[0]] * u.reshape(-1)
    tgt[:, axes[1]] = lo[axes[1]] + (hi - lo)[axes[1]] * v.reshape(-1)
    d = tgt - cam
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rows = [query_rows(np.tile(cam, (n_cam, 1)), d, 0.0, np.inf)]
    n_rest = n - n_cam
    o = lo + (hi - lo) * rng.uniform(0.02, 0.98, (n_rest, 3))
    d = rng.normal(size=(n_rest, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dmax = np.full(n_rest, np.inf)
    short = np.arange(n_rest) >= n_rest - n // 4
    dmax[short] = rng.uniform(0.0, 0.05, short.sum()) * diag
    dmin = np.where(rng.uniform(size=n_rest) < 0.5, 0.0, 1e-4 * diag)
    rows.append(query_rows(o, d, dmin, dmax))
    return np.concatenate(rows).astype(np.float32)


def golden_ray_names():
    out = []
    for p in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        with np.load(p) as g:
            if "rays" in g.files and "hits" in g.files:
                out.append(os.path.basename(p)[:-4])
    return out


def golden_scene(g):
    if "generator" in g.files:
        from test_oracle_golden import procedural_scene
        return procedural_scene(g)
    return scene_from_golden(g)


def golden_rows(g):
    r = g["rays"]
    return query_rows(r["org"], r["dir"], r["dist_min"], r["dist_max"])


# ---- GPU: against the compiled reference's goldens ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", golden_ray_names())
def test_golden_hits_bit_equal_and_visibility(name):
    g = load_golden(name)
    mode = abi.MODE_SPECTRAL if name.startswith("spectral") else abi.MODE_RGB
    ctx = binding.Context(mode=mode)
    try:
        sc = golden_scene(g)
        ctx.upload_scene(sc)
        if name == "rgb_grid400":
            assert ctx.counters().bvh_nodes >= 65536          # the quantized tree
        rows = golden_rows(g)
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        vis = ctx.test_visibility(rows)
    finally:
        ctx.close()
    want = g["hits"]
    tri = triangles_of(hits)
    assert (tri == want["triangle"]).all(), (name, int((tri != want["triangle"]).sum()))
    hit = want["triangle"] != MISS
    assert hit.any()
    for col, k in ((1, "dist"), (2, "b0"), (3, "b1")):
        assert (hits[hit, col].view(np.uint32) == want[k][hit].view(np.uint32)).all(), (name, k)
    assert (vis == (want["triangle"] == MISS)).all(), name
    assert (inst[~hit] == -1).all()
    if len(sc.instances) == 0:
        assert (inst == -1).all()


# ---- GPU: against slrhip_trace_rays on every tree kind -------------------------------------------------------------------------
CROSS = {
    "cornell_float": (lambda: scenes.cornell_box_spheres(4.0 / 3.0, 32, 16, "glass"), 0),
    "grid_quantized": (lambda: scenes.displaced_grid(400, 16.0 / 9.0), 0),
    "cornell_device_build": (lambda: scenes.cornell_box_spheres(4.0 / 3.0, 32, 16, "glass"), abi.FLAG_BVH_DEVICE_BUILD),
    "grid_device_build": (lambda: scenes.displaced_grid(400, 16.0 / 9.0), abi.FLAG_BVH_DEVICE_BUILD),
    "cornell_spatial_splits": (lambda: scenes.cornell_box_spheres(4.0 / 3.0, 32, 16, "glass"), abi.FLAG_BVH_SPATIAL_SPLITS),
    "cornell_instanced": (lambda: scenes.cornell_instanced(4.0 / 3.0, 16, 8, copies=24), 0),
    "instanced_grid": (lambda: scenes.instanced_grid(tiles_x=10, tiles_z=20, cells=32), 0),
    "textured_alpha": (lambda: scenes.cornell_textured(4.0 / 3.0, 20, 10), 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CROSS))
def test_queries_match_trace_rays_on_every_tree(name):
    make, flags = CROSS[name]
    sc = make()
    rows = seeded_rays(sc, 1 << 20, seed=zlib.crc32(name.encode()))
    ctx = binding.Context(flags=flags)
    try:
        ctx.upload_scene(sc)
        if name.startswith("grid"):
            assert ctx.counters().bvh_nodes >= 65536
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        vis = ctx.test_visibility(rows)
        want = batch_hits(ctx, rows)
    finally:
        ctx.close()
    assert_same_hits(hits, want, name)
    tri = triangles_of(hits)
    assert 0.05 < (tri != MISS).mean() < 0.999, (name, (tri != MISS).mean())
    # visibility: no hit in [dist_min, dist_max] <=> no closest hit
    assert (vis == (tri == MISS)).all(), (name, int((vis != (tri == MISS)).sum()))
    check_instances(sc, rows, hits, inst, name)


def check_instances(sc, rows, hits, inst, what):
    """An instanced hit lies on the reported instance's transformed triangle: org + dir * dist equals the world triangle's point
    at (b0, b1) within 1e-4 of the scene's diagonal, and the triangle is inside that instance's mesh; loose triangles report -1."""
    tri = triangles_of(hits)
    hit = tri != MISS
    assert (inst[~hit] == -1).all(), what
    ranges = instance_ranges(sc)
    if not ranges:
        assert (inst == -1).all(), what
        return
    mesh = np.zeros(len(sc.triangles), bool)
    for first, num in ranges:
        mesh[first:first + num] = True
    assert ((inst >= 0) == (hit & mesh[np.where(hit, tri, 0)])).all(), what
    k = np.nonzero(inst >= 0)[0]
    assert len(k) > 1000, (what, len(k))
    k = k[:: max(1, len(k) // 20000)]
    lo, hi = scene_bounds(sc)
    tol = 1e-4 * float(np.linalg.norm(hi - lo))
    pos = sc.vertices["position"].astype(np.float64)
    v = sc.triangles["v"][tri[k]]
    first = np.array([ranges[i][0] for i in inst[k]])
    num = np.array([ranges[i][1] for i in inst[k]])
    assert ((tri[k] >= first) & (tri[k] < first + num)).all(), what
    M = np.stack([instance_matrix(sc.instances[i]) for i in inst[k]])
    world = [np.einsum("kij,kj->ki", M[:, :3, :3], pos[v[:, c]]) + M[:, :3, 3] for c in range(3)]
    b0, b1 = hits[k, 2].astype(np.float64), hits[k, 3].astype(np.float64)
    p_bary = b0[:, None] * world[0] + b1[:, None] * world[1] + (1.0 - b0 - b1)[:, None] * world[2]
    p_ray = rows[k, 0:3].astype(np.float64) + rows[k, 4:7].astype(np.float64) * hits[k, 1:2].astype(np.float64)
    err = np.linalg.norm(p_bary - p_ray, axis=1)
    assert err.max() <= tol, (what, float(err.max()), tol)


# ---- GPU: the live compiled reference ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [abi.MODE_RGB, abi.MODE_SPECTRAL])
def test_instanced_scene_against_live_reference(request, mode):
    from oracle import binding as ob
    ref = request.getfixturevalue("ref_rgb" if mode == abi.MODE_RGB else "ref_spectral")
    sc = scenes.cornell_instanced(4.0 / 3.0, 16, 8, copies=24)
    rows = seeded_rays(sc, 1 << 16, seed=77)
    rays = np.zeros(len(rows), ob.ray_dtype)
    rays["org"], rays["dir"], rays["dist_min"], rays["dist_max"] = rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7]
    want = ref.scene(sc).trace(rays)
    ctx = binding.Context(mode=mode)
    try:
        ctx.upload_scene(sc)
        hits = ctx.intersect_rays(rows)
    finally:
        ctx.close()
    tri = triangles_of(hits)
    assert (tri == want["triangle"]).all(), int((tri != want["triangle"]).sum())
    assert (tri != MISS).sum() > 10000


# ---- GPU: device tensors, streams, graph capture, independence from the render ------------------------------------------------
# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process.  The checks on torch tensors
# therefore run in a fresh child process that imports torch BEFORE libslrhip.so is loaded, so that the library binds to torch's
# copy (bench.py's order); this test process has the device open through the system's copy.
def in_child(check):
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_ray_queries as T\nT.%s()\nprint('CHILD_OK')\n"
           % (ROOT, os.path.join(ROOT, "tests"), check))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (check, p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.gpu
def test_device_tensors_on_a_side_stream_match_the_numpy_path():
    in_child("_side_stream_check")


@pytest.mark.gpu
def test_graph_captured_query_replays_on_new_rays():
    in_child("_graph_check")


@pytest.mark.gpu
def test_loud_failures():
    """No scene, misaligned rays, bad pointers, n >= 2^31 fail at the call; n == 0 is a no-op (torch tensors, in a child process);
    and the numpy path here."""
    in_child("_loud_failures_check")
    ctx = binding.Context()
    try:
        rows = np.zeros((64, 8), np.float32)
        with pytest.raises(binding.SlrHipError, match="no scene"):
            ctx.intersect_rays(rows)
        ctx.upload_scene(scenes.tiny_box())
        assert ctx.intersect_rays(rows[:0]).shape == (0, 4) and ctx.test_visibility(rows[:0]).shape == (0,)
    finally:
        ctx.close()


def _side_stream_check():
    import torch
    sc = scenes.cornell_instanced(4.0 / 3.0, 16, 8, copies=24)
    rows = seeded_rays(sc, 1 << 18, seed=5)
    ctx = binding.Context()
    try:
        ctx.upload_scene(sc)
        want_hits, want_inst = ctx.intersect_rays(rows, want_instances=True)
        want_vis = ctx.test_visibility(rows)
        s = torch.cuda.Stream()
        r = torch.from_numpy(rows).cuda()
        s.wait_stream(torch.cuda.current_stream())
        hits, inst = ctx.intersect_rays(r, stream=s, want_instances=True)
        vis = ctx.test_visibility(r, stream=s)
        assert hits.is_cuda and hits.shape == (len(rows), 4) and inst.dtype == torch.int32 and vis.dtype == torch.int32
        assert ctx.query_status(s) == 0
        s.synchronize()
        assert (hits.cpu().numpy().view(np.uint32) == want_hits.view(np.uint32)).all()
        assert (inst.cpu().numpy() == want_inst).all()
        assert (vis.cpu().numpy() == want_vis).all()
    finally:
        ctx.close()


def _graph_check():
    import torch
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 32, 16, "glass")
    a, b = seeded_rays(sc, 1 << 16, seed=1), seeded_rays(sc, 1 << 16, seed=2)
    ctx = binding.Context()
    try:
        ctx.upload_scene(sc)
        want_b = ctx.intersect_rays(b)
        want_vis_b = ctx.test_visibility(b)
        static = torch.from_numpy(a).cuda()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                       # warm-up outside the capture
            ctx.intersect_rays(static)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            hits = ctx.intersect_rays(static)
            vis = ctx.test_visibility(static)
        static.copy_(torch.from_numpy(b))
        graph.replay()
        torch.cuda.synchronize()
        assert ctx.query_status() == 0
        assert (hits.cpu().numpy().view(np.uint32) == want_b.view(np.uint32)).all()
        assert (vis.cpu().numpy() == want_vis_b).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_query_between_render_calls_leaves_the_frame_bit_identical():
    from oracle import binding as ob
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "glass")
    st = ob.settings(96, 72, seed=3)
    rows = seeded_rays(sc, 1 << 18, seed=9)
    ctx = binding.Context(stripes=1)
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        ctx.render(0, 16)
        whole = ctx.read_framebuffer()
        ctx.render_begin(st)
        ctx.render(0, 6)
        hits = ctx.intersect_rays(rows)
        vis = ctx.test_visibility(rows)
        ctx.render(6, 10)
        split = ctx.read_framebuffer()
    finally:
        ctx.close()
    assert (triangles_of(hits) != MISS).any() and vis.any()
    assert (split.view(np.uint32) == whole.view(np.uint32)).all()


def _loud_failures_check():
    import torch
    ctx = binding.Context()
    try:
        r = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
        with pytest.raises(binding.SlrHipError, match="no scene"):
            ctx.intersect_rays(r)
        with pytest.raises(binding.SlrHipError, match="no scene"):
            ctx.test_visibility(r)
        ctx.upload_scene(scenes.tiny_box())
        flat = torch.zeros(64 * 8 + 1, dtype=torch.float32, device="cuda")
        skewed = flat[1:].view(64, 8)
        assert skewed.data_ptr() % 16 != 0
        with pytest.raises(binding.SlrHipError, match="misaligned"):
            ctx.intersect_rays(skewed)
        with pytest.raises(binding.SlrHipError, match="misaligned"):
            ctx.test_visibility(skewed)
        lib, h = ctx.lib, ctx.handle
        hits = torch.empty((64, 4), dtype=torch.float32, device="cuda")
        assert lib.slrhip_intersect_rays(h, r.data_ptr(), 1 << 31, hits.data_ptr(), None, None) == 1
        assert lib.slrhip_intersect_rays(h, None, 64, hits.data_ptr(), None, None) == 1
        assert lib.slrhip_intersect_rays(h, r.data_ptr(), 64, None, None, None) == 1
        assert lib.slrhip_test_visibility(h, r.data_ptr(), 64, None, None) == 1
        # n == 0 is a no-op (an empty tensor may have a null data pointer)
        empty = torch.zeros((0, 8), dtype=torch.float32, device="cuda")
        h0, i0 = ctx.intersect_rays(empty, want_instances=True)
        assert h0.shape == (0, 4) and i0.shape == (0,) and ctx.test_visibility(empty).shape == (0,)
        assert lib.slrhip_intersect_rays(h, None, 0, None, None, None) == 0
        assert ctx.query_status() == 0
    finally:
        ctx.close()
