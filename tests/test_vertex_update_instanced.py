"""Moving the vertices of a scene WITH instances without a scene upload (slrhip_set_vertices in a context created with
SLRHIP_FLAG_DYNAMIC_GEOMETRY | SLRHIP_FLAG_DYNAMIC_INSTANCED).

CPU: the flag, the new exports and the version; every refusal through the new check twin with its code and message; the old twin's answers.

GPU: after every move the two-level tree passes tree_checks.check_tree against the moved scene (leaf_box, inner_box and instance_box are
equalities) with the shape of both levels untouched; mesh boxes, instance boxes and every record equal the fresh upload's; the context
renders, answers queries (with instance ids) and fills feature and albedo buffers bit for bit as a fresh context without flags that
uploaded the moved scene; the merged mesh-level list names every mesh node once, level by level; and the call works together with
slrhip_rebuild_top_level, slrhip_set_instance_transforms, a render in progress and a captured graph.  The yardstick throughout is the
fresh upload and the validator; no tolerance is involved.  Node planes compare as float values (the sign of a zero may differ from the
host's fmin), everything else by bytes."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_instance_update as T
import test_vertex_update as V
from helpers import assert_bit_equal, ray_rows
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, SlrHipError
from test_top_level_rebuild import assert_same_nodes
from tree_checks import check_tree

ROOT = V.ROOT
F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
SIZE, SPP = V.SIZE, V.SPP
DYNAMIC, INSTANCED = abi.FLAG_DYNAMIC_GEOMETRY, abi.FLAG_DYNAMIC_INSTANCED
BOTH = DYNAMIC | INSTANCED
RGB, SPECTRAL = abi.MODE_RGB, abi.MODE_SPECTRAL
same_bytes, kahan = V.same_bytes, V.kahan

# name -> (a lattice scene: exact coordinates, the reach of the seeded perturbation in the scene's own units)
CASES = {"lattice": (True, 0.5), "cornell": (False, 0.02), "grid": (False, 0.2), "patch": (False, 1.0 / 64.0), "nine": (True, 0.5)}
NAMES = list(CASES)
MOVES = ["shift", "perturb", "partial", "loose", "one_mesh", "collapse"]


def nine_meshes():
    """Nine distinct meshes of different depths next to a loose emitter: the lattice terrains of n = 1 .. 8 (13 .. 139 triangles) and a
    single triangle, whose tree is one node with one valid child; every second one placed twice.  Exact matrices (integer translations)."""
    b = scenes.SceneBuilder()
    grey = b.matte(b.spectrum_grey(0.5))
    light = b.matte(b.spectrum_grey(0.8), emittance=b.spectrum_d65(1.0, scenes.D65_RGB))
    b.add_quad([(-8, 14, -8), (28, 14, -8), (28, 14, 28), (-8, 14, 28)], (0, -1, 0), (1, 0, 0), light)
    ranges = []
    for n in range(1, 9):
        part = scenes.lattice_terrain(n)
        first = b.num_triangles()
        b.add_mesh(part.vertices["position"], part.vertices["normal"], part.vertices["tangent"], part.vertices["texcoord"], part.triangles["v"], grey)
        ranges.append((first, b.num_triangles() - first))
    first = b.num_triangles()
    b.add_mesh([(0, 0, 0), (3, 1, 0), (0, 2, 3)], [(0, 1, 0)] * 3, [(1, 0, 0)] * 3, [(0, 0), (1, 0), (0, 1)], [(0, 1, 2)], grey)
    ranges.append((first, 1))
    for k, (first, count) in enumerate(ranges):
        m = np.eye(4)
        m[:3, 3] = (-6 + 10 * (k % 3), 0, -4 + 10 * (k // 3))
        b.add_instance(first, count, m)
        if k % 2 == 0:
            m[:3, 3] += (1, 7, 2)
            b.add_instance(first, count, m)
    return b.build(scenes.lattice_instanced().camera, name="nine_meshes")


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name in T.SCENES:
        return T.base_scene(name)
    if name == "patch":
        return scenes.instanced_grid(tiles_x=2, tiles_z=2, cells=64, aspect=1.0)
    assert name == "nine"
    return nine_meshes()


def with_scene(sc, vertices=None, rec=None):
    """The scene with another vertex array and / or other instance matrices: what a fresh context uploads."""
    inst = sc.instances.copy()
    if rec is not None:
        inst["local_to_world"], inst["world_to_local"] = rec[:, :16], rec[:, 16:]
    assert sc.env is None and len(sc.textures) == 0
    return abi.Scene(sc.vertices if vertices is None else vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, None,
                     sc.name + "_moved", instances=inst)


@functools.lru_cache(maxsize=None)
def vertex_sets(name):
    """(vertices of loose triangles, [vertices of each distinct mesh in the order of its first placement])."""
    sc = base_scene(name)
    instanced = np.zeros(len(sc.triangles), bool)
    meshes, seen = [], set()
    for rec in sc.instances:
        lo, n = int(rec["first_triangle"]), int(rec["num_triangles"])
        instanced[lo:lo + n] = True
        if lo not in seen:
            seen.add(lo)
            meshes.append(np.unique(sc.triangles["v"][lo:lo + n]))
    return np.unique(sc.triangles["v"][~instanced]), meshes


def perturbed(name, seed=5):
    sc = base_scene(name)
    rng = np.random.default_rng(seed)
    reach = CASES[name][1]
    v = sc.vertices.copy()
    v["position"] = (v["position"].astype(np.float64) + rng.uniform(-reach, reach, v["position"].shape)).astype(F)
    v["texcoord"] = (v["texcoord"] + rng.uniform(-0.05, 0.05, v["texcoord"].shape)).astype(F)
    return v


def moved(name, move):
    """(the full vertex array after the move, first, count): the update call is given rows first .. first + count."""
    sc = base_scene(name)
    n = len(sc.vertices)
    loose, meshes = vertex_sets(name)
    v = sc.vertices.copy()
    if move == "identity":
        return v, 0, n
    if move == "shift":
        assert CASES[name][0]
        v["position"][:, 1] += (np.random.default_rng(6).integers(-2, 3, n) * 0.25).astype(F)
        return v, 0, n
    if move == "perturb":
        return perturbed(name), 0, n
    if move == "partial":
        first, count = n // 3, max(1, n // 3)
        v[first:first + count] = perturbed(name)[first:first + count]
        return v, first, count
    chosen = {"loose": loose, "one_mesh": meshes[-1], "collapse": meshes[len(meshes) // 2]}[move]
    if move == "collapse":
        v["position"][chosen] = v["position"][chosen[0]]          # one whole mesh onto a point: its tree, its box and its instances' boxes degenerate
    else:
        v[chosen] = perturbed(name)[chosen]
    first, last = int(chosen.min()), int(chosen.max())
    return v, first, last - first + 1


def moves_of(name):
    return [m for m in MOVES if m != "shift" or CASES[name][0]]


@functools.lru_cache(maxsize=None)
def query_rays(name, n=2048, seed=3):
    """Seeded rays towards points of the scene as placed: loose vertices and every instance's vertices in world space."""
    sc = base_scene(name)
    loose, _ = vertex_sets(name)
    pts = [sc.vertices["position"][loose].astype(np.float64)]
    for rec in sc.instances:
        lo, cnt = int(rec["first_triangle"]), int(rec["num_triangles"])
        p = sc.vertices["position"][np.unique(sc.triangles["v"][lo:lo + cnt])].astype(np.float64)
        m = rec["local_to_world"].astype(np.float64).reshape(4, 4).T
        pts.append(p @ m[:3, :3].T + m[:3, 3])
    pts = np.concatenate(pts)
    rng = np.random.default_rng(seed)
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    pad = 0.25 * (hi - lo) + 0.5
    org = rng.uniform(lo - pad, hi + pad, (n, 3))
    d = pts[rng.integers(0, len(pts), n)] + rng.uniform(-0.25, 0.25, (n, 3)) * CASES[name][1] - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return ray_rows(org, d, 0.0, 1.0e30)


def settings(seed=9):
    return ob.settings(SIZE, SIZE, seed=seed)


def everything(ctx, rays, seed=9):
    """What a caller can get out of a context for its scene: the frame and its counters, closest hits with instance ids and visibility of
    seeded rays, every feature buffer, the albedo."""
    ctx.render_begin(settings(seed))
    ctx.render(0, SPP)
    k = ctx.counters()
    out = dict(frame=ctx.read_framebuffer(), counters=np.array([k.samples, k.extension_rays, k.shadow_rays], np.uint64))
    out["hits"], out["hit_instances"] = ctx.intersect_rays(rays, want_instances=True)
    shadow = rays.copy()
    hit = np.isfinite(out["hits"][:, 1]) & (out["hits"].view(np.uint32)[:, 0] != abi.MISS)
    shadow[:, 7] = np.where(hit, out["hits"][:, 1] * F(2.0), F(10.0))
    shadow[::2, 7] = np.where(hit[::2], out["hits"][::2, 1] * F(0.5), F(10.0))
    out["visible"] = ctx.test_visibility(shadow)
    ctx.render_begin(settings(seed))
    ctx.render_features(abi.FEATURE_ALL, 2)
    for ch in sorted(abi.FEATURE_CHANNELS):
        out["feature_" + abi.FEATURE_CHANNELS[ch][0]] = ctx.features(ch)
    ctx.render_albedo(2)
    out["albedo"], passes = ctx.albedo()
    assert passes == 2
    return out


assert_same = V.assert_same


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(mode=RGB, which=0, flags=0):
        key = (mode, which, flags)
        if key not in made:
            made[key] = Context(device=0, mode=mode, flags=flags)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def snapshot(ctx):
    return dict(tree=ctx.debug_tree(), geo=ctx.debug_geometry(), top=ctx.debug_top_level())


def assert_same_snapshot(got, want, what):
    """Node planes and boxes as float values, everything else by bytes."""
    t, w = got["tree"], want["tree"]
    for k in ("builder", "num_nodes", "depth", "leaf_references", "num_triangles", "quantized", "num_instances", "top_nodes"):
        assert t[k] == w[k], (what, k)
    for plane in ("lo", "hi"):
        assert np.array_equal(t["nodes"][plane], w["nodes"][plane]), "%s: node planes %s differ" % (what, plane)
    same_bytes(t["nodes"]["child"], w["nodes"]["child"], what + ": child words")
    same_bytes(t["nodes"]["pad"], w["nodes"]["pad"], what + ": pad words")
    assert t["nodes_q"] is None and w["nodes_q"] is None
    for k in ("leaf_tris", "shade_tris", "instances"):
        same_bytes(t[k], w[k], "%s: %s" % (what, k))
    for k in ("boxes", "mesh_boxes"):
        assert np.array_equal(got["top"][k], want["top"][k]), "%s: %s differ" % (what, k)
    assert np.array_equal(got["top"]["levels"], want["top"]["levels"])
    g, h = got["geo"], want["geo"]
    assert g["staged"] == h["staged"] and np.array_equal(g["levels"], h["levels"]) and np.array_equal(g["mesh_levels"], h["mesh_levels"])
    for k in ("vertices", "light_tris", "tri_uv", "alpha", "mesh_level_nodes", "mesh_roots"):
        same_bytes(g[k], h[k], "%s: %s" % (what, k))
    if g["staged"]:
        same_bytes(g["light_tris_staged"], h["light_tris_staged"], what + ": staged LightTri")


def check_against_scene(snap, original, sc_moved, what):
    """The validator on the moved scene (exact unions on both levels, instance children = the instances' world boxes), and the shape of
    both levels untouched."""
    t, o = snap["tree"], original["tree"]
    check_tree(t, sc_moved)
    same_bytes(t["nodes"]["child"], o["nodes"]["child"], what + ": child words")
    same_bytes(t["nodes"]["pad"], o["nodes"]["pad"], what + ": pad words")
    for k in ("num_nodes", "depth", "builder", "quantized", "top_nodes", "num_instances"):
        assert t[k] == o[k], (what, k)
    assert t["builder_name"] == "instanced" and not t["quantized"]
    for k in ("tri", "alpha", "pad"):
        same_bytes(t["leaf_tris"][k], o["leaf_tris"][k], "%s: LeafTri.%s" % (what, k))
    same_bytes(t["instances"], o["instances"], what + ": the instances' records")
    g = snap["geo"]
    same_bytes(g["vertices"], sc_moved.vertices, what + ": kept vertices")
    if g["staged"]:
        same_bytes(g["light_tris_staged"], g["light_tris"], what + ": the two copies of the lights")
    # the leaf-box scratch is the triangle's exact box, record by record
    p = sc_moved.vertices["position"][sc_moved.triangles["v"]][t["leaf_tris"]["tri"]]
    assert np.array_equal(g["leaf_boxes"][:, 0, :3], p.min(axis=1)) and np.array_equal(g["leaf_boxes"][:, 1, :3], p.max(axis=1)), what + ": leaf boxes"


def check_against_fresh(snap, fresh_tree, fresh_top, fresh_geo, what):
    """Boxes and records against a fresh upload of the moved scene (its trees have another shape: nodes are not compared)."""
    for k in ("boxes", "mesh_boxes"):
        assert np.array_equal(snap["top"][k], fresh_top[k]), "%s: %s against the fresh upload: %d values differ" % (what, k, (snap["top"][k] != fresh_top[k]).sum())
    assert np.array_equal(snap["tree"]["instance_boxes"], fresh_tree["instance_boxes"])
    V.check_against_fresh(snap, fresh_tree, fresh_geo, what)


def upload(ctx, sc):
    ctx.upload_scene(sc)
    assert ctx.debug_tree(summary_only=True)["builder_name"] == "instanced", sc.name


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_flag_exports_and_version():
    lib = binding.load_library()
    assert hasattr(lib, "slrhip_debug_geometry_update_check2") and "slrhip_debug_geometry_update_check2" in binding.EXPORTS
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    debug = open(os.path.join(ROOT, "include", "slrhip_debug.h")).read()
    flag = re.search(r"#define SLRHIP_FLAG_DYNAMIC_INSTANCED (\d+)u", header)
    assert flag and int(flag.group(1)) == abi.FLAG_DYNAMIC_INSTANCED == 1024
    others = [int(m) for m in re.findall(r"#define SLRHIP_FLAG_\w+\s+(\d+)u", header)]
    assert others.count(1024) == 1 and others.count(512) == 1 and all(v & (v - 1) == 0 for v in others) and len(set(others)) == len(others)
    assert "int slrhip_set_vertices(slrhip_ctx* ctx, const slrhip_vertex* device_src, uint32_t first_vertex, uint32_t count, void* stream);" in header
    assert "int slrhip_geometry_status(slrhip_ctx* ctx, uint32_t* bits, void* stream);" in header
    assert "int slrhip_debug_geometry_update_check2(int32_t have_scene, int32_t dynamic, int32_t instanced_kept, uint32_t tree_builder" in debug
    assert "int slrhip_debug_geometry_update_check(int32_t have_scene, int32_t dynamic, uint32_t tree_builder" in debug
    assert lib.slrhip_version() == 7 and re.search(r"#define SLRHIP_VERSION 7\b", header)


def test_refusals_through_the_new_check_twin():
    lib = binding.load_library()
    ok = dict(have_scene=1, dynamic=1, kept=1, builder=abi.TREE_INSTANCED, num_instances=6, num_vertices=100, src=4096, first=20, count=80)

    def call(**over):
        a = dict(ok, **over)
        rc = lib.slrhip_debug_geometry_update_check2(a["have_scene"], a["dynamic"], a["kept"], a["builder"], a["num_instances"], a["num_vertices"], a["src"],
                                                     a["first"], a["count"])
        return rc, lib.slrhip_last_error_string().decode()
    # accepted: an instanced scene when kept; a flat scene with or without the new flag; the range exactly up to the end; 4-byte alignment
    for over in (dict(), dict(first=0, count=100), dict(first=99, count=1), dict(src=4096 + 4), dict(builder=abi.TREE_HOST_SAH, num_instances=0),
                 dict(builder=abi.TREE_DEVICE, num_instances=0), dict(kept=0, builder=abi.TREE_HOST_SAH, num_instances=0),
                 dict(kept=0, builder=abi.TREE_DEVICE, num_instances=0)):
        assert call(**over)[0] == 0, over
    beyond = "first_vertex + count is beyond the scene's vertices"
    without = "the context was created without SLRHIP_FLAG_DYNAMIC_GEOMETRY"
    for over, code, text in ((dict(have_scene=0), NO_SCENE, "no scene uploaded"),
                             (dict(dynamic=0), UNSUPPORTED, without),
                             (dict(dynamic=0, kept=1, builder=abi.TREE_HOST_SAH, num_instances=0), UNSUPPORTED, without),      # 1024 alone: as no flag
                             (dict(kept=0), UNSUPPORTED, "the scene has instances"),                                          # 512 alone
                             (dict(kept=0, num_instances=0), UNSUPPORTED, "the scene has instances"),
                             (dict(kept=0, builder=abi.TREE_HOST_SAH), UNSUPPORTED, "the scene has instances"),
                             (dict(builder=abi.TREE_HOST_SPATIAL_SPLITS, num_instances=0), UNSUPPORTED, "the tree was built with spatial splits"),
                             (dict(builder=abi.TREE_HOST_SPATIAL_SPLITS), UNSUPPORTED, "the tree was built with spatial splits"),
                             (dict(src=None), INVALID, "null device_src"),
                             (dict(count=0), INVALID, "count must be >= 1"),
                             (dict(src=4096 + 2), INVALID, "misaligned device_src (4 bytes)"),
                             (dict(first=21), INVALID, beyond),
                             (dict(first=100, count=1), INVALID, beyond),
                             (dict(first=1, count=0xFFFFFFFF), INVALID, beyond),
                             (dict(src=None, have_scene=0), INVALID, "null device_src"),        # the argument checks come first, as before
                             (dict(have_scene=0, dynamic=0, kept=0), NO_SCENE, "no scene uploaded")):
        rc, msg = call(**over)
        assert rc == code and msg == "slrhip_set_vertices: " + text, (over, rc, msg)
    with pytest.raises(SlrHipError, match=r"failed \(%d\): slrhip_set_vertices: the scene has instances" % UNSUPPORTED):
        binding.geometry_update_check2(True, True, False, abi.TREE_INSTANCED, 6, 100, 4096, 0, 1)
    binding.geometry_update_check2(True, True, True, abi.TREE_INSTANCED, 6, 100, 4096, 0, 100)


def test_the_old_twin_still_refuses_instances():
    lib = binding.load_library()
    for builder, n in ((abi.TREE_INSTANCED, 6), (abi.TREE_INSTANCED, 0), (abi.TREE_HOST_SAH, 6)):
        assert lib.slrhip_debug_geometry_update_check(1, 1, builder, n, 100, 4096, 0, 100) == UNSUPPORTED
        assert lib.slrhip_last_error_string().decode() == "slrhip_set_vertices: the scene has instances"
    assert lib.slrhip_debug_geometry_update_check(1, 1, abi.TREE_HOST_SAH, 0, 100, 4096, 0, 100) == 0
    # the two twins agree wherever the new input is 0
    for args in ((1, 1, abi.TREE_HOST_SAH, 0, 100, 4096, 0, 100), (0, 1, 0, 0, 100, 4096, 0, 1), (1, 0, 0, 0, 100, 4096, 0, 1), (1, 1, 1, 0, 100, 4096, 0, 1),
                 (1, 1, 3, 6, 100, 4096, 0, 1), (1, 1, 0, 0, 100, None, 0, 1), (1, 1, 0, 0, 100, 4098, 0, 1), (1, 1, 0, 0, 100, 4096, 0, 0),
                 (1, 1, 0, 0, 100, 4096, 100, 1)):
        old = (lib.slrhip_debug_geometry_update_check(*args), lib.slrhip_last_error_string())
        new = (lib.slrhip_debug_geometry_update_check2(args[0], args[1], 0, *args[2:]), lib.slrhip_last_error_string())
        assert old[0] == new[0] and (old[0] == 0 or old[1] == new[1]), args


def test_the_scene_of_nine_meshes_is_what_it_is_for():
    """Host only: nine distinct meshes of different depths, one of them a single node with one valid child."""
    sc = base_scene("nine")
    tree = binding.host_tree(sc)
    check_tree(tree, sc)
    roots = np.unique(tree["instances"]["root"])
    assert len(roots) == 9 and len(sc.instances) == 14
    single = tree["nodes"][roots[-1]]
    assert (single["child"] != abi.INVALID_CHILD).sum() == 1 and (single["child"][0] >> abi.LEAF_COUNT_SHIFT) & 0xF == 1
    sizes = np.diff(np.append(roots, tree["num_nodes"]))
    assert sizes[-1] == 1 and len(set(sizes.tolist())) >= 4                      # (and so different depths: see the merged list's test)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def expected_shape(name, snap):
    """What the scene is in the list for."""
    g, top = snap["geo"], snap["top"]
    group = g["group_nodes"]
    top_widths, mesh_widths = np.diff(g["levels"]), np.diff(g["mesh_levels"])
    assert g["instanced"] and g["levels"][0] == 0 and g["levels"][-1] == g["top_nodes"] == top["top_nodes"] and np.array_equal(g["levels"], top["levels"])
    assert (top_widths > 0).all() and (mesh_widths > 0).all() and len(mesh_widths) == g["mesh_depth"] and len(top_widths) == g["top_levels"]
    assert g["top_nodes"] + g["mesh_levels"][-1] == snap["tree"]["num_nodes"] == g["num_nodes"]
    assert snap["tree"]["depth"] == g["top_levels"] + 1 + g["mesh_depth"]
    assert g["num_meshes"] == len(top["mesh_boxes"]) == len(g["mesh_roots"]) and g["num_instances"] == len(top["boxes"])
    if name == "lattice":
        assert g["num_meshes"] == 2 and g["num_instances"] == 6 and len(g["light_tris"]) == 2
    if name == "grid":
        assert g["num_instances"] == 1250 and top_widths.max() > group, "the top-level refit's launch path must run: " + str(top_widths)
    if name == "patch":
        assert g["num_meshes"] == 1 and snap["tree"]["num_triangles"] == 8192 + 2 and mesh_widths.max() > group >= mesh_widths.min(), str(mesh_widths)
    if name == "nine":
        assert g["num_meshes"] == 9 and mesh_widths[0] == 9 and g["mesh_depth"] >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_merged_list_and_identity_update(contexts, name):
    sc = base_scene(name)
    ctx = contexts(RGB, 0, BOTH)
    upload(ctx, sc)
    before = snapshot(ctx)
    expected_shape(name, before)
    g, t = before["geo"], before["tree"]
    # the merged list: every mesh node exactly once; level 0 the roots; level d + 1 exactly the inner children of level d
    nodes, first = g["mesh_level_nodes"], g["mesh_levels"]
    assert np.array_equal(np.sort(nodes), np.arange(g["top_nodes"], t["num_nodes"], dtype=np.uint32))
    assert np.array_equal(np.sort(nodes[first[0]:first[1]]), np.sort(g["mesh_roots"]))
    assert np.array_equal(g["mesh_roots"][t["instances"]["mesh"]], t["instances"]["root"])
    for d in range(g["mesh_depth"]):
        child = t["nodes"]["child"][nodes[first[d]:first[d + 1]]]
        inner = child[(child != abi.INVALID_CHILD) & ((child & abi.LEAF_FLAG) == 0)]
        nxt = nodes[first[d + 1]:first[d + 2]] if d + 1 < g["mesh_depth"] else nodes[:0]
        assert np.array_equal(np.sort(inner), np.sort(nxt)), "%s: merged level %d" % (name, d + 1)
    same_bytes(g["vertices"], sc.vertices, name + ": kept vertices as uploaded")
    # an identity update changes nothing
    ctx.set_vertices(sc.vertices)
    assert ctx.geometry_status() == 0
    after = snapshot(ctx)
    assert_same_snapshot(after, before, name + " identity")
    check_against_scene(after, before, sc, name + " identity")
    # the launches: four record kernels (three without loose lights), the mesh refit bounded by the deepest mesh, the boxes, the top level
    lights = 1 if len(g["light_tris"]) else 0
    assert 3 + lights + 1 + 1 + 1 <= after["geo"]["launches"] <= 3 + lights + g["mesh_depth"] + 1 + g["top_levels"]
    assert after["geo"]["packet_boxes"].shape[0] == 0                            # slrhip_rebuild_top_level has built no tables: nothing to refresh


@pytest.mark.gpu
@pytest.mark.parametrize("name,move", [(n, m) for n in NAMES for m in moves_of(n)])
def test_moved_trees_are_exact_and_records_equal_a_fresh_upload(contexts, name, move):
    sc = base_scene(name)
    ctx, fresh, third = contexts(RGB, 0, BOTH), contexts(RGB, 1, 0), contexts(RGB, 2, BOTH)
    upload(ctx, sc)
    original = snapshot(ctx)
    v, first, count = moved(name, move)
    ctx.set_vertices(v[first:first + count], first=first)
    assert ctx.geometry_status() == 0
    snap = snapshot(ctx)
    sc_moved = with_scene(sc, v)
    what = "%s %s" % (name, move)
    check_against_scene(snap, original, sc_moved, what)
    assert not np.array_equal(snap["tree"]["leaf_tris"], original["tree"]["leaf_tris"]), what
    loose, meshes = vertex_sets(name)
    if move == "loose":
        assert np.array_equal(snap["top"]["mesh_boxes"], original["top"]["mesh_boxes"]) and np.array_equal(snap["top"]["boxes"], original["top"]["boxes"])
    elif move in ("perturb", "one_mesh", "collapse"):                             # every vertex of at least one mesh moved
        assert not np.array_equal(snap["top"]["mesh_boxes"], original["top"]["mesh_boxes"]), what
        assert not np.array_equal(snap["top"]["boxes"], original["top"]["boxes"]), what
    if move == "collapse":
        k = len(meshes) // 2
        assert np.array_equal(snap["top"]["mesh_boxes"][k, 0], snap["top"]["mesh_boxes"][k, 1]), what + ": the collapsed mesh's box is a point"
    upload(fresh, sc_moved)
    upload(third, sc_moved)
    check_against_fresh(snap, fresh.debug_tree(), fresh.debug_top_level(), third.debug_geometry(), what)
    if move == "perturb":
        ctx.set_vertices(sc.vertices)                                             # and back: no drift
        assert ctx.geometry_status() == 0
        assert_same_snapshot(snapshot(ctx), original, what + " and back")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lattice", "nine"])
def test_bad_records_leave_their_vertices_and_set_the_status_bit(contexts, name):
    sc = base_scene(name)
    ctx, fresh, third = contexts(RGB, 0, BOTH), contexts(RGB, 1, 0), contexts(RGB, 2, BOTH)
    upload(ctx, sc)
    original = snapshot(ctx)
    v, _, n = moved(name, "perturb")
    loose, meshes = vertex_sets(name)
    bad = [int(loose[1]), int(meshes[0][len(meshes[0]) // 2]), int(meshes[-1][-1])]
    batch = v.copy()
    batch["position"][bad[0], 1] = np.nan
    batch["normal"][bad[1], 2] = np.inf
    batch["position"][bad[2], 0] = -np.inf
    ctx.set_vertices(batch)
    assert ctx.geometry_status() == abi.GEOMETRY_BAD_VERTEX
    assert ctx.geometry_status() == 0                          # read and cleared
    applied = v.copy()
    applied[bad] = sc.vertices[bad]
    snap = snapshot(ctx)
    same_bytes(snap["geo"]["vertices"][bad], sc.vertices[bad], name + ": the bad vertices keep their records")
    sc_applied = with_scene(sc, applied)
    check_against_scene(snap, original, sc_applied, name + " bad")
    assert not np.array_equal(snap["top"]["mesh_boxes"], original["top"]["mesh_boxes"])              # the rest of the call took effect
    upload(fresh, sc_applied)
    upload(third, sc_applied)
    check_against_fresh(snap, fresh.debug_tree(), fresh.debug_top_level(), third.debug_geometry(), name + " bad")
    rays = query_rays(name)
    assert_same(everything(ctx, rays), everything(fresh, rays), name + " bad")


@pytest.mark.gpu
@pytest.mark.parametrize("move", ["perturb", "collapse"])
@pytest.mark.parametrize("name", NAMES)
def test_updated_context_behaves_as_a_fresh_upload(contexts, name, move):
    sc = base_scene(name)
    ctx, fresh = contexts(RGB, 0, BOTH), contexts(RGB, 1, 0)
    upload(ctx, sc)
    v, first, count = moved(name, move)
    rays = query_rays(name)
    before = everything(ctx, rays)
    ctx.set_vertices(v[first:first + count], first=first)
    assert ctx.geometry_status() == 0
    got = everything(ctx, rays)
    upload(fresh, with_scene(sc, v))
    assert_same(got, everything(fresh, rays), "%s %s" % (name, move))
    # (grid and patch have ONE mesh and nothing else in view: collapsed onto a point it leaves a black frame and no instance to hit,
    # in both contexts alike)
    assert (np.nan_to_num(got["frame"], nan=1.0).max() > 0 and (got["hit_instances"] >= 0).any()) or (move == "collapse" and name in ("grid", "patch"))
    assert not np.array_equal(got["hits"].view(np.uint32), before["hits"].view(np.uint32))
    k, t = ctx.counters(), ctx.debug_tree(summary_only=True)
    assert k.bvh_nodes == t["num_nodes"] and k.bvh_depth == t["depth"]


@pytest.mark.gpu
def test_spectral_context(contexts):
    sc = base_scene("cornell")
    ctx, fresh = contexts(SPECTRAL, 0, BOTH), contexts(SPECTRAL, 1, 0)
    upload(ctx, sc)
    v, first, count = moved("cornell", "perturb")
    ctx.set_vertices(v[first:first + count], first=first)
    assert ctx.geometry_status() == 0
    upload(fresh, with_scene(sc, v))
    rays = query_rays("cornell")
    got = everything(ctx, rays)
    assert got["frame"].shape[-1] == 16 and got["frame"].max() > 0
    assert_same(got, everything(fresh, rays), "cornell perturb, spectral")


@pytest.mark.gpu
def test_shifted_lattice_equals_the_oracle(contexts):
    sc = base_scene("lattice")
    ctx = contexts(RGB, 0, BOTH)
    upload(ctx, sc)
    v, first, count = moved("lattice", "shift")
    ctx.set_vertices(v[first:first + count], first=first)
    ctx.render_begin(settings())
    ctx.render(0, SPP)
    got, k = ctx.read_framebuffer(), ctx.counters()
    frame, ctr = ob.load("oracle", RGB).scene(with_scene(sc, v)).render(settings(), SPP)
    assert_bit_equal(got, frame, "lattice shift vs the oracle")
    assert int(k.extension_rays) == int(ctr.extension_rays) and int(k.shadow_rays) == int(ctr.shadow_rays)


# ---- together with the other dynamic-scene calls --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lattice", "grid"])
def test_rebuild_after_loose_vertices_moved_seats_with_their_new_boxes(contexts, name):
    """slrhip_rebuild_top_level keeps a device table of the loose packets' boxes from its first call on: slrhip_set_vertices refreshes it."""
    sc = base_scene(name)
    ctx, fresh = contexts(RGB, 0, BOTH), contexts(RGB, 1, 0)
    upload(ctx, sc)
    ctx.rebuild_top_level()                                                       # the tables exist from here on
    info = ctx.debug_top_level_rebuild()
    packets = info["primitives"] - len(sc.instances)
    assert packets >= 1
    v, first, count = moved(name, "loose")
    ctx.set_vertices(v[first:first + count], first=first)
    assert ctx.geometry_status() == 0
    geo = ctx.debug_geometry()
    before = ctx.debug_top_level()
    tn = before["top_nodes"]
    # the refreshed table: packet p of the canonical order has the box of the slot that holds its child word
    words = before["nodes"][:tn]
    refs = info["refs"][len(sc.instances):]
    assert geo["packet_boxes"].shape == (packets, 2, 4)
    for p, ref in enumerate(refs):
        node, c = (int(x[0]) for x in np.nonzero(words[:, 24:28] == ref))
        planes = words[node, :24].view(F).reshape(6, 4)[:, c]
        assert np.array_equal(geo["packet_boxes"][p, 0, :3], planes[:3]) and np.array_equal(geo["packet_boxes"][p, 1, :3], planes[3:]), (name, p)
    ctx.rebuild_top_level()
    after = ctx.debug_top_level()
    want, keys, order = binding.top_level_reseat(before["nodes"], tn, before["boxes"])
    assert_same_nodes(after["nodes"], want, name + ": rebuild after the loose vertices moved")
    out = ctx.debug_top_level_rebuild()
    assert np.array_equal(out["keys"], keys) and np.array_equal(out["order"], order)
    sc_moved = with_scene(sc, v)
    check_tree(ctx.debug_tree(), sc_moved)
    upload(fresh, sc_moved)
    rays = query_rays(name)
    assert_same(everything(ctx, rays), everything(fresh, rays), name + ": rebuild, loose move, rebuild")
    # one launch more than without the tables
    upload(ctx, sc)
    ctx.set_vertices(v[first:first + count], first=first)
    launches_without = ctx.debug_geometry()["launches"]
    assert geo["launches"] == launches_without + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_instances_place_against_the_new_mesh_boxes(contexts, name):
    sc = base_scene(name)
    ctx, fresh = contexts(RGB, 0, BOTH), contexts(RGB, 1, 0)
    upload(ctx, sc)
    v, first, count = moved(name, "perturb")
    ctx.set_vertices(v[first:first + count], first=first)
    rec, lo, n = T.moved(name, "perturb")
    ctx.set_instance_transforms(rec[lo:lo + n], first=lo)
    assert ctx.geometry_status() == 0 and ctx.instances_status() == 0
    sc_moved = with_scene(sc, v, rec)
    check_tree(ctx.debug_tree(), sc_moved)
    upload(fresh, sc_moved)
    top, want = ctx.debug_top_level(), fresh.debug_top_level()
    for k in ("boxes", "mesh_boxes"):
        assert np.array_equal(top[k], want[k]), (name, k)
    same_bytes(top["instances"][:, :32], want["instances"][:, :32], name + ": the matrices")
    rays = query_rays(name)
    assert_same(everything(ctx, rays), everything(fresh, rays), name + ": vertices, then placements")
    # and the other way round: placements first, vertices second, give the same context
    upload(ctx, sc)
    ctx.set_instance_transforms(rec[lo:lo + n], first=lo)
    ctx.set_vertices(v[first:first + count], first=first)
    again = ctx.debug_top_level()
    for k in ("boxes", "mesh_boxes", "nodes", "instances"):
        assert np.array_equal(again[k].view(np.uint32), top[k].view(np.uint32)), (name, k)


@pytest.mark.gpu
def test_nothing_is_reset_between_two_renders(contexts):
    """render, set_vertices, render with no render_begin between: the sensor holds the first passes of the old scene and the later passes of
    the new one, added in pass order."""
    sc = base_scene("lattice")
    ctx, fresh = contexts(RGB, 0, BOTH), contexts(RGB, 1, 0)
    v, first, count = moved("lattice", "perturb")
    half = SPP // 2

    def passes(c, which):
        out = []
        for p in which:
            c.render_begin(settings())
            c.render(p, 1)
            out.append(c.read_framebuffer())
        return out
    upload(fresh, sc)
    old = passes(fresh, range(SPP))
    upload(fresh, with_scene(sc, v))
    new = passes(fresh, range(half, SPP))
    upload(ctx, sc)
    ctx.render_begin(settings())
    ctx.render(0, half)
    ctx.set_vertices(v[first:first + count], first=first)
    ctx.render(half, SPP - half)
    got = ctx.read_framebuffer()
    assert_bit_equal(got, kahan(old[:half] + new), "old first half + new second half")
    assert not np.array_equal(got, kahan(old))
    assert ctx.counters().samples == SIZE * SIZE * SPP


@pytest.mark.gpu
def test_the_new_flag_is_the_only_switch(contexts):
    sc = base_scene("lattice")
    v = moved("lattice", "perturb")[0]
    rays = query_rays("lattice")
    host = binding.host_tree(sc)
    # 512 alone: refused as before, nothing kept, nothing changed; 1024 alone: as no flag
    for flags, text in ((DYNAMIC, "the scene has instances"), (INSTANCED, "without SLRHIP_FLAG_DYNAMIC_GEOMETRY"), (0, "without SLRHIP_FLAG_DYNAMIC_GEOMETRY")):
        c = contexts(RGB, 3, flags)
        upload(c, sc)
        before = everything(c, rays)
        with pytest.raises(SlrHipError, match=r"slrhip_set_vertices failed \(%d\).*%s" % (UNSUPPORTED, text)):
            c.set_vertices(v)
        with pytest.raises(SlrHipError, match=r"slrhip_debug_geometry failed \(%d\)" % UNSUPPORTED):
            c.debug_geometry()
        assert c.geometry_status() == 0
        assert_same(everything(c, rays), before, text)
        got = c.debug_tree()
        for k in ("nodes", "leaf_tris", "shade_tris", "instances", "instance_boxes"):
            same_bytes(got[k], host[k], "flags %d: %s is the host's" % (flags, k))
    # with both, the same tree byte for byte
    both = contexts(RGB, 0, BOTH)
    upload(both, sc)
    got = both.debug_tree()
    for k in ("nodes", "leaf_tris", "shade_tris", "instances", "instance_boxes"):
        same_bytes(got[k], host[k], "both flags: %s is the host's" % k)
    # and a flat scene behaves in a context with both as in one with 512
    flat = V.base_scene("terrain8")
    fv = V.moved("terrain8", "perturb")[0]
    a, b = contexts(RGB, 0, BOTH), contexts(RGB, 2, DYNAMIC)
    for c in (a, b):
        c.upload_scene(flat)
        c.set_vertices(fv)
        assert c.geometry_status() == 0
    ga, gb = a.debug_geometry(), b.debug_geometry()
    assert not ga["instanced"] and ga["launches"] == gb["launches"]
    V.assert_same_snapshot(V.snapshot(a), V.snapshot(b), "a flat scene with both flags")


# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process: the check on a torch stream runs in a
# fresh child process that imports torch BEFORE libslrhip.so is loaded.
@pytest.mark.gpu
def test_later_calls_on_a_torch_stream_can_be_captured_in_a_graph():
    """The call allocates nothing and does not synchronise, so it replays from a graph with the eager result."""
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_vertex_update_instanced as I\nI._graph_check()\n" % (ROOT, os.path.join(ROOT, "tests")))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert "OK _graph_check" in p.stdout, p.stdout[-4000:] + "\n" + p.stderr[-3000:]


def _graph_check():
    import torch
    ctx = Context(device=0, flags=BOTH)
    try:
        for name in ("lattice", "patch"):
            sc = base_scene(name)
            v = moved(name, "perturb")[0]
            ctx.upload_scene(sc)
            ctx.rebuild_top_level()                                               # its tables exist: the call refreshes them too
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                new = torch.from_numpy(v.view(F).reshape(-1, 11).copy()).cuda()
                old = torch.from_numpy(sc.vertices.view(F).reshape(-1, 11).copy()).cuda()
                ctx.set_vertices(new, stream=side)
                side.synchronize()
                want = snapshot(ctx)
                ctx.set_vertices(old, stream=side)                                # somewhere else, in between
                side.synchronize()
                assert not np.array_equal(ctx.debug_top_level()["nodes"], want["top"]["nodes"])
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    ctx.set_vertices(new, stream=torch.cuda.current_stream())
                g.replay()
                torch.cuda.synchronize()
            assert ctx.geometry_status(side) == 0
            got = snapshot(ctx)
            assert_same_snapshot(got, want, name + " replayed from a graph")
            same_bytes(got["geo"]["packet_boxes"], want["geo"]["packet_boxes"], name + ": packet boxes")
        print("OK _graph_check", flush=True)
    finally:
        ctx.close()
