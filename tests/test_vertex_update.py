"""Moving vertices without a scene upload (slrhip_set_vertices, contexts created with SLRHIP_FLAG_DYNAMIC_GEOMETRY).

CPU: the exports and the two #defines; every refusal through the context-free check, with its code and message.

GPU: an update with the uploaded vertices changes nothing; after every move the tree passes tree_checks.check_tree against the moved
scene (exact unions: leaf_box and inner_box are equalities) with its shape untouched; every record equals the fresh upload's; and a
context that was updated renders, answers queries and fills feature and albedo buffers bit for bit as a context freshly uploaded with
the moved scene does.  The yardstick throughout is the fresh upload (and, on the exact lattice scene, the oracle); no tolerance is
involved."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from helpers import assert_bit_equal, ray_rows
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, DeviceBlocks, SlrHipError
from test_tree_builders import SMALL_CUT, cut_scene
from tree_checks import check_tree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
SIZE, SPP = 32, 8
DYNAMIC, DEVICE, SPLITS = abi.FLAG_DYNAMIC_GEOMETRY, abi.FLAG_BVH_DEVICE_BUILD, abi.FLAG_BVH_SPATIAL_SPLITS
RGB, SPECTRAL = abi.MODE_RGB, abi.MODE_SPECTRAL

# name -> (scene, context flags besides DYNAMIC, mode, the builder the summary must name, a lattice scene)
CASES = {
    "terrain8": ("terrain8", 0, RGB, "host SAH", True),
    "cut1": ("cut1", 0, RGB, "host SAH", True),
    "cut5": ("cut5", 0, RGB, "host SAH", True),
    "terrain23_device": ("terrain23", DEVICE, RGB, "device", True),
    "deck_device": ("deck", DEVICE, RGB, "device", True),
    "grid400_host": ("grid400", 0, RGB, "host SAH", True),
    "grid400_device": ("grid400", DEVICE, RGB, "device", True),
    "textured": ("textured", 0, RGB, "host SAH", False),
    "cornell": ("cornell", 0, RGB, "host SAH", False),
    "cornell_spectral": ("cornell", 0, SPECTRAL, "host SAH", False),
}
SMALL = ["terrain8", "cut1", "cut5", "terrain23_device", "deck_device", "textured", "cornell", "cornell_spectral"]
LARGE = ["grid400_host", "grid400_device"]
BEHAVIOUR = ["terrain8", "cut1", "cut5", "cornell", "cornell_spectral", "textured", "terrain23_device"]


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name == "terrain8":
        return scenes.lattice_terrain(8)
    if name.startswith("cut"):
        return cut_scene(base_scene("terrain8"), SMALL_CUT[:int(name[3:])], name)
    if name == "terrain23":
        return scenes.lattice_terrain(23)
    if name == "deck":
        return scenes.quad_deck()
    if name == "grid400":
        return scenes.lattice_grid(400)
    if name == "textured":
        return scenes.cornell_textured(1.0, 16, 8)
    if name == "instanced":
        return scenes.lattice_instanced()
    assert name == "cornell"
    return scenes.cornell_box_spheres(1.0, 8, 4, "glass")


def settings(seed=9):
    return ob.settings(SIZE, SIZE, seed=seed)


def with_vertices(sc, vertices):
    """The scene with another vertex array: what a fresh context uploads."""
    assert sc.env is None and len(sc.instances) == 0
    return abi.Scene(vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, None, sc.name + "_moved", textures=sc.textures,
                     texture_texels=sc.texture_texels, texture_texels_uvs=sc.texture_texels_uvs)


def used_vertices(sc):
    return np.unique(sc.triangles["v"])


def perturbed(case, seed=5):
    """A seeded random displacement per vertex of up to half a cell (the lattice's cell is 1; the box scenes get 0.02 of their unit
    size): boxes overlap and the tree fits badly."""
    sc = base_scene(CASES[case][0])
    rng = np.random.default_rng(seed)
    reach = 0.5 if CASES[case][4] else 0.02
    v = sc.vertices.copy()
    v["position"] = (v["position"].astype(np.float64) + rng.uniform(-reach, reach, v["position"].shape)).astype(F)
    v["texcoord"] = (v["texcoord"] + rng.uniform(-0.05, 0.05, v["texcoord"].shape)).astype(F)
    return v


def moved(case, move):
    """(the full vertex array after the move, first, count): what the update call is given is rows first .. first + count."""
    sc = base_scene(CASES[case][0])
    n = len(sc.vertices)
    if move == "identity":
        return sc.vertices.copy(), 0, n
    if move == "shift":
        # an exact quarter-lattice offset per vertex on the heights: every coordinate stays exact, so the oracle stays bit-exact
        assert CASES[case][4]
        v = sc.vertices.copy()
        v["position"][:, 1] += (np.random.default_rng(6).integers(-2, 3, n) * 0.25).astype(F)
        return v, 0, n
    if move == "perturb":
        return perturbed(case), 0, n
    if move == "collapse":
        # every vertex of a few triangles onto one point: new degenerate triangles, the first emitter among them
        v = sc.vertices.copy()
        emitters = np.nonzero(sc.materials["emittance"][sc.triangles["material"]] >= 0)[0]
        chosen = sorted(set([0, len(sc.triangles) // 2, int(emitters[0])]))
        for t in chosen:
            idx = sc.triangles["v"][t]
            v["position"][idx] = v["position"][idx[0]]
        return v, 0, n
    assert move == "partial"
    first, count = n // 3, max(1, n // 3)
    v = sc.vertices.copy()
    v[first:first + count] = perturbed(case)[first:first + count]
    return v, first, count


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


def pair(contexts, case):
    """(the dynamic context, the fresh one without the flag) of a case."""
    _, flags, mode, _, _ = CASES[case]
    return contexts(mode, 0, flags | DYNAMIC), contexts(mode, 1, flags)


def snapshot(ctx):
    return dict(tree=ctx.debug_tree(), geo=ctx.debug_geometry())


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    differ = a.view(np.uint8) != b.view(np.uint8)
    assert not differ.any(), "%s: %d of %d bytes differ" % (what, differ.sum(), differ.size)


def assert_same_snapshot(got, want, what):
    """Assertion 1's comparison: float node planes as float values (+-0 compare equal: the order of the host's fmin is not the kernel's),
    everything else by bytes."""
    t, w = got["tree"], want["tree"]
    for k in ("builder", "num_nodes", "depth", "leaf_references", "num_triangles", "quantized"):
        assert t[k] == w[k], (what, k)
    for plane in ("lo", "hi"):
        assert np.array_equal(t["nodes"][plane], w["nodes"][plane]), "%s: node planes %s differ" % (what, plane)
    same_bytes(t["nodes"]["child"], w["nodes"]["child"], what + ": child words")
    same_bytes(t["nodes"]["pad"], w["nodes"]["pad"], what + ": pad words")
    assert (t["nodes_q"] is None) == (w["nodes_q"] is None)
    if t["nodes_q"] is not None:
        same_bytes(t["nodes_q"], w["nodes_q"], what + ": QNodeQ")
    same_bytes(t["leaf_tris"], w["leaf_tris"], what + ": LeafTri")
    same_bytes(t["shade_tris"], w["shade_tris"], what + ": ShadeTri")
    g, h = got["geo"], want["geo"]
    assert g["staged"] == h["staged"] and np.array_equal(g["levels"], h["levels"])
    same_bytes(g["vertices"], h["vertices"], what + ": kept vertices")
    same_bytes(g["light_tris"], h["light_tris"], what + ": LightTri")
    if g["staged"]:
        same_bytes(g["light_tris_staged"], h["light_tris_staged"], what + ": staged LightTri")
    same_bytes(g["tri_uv"], h["tri_uv"], what + ": triUV")
    same_bytes(g["alpha"], h["alpha"], what + ": alpha records")


def check_against_scene(snap, original, sc_moved, what):
    """Assertion 2: the validator on the moved scene, the shape untouched, the quantized nodes the host quantizer's of the refitted nodes."""
    t, o = snap["tree"], original["tree"]
    check_tree(t, sc_moved)
    same_bytes(t["nodes"]["child"], o["nodes"]["child"], what + ": child words")
    assert t["num_nodes"] == o["num_nodes"] and t["depth"] == o["depth"] and t["builder"] == o["builder"] and t["quantized"] == o["quantized"]
    same_bytes(t["leaf_tris"]["tri"], o["leaf_tris"]["tri"], what + ": LeafTri.tri")
    same_bytes(t["leaf_tris"]["alpha"], o["leaf_tris"]["alpha"], what + ": LeafTri.alpha")
    same_bytes(t["leaf_tris"]["pad"], o["leaf_tris"]["pad"], what + ": LeafTri.pad")
    if t["quantized"]:
        same_bytes(t["nodes_q"], binding.quantize_nodes(t["nodes"]), what + ": QNodeQ against the host quantizer")
    g = snap["geo"]
    same_bytes(g["vertices"], sc_moved.vertices, what + ": kept vertices")
    if g["staged"]:
        same_bytes(g["light_tris_staged"], g["light_tris"], what + ": the two copies of the lights")


def check_against_fresh(snap, fresh_tree, fresh_flagged_geo, what):
    """Assertion 3: the records against a fresh upload of the moved scene."""
    t = snap["tree"]
    same_bytes(t["shade_tris"], fresh_tree["shade_tris"], what + ": ShadeTri against the fresh upload")
    a, b = t["leaf_tris"], fresh_tree["leaf_tris"]
    same_bytes(a[np.argsort(a["tri"], kind="stable")], b[np.argsort(b["tri"], kind="stable")], what + ": LeafTri by triangle against the fresh upload")
    if fresh_flagged_geo is not None:
        for k in ("light_tris", "tri_uv", "alpha", "vertices"):
            same_bytes(snap["geo"][k], fresh_flagged_geo[k], "%s: %s against the fresh upload" % (what, k))


def query_rays(sc, n=2048, seed=3):
    rng = np.random.default_rng(seed)
    used = sc.vertices["position"][used_vertices(sc)].astype(np.float64)
    lo, hi = used.min(axis=0), used.max(axis=0)
    pad = 0.25 * (hi - lo) + 0.5
    org = rng.uniform(lo - pad, hi + pad, (n, 3))
    target = used[rng.integers(0, len(used), n)] + rng.uniform(-0.25, 0.25, (n, 3))
    d = target - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return ray_rows(org, d, 0.0, 1.0e30)


def everything(ctx, rays, seed=9):
    """What a caller can get out of a context for its scene: the frame and its counters, closest hits and visibility of seeded rays,
    every feature buffer, the albedo."""
    ctx.render_begin(settings(seed))
    ctx.render(0, SPP)
    k = ctx.counters()
    out = dict(frame=ctx.read_framebuffer(), counters=np.array([k.samples, k.extension_rays, k.shadow_rays], np.uint64))
    out["hits"] = ctx.intersect_rays(rays)
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


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        same_bytes(got[k], want[k], "%s: %s" % (what, k))


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_exports_defines_and_version():
    lib = binding.load_library()
    for name in ("slrhip_set_vertices", "slrhip_geometry_status", "slrhip_debug_geometry_update_check", "slrhip_debug_geometry"):
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    debug = open(os.path.join(ROOT, "include", "slrhip_debug.h")).read()
    flag = re.search(r"#define SLRHIP_FLAG_DYNAMIC_GEOMETRY (\d+)u", header)
    assert flag and int(flag.group(1)) == abi.FLAG_DYNAMIC_GEOMETRY == 512
    others = [int(m) for m in re.findall(r"#define SLRHIP_FLAG_\w+\s+(\d+)u", header)]
    assert others.count(512) == 1 and all(v & (v - 1) == 0 for v in others) and len(set(others)) == len(others)
    bad = re.search(r"#define SLRHIP_GEOMETRY_BAD_VERTEX (\d+)u", header)
    assert bad and int(bad.group(1)) == abi.GEOMETRY_BAD_VERTEX == 1
    assert "int slrhip_set_vertices(slrhip_ctx* ctx, const slrhip_vertex* device_src, uint32_t first_vertex, uint32_t count, void* stream);" in header
    assert "int slrhip_geometry_status(slrhip_ctx* ctx, uint32_t* bits, void* stream);" in header
    assert "slrhip_debug_geometry_update_check(" in debug and "int slrhip_debug_geometry(slrhip_ctx* ctx, uint32_t what, void* host_dst, size_t num_words);" in debug
    assert lib.slrhip_version() == 7
    assert abi.vertex_dtype.itemsize == 44


def test_refusals_through_the_check_twin():
    lib = binding.load_library()
    check = lib.slrhip_debug_geometry_update_check
    ok = dict(have_scene=1, dynamic=1, builder=abi.TREE_HOST_SAH, num_instances=0, num_vertices=100, src=4096, first=20, count=80)

    def call(**over):
        a = dict(ok, **over)
        rc = check(a["have_scene"], a["dynamic"], a["builder"], a["num_instances"], a["num_vertices"], a["src"], a["first"], a["count"])
        return rc, lib.slrhip_last_error_string().decode()
    # the range exactly up to the end is accepted, from either builder that keeps whole triangles
    assert call()[0] == 0 and call(first=0, count=100)[0] == 0 and call(first=99, count=1)[0] == 0 and call(builder=abi.TREE_DEVICE)[0] == 0
    assert call(src=4096 + 4)[0] == 0                                          # 4-byte alignment is enough
    beyond = "first_vertex + count is beyond the scene's vertices"
    for over, code, text in ((dict(have_scene=0), NO_SCENE, "no scene uploaded"),
                             (dict(dynamic=0), UNSUPPORTED, "the context was created without SLRHIP_FLAG_DYNAMIC_GEOMETRY"),
                             (dict(num_instances=6), UNSUPPORTED, "the scene has instances"),
                             (dict(builder=abi.TREE_INSTANCED), UNSUPPORTED, "the scene has instances"),
                             (dict(builder=abi.TREE_HOST_SPATIAL_SPLITS), UNSUPPORTED, "the tree was built with spatial splits"),
                             (dict(src=None), INVALID, "null device_src"),
                             (dict(count=0), INVALID, "count must be >= 1"),
                             (dict(src=4096 + 2), INVALID, "misaligned device_src (4 bytes)"),
                             (dict(first=21), INVALID, beyond),                 # one past the end
                             (dict(first=100, count=1), INVALID, beyond),
                             (dict(first=1, count=0xFFFFFFFF), INVALID, beyond)):   # first + count wraps in 32 bits
        rc, msg = call(**over)
        assert rc == code and msg == "slrhip_set_vertices: " + text, (over, rc, msg)
    assert lib.slrhip_set_vertices(None, 4096, 0, 1, None) == INVALID
    bits_ = C.c_uint32(5)
    assert lib.slrhip_geometry_status(None, C.byref(bits_), None) == INVALID
    assert lib.slrhip_debug_geometry(None, 0, None, 0) == INVALID
    with pytest.raises(SlrHipError, match=r"failed \(%d\): slrhip_set_vertices: the scene has instances" % UNSUPPORTED):
        binding.geometry_update_check(True, True, abi.TREE_INSTANCED, 6, 100, 4096, 0, 1)
    binding.geometry_update_check(True, True, abi.TREE_HOST_SAH, 0, 100, 4096, 0, 100)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def upload(ctx, sc, builder=None):
    ctx.upload_scene(sc)
    if builder is not None:
        assert ctx.debug_tree(summary_only=True)["builder_name"] == builder, sc.name


def expected_shape(case, snap):
    """What the case is in the list for."""
    levels, group = snap["geo"]["levels"], snap["geo"]["group_nodes"]
    widths = np.diff(levels)
    assert levels[0] == 0 and levels[-1] == snap["tree"]["num_nodes"] and len(widths) == snap["tree"]["depth"] and (widths > 0).all()
    if case == "terrain8":
        assert snap["tree"]["num_triangles"] == 139 and widths.max() <= group
    if case == "cut1":
        assert snap["tree"]["num_nodes"] == 1 and snap["tree"]["leaf_references"] == 1
    if case == "cut5":
        assert snap["tree"]["depth"] == 1 or snap["tree"]["num_nodes"] <= 5
    if case == "terrain23_device":
        assert snap["tree"]["num_triangles"] == 1069
    if case in LARGE:
        assert snap["tree"]["num_triangles"] == 320011 and snap["tree"]["num_nodes"] >= 65536 and snap["tree"]["quantized"]
        assert widths.max() > group >= widths.min(), "both paths of the refit must run: " + str(widths)
    if case == "textured":
        assert len(snap["geo"]["tri_uv"]) == 2 * snap["tree"]["num_triangles"] and len(snap["geo"]["alpha"]) > 0
        assert (snap["tree"]["leaf_tris"]["alpha"] != 0xFFFFFFFF).any()
    if case.startswith("cornell"):
        assert snap["geo"]["staged"] and len(snap["geo"]["light_tris"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("case", SMALL + LARGE)
def test_identity_update_changes_nothing(contexts, case):
    name, _, _, builder, _ = CASES[case]
    sc = base_scene(name)
    ctx, _ = pair(contexts, case)
    upload(ctx, sc, builder)
    before = snapshot(ctx)
    expected_shape(case, before)
    same_bytes(before["geo"]["vertices"], sc.vertices, case + ": kept vertices as uploaded")
    ctx.set_vertices(sc.vertices)
    assert ctx.geometry_status() == 0
    after = snapshot(ctx)
    assert after["geo"]["launches"] >= 4
    assert_same_snapshot(after, before, case + " identity")
    check_against_scene(after, before, sc, case + " identity")


def moves_of(case):
    return (["shift"] if CASES[case][4] else []) + ["perturb", "collapse", "partial"]


@pytest.mark.gpu
@pytest.mark.parametrize("case,move", [(c, m) for c in SMALL + LARGE for m in moves_of(c)])
def test_moved_tree_is_exact_and_records_equal_a_fresh_upload(contexts, case, move):
    name, flags, mode, builder, _ = CASES[case]
    sc = base_scene(name)
    ctx, fresh = pair(contexts, case)
    upload(ctx, sc, builder)
    original = snapshot(ctx)
    v, first, count = moved(case, move)
    ctx.set_vertices(v[first:first + count], first=first)
    assert ctx.geometry_status() == 0
    snap = snapshot(ctx)
    sc_moved = with_vertices(sc, v)
    what = "%s %s" % (case, move)
    check_against_scene(snap, original, sc_moved, what)
    used = used_vertices(sc)
    touched = (v["position"][used].view(np.uint32) != sc.vertices["position"][used].view(np.uint32)).any()
    assert touched or case.startswith("cut"), what                      # (a cut scene keeps the terrain's vertex array: a range may miss its triangles)
    assert np.array_equal(snap["tree"]["leaf_tris"], original["tree"]["leaf_tris"]) != touched
    upload(fresh, sc_moved)
    fresh_tree = fresh.debug_tree()
    geo = None
    if case in SMALL:                                  # the light, texture-coordinate and alpha records of a fresh upload: from a flagged context
        third = contexts(mode, 2, flags | DYNAMIC)
        upload(third, sc_moved)
        geo = third.debug_geometry()
    check_against_fresh(snap, fresh_tree, geo, what)
    if move == "perturb":
        # and back: no drift
        ctx.set_vertices(sc.vertices)
        assert ctx.geometry_status() == 0
        assert_same_snapshot(snapshot(ctx), original, what + " and back")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["terrain8", "textured", "terrain23_device"])
def test_bad_records_leave_their_vertices_and_set_the_status_bit(contexts, case):
    name, flags, mode, builder, _ = CASES[case]
    sc = base_scene(name)
    ctx, fresh = pair(contexts, case)
    upload(ctx, sc, builder)
    original = snapshot(ctx)
    v, _, n = moved(case, "perturb")
    used = used_vertices(sc)
    bad = [int(used[1]), int(used[len(used) // 2]), int(used[-2])]
    batch = v.copy()
    batch["position"][bad[0], 1] = np.nan
    batch["normal"][bad[1], 2] = np.inf
    batch["texcoord"][bad[2], 0] = -np.inf
    ctx.set_vertices(batch)
    assert ctx.geometry_status() == abi.GEOMETRY_BAD_VERTEX
    assert ctx.geometry_status() == 0                          # read and cleared
    applied = v.copy()
    applied[bad] = sc.vertices[bad]
    snap = snapshot(ctx)
    same_bytes(snap["geo"]["vertices"][bad], sc.vertices[bad], case + ": the bad vertices keep their records")
    good = np.setdiff1d(np.arange(n), bad)
    assert not (snap["geo"]["vertices"]["position"][good] == sc.vertices["position"][good]).all(axis=1).any()
    sc_applied = with_vertices(sc, applied)
    check_against_scene(snap, original, sc_applied, case + " bad")
    upload(fresh, sc_applied)
    third = contexts(mode, 2, flags | DYNAMIC)
    upload(third, sc_applied)
    check_against_fresh(snap, fresh.debug_tree(), third.debug_geometry(), case + " bad")
    rays = query_rays(sc_applied)
    assert_same(everything(ctx, rays), everything(fresh, rays), case + " bad")


@pytest.mark.gpu
@pytest.mark.parametrize("move", ["perturb", "collapse"])
@pytest.mark.parametrize("case", BEHAVIOUR)
def test_updated_context_behaves_as_a_fresh_upload(contexts, case, move):
    name, _, _, builder, _ = CASES[case]
    sc = base_scene(name)
    ctx, fresh = pair(contexts, case)
    upload(ctx, sc, builder)
    v, first, count = moved(case, move)
    sc_moved = with_vertices(sc, v)
    rays = query_rays(sc_moved)
    before = everything(ctx, rays)
    ctx.set_vertices(v[first:first + count], first=first)
    assert ctx.geometry_status() == 0
    got = everything(ctx, rays)
    upload(fresh, sc_moved)
    want = everything(fresh, rays)
    assert_same(got, want, "%s %s" % (case, move))
    # (a collapsed emitter gives NaN samples, in both contexts alike; cut1's one triangle, the emitter, is a point then: a black frame)
    assert np.nan_to_num(got["frame"], nan=1.0).max() > 0 or (case == "cut1" and move == "collapse")
    assert not np.array_equal(got["hits"].view(np.uint32), before["hits"].view(np.uint32))
    k = ctx.counters()
    t = ctx.debug_tree(summary_only=True)
    assert k.bvh_nodes == t["num_nodes"] and k.bvh_depth == t["depth"]


@pytest.mark.gpu
def test_shifted_lattice_equals_the_oracle(contexts):
    sc = base_scene("terrain8")
    ctx, _ = pair(contexts, "terrain8")
    upload(ctx, sc)
    v, first, count = moved("terrain8", "shift")
    ctx.set_vertices(v[first:first + count], first=first)
    ctx.render_begin(settings())
    ctx.render(0, SPP)
    got, k = ctx.read_framebuffer(), ctx.counters()
    frame, ctr = ob.load("oracle", RGB).scene(with_vertices(sc, v)).render(settings(), SPP)
    assert_bit_equal(got, frame, "terrain8 shift vs the oracle")
    assert int(k.extension_rays) == int(ctr.extension_rays) and int(k.shadow_rays) == int(ctr.shadow_rays)
    assert np.isfinite(got).all() and got.max() > 0


def kahan(frames):
    """The sensor's per-pixel Kahan sum (BasicTypes/CompensatedSum.h:24-30) of per-pass frames, in float32."""
    result, comp = np.zeros_like(frames[0]), np.zeros_like(frames[0])
    for value in frames:
        c_input = value - comp
        sum_temp = result + c_input
        comp = (sum_temp - result) - c_input
        result = sum_temp
    return result


@pytest.mark.gpu
def test_nothing_is_reset_between_two_renders(contexts):
    """render, set_vertices, render with no render_begin between: the sensor holds the first passes of the old scene and the later
    passes of the new one, added in pass order."""
    sc = base_scene("terrain8")
    ctx, fresh = pair(contexts, "terrain8")
    v, first, count = moved("terrain8", "perturb")
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
    fresh.render_begin(settings())
    fresh.render(0, SPP)
    assert_bit_equal(kahan(old), fresh.read_framebuffer(), "the restated sensor sum against a plain render")
    upload(fresh, with_vertices(sc, v))
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
def test_refusals_on_a_live_context_change_nothing(contexts):
    lib = binding.load_library()
    sc = base_scene("terrain8")
    v = moved("terrain8", "perturb")[0]
    rays = query_rays(sc)
    empty = Context(device=0, flags=DYNAMIC)
    try:
        with pytest.raises(SlrHipError, match=r"slrhip_set_vertices failed \(%d\).*no scene uploaded" % NO_SCENE):
            empty.set_vertices(v)
        assert empty.geometry_status() == 0
        with pytest.raises(SlrHipError, match=r"slrhip_debug_geometry failed \(%d\)" % NO_SCENE):
            empty.debug_geometry()
    finally:
        empty.close()
    # no flag
    plain = contexts(RGB, 1, 0)
    upload(plain, sc)
    first = everything(plain, rays)
    with pytest.raises(SlrHipError, match=r"slrhip_set_vertices failed \(%d\).*without SLRHIP_FLAG_DYNAMIC_GEOMETRY" % UNSUPPORTED):
        plain.set_vertices(v)
    with pytest.raises(SlrHipError, match=r"slrhip_debug_geometry failed \(%d\)" % UNSUPPORTED):
        plain.debug_geometry()
    assert plain.geometry_status() == 0
    assert_same(everything(plain, rays), first, "no flag")
    # an instanced scene; spatial splits together with the flag
    inst = base_scene("instanced")
    for c, scene_, text in ((contexts(RGB, 0, DYNAMIC), inst, "the scene has instances"),
                            (contexts(RGB, 0, DYNAMIC | SPLITS), sc, "the tree was built with spatial splits")):
        upload(c, scene_)
        r = query_rays(scene_) if len(scene_.instances) == 0 else rays
        before = everything(c, r)
        with pytest.raises(SlrHipError, match=r"slrhip_set_vertices failed \(%d\).*%s" % (UNSUPPORTED, text)):
            c.set_vertices(scene_.vertices)
        assert c.geometry_status() == 0
        assert_same(everything(c, r), before, text)
    # argument errors on a context that would accept the call
    ctx = contexts(RGB, 0, DYNAMIC)
    upload(ctx, sc)
    before_snap, before = snapshot(ctx), everything(ctx, rays)
    n = len(v)
    with DeviceBlocks() as dev:
        p = dev.put(np.concatenate([v.view(F).reshape(-1), np.zeros(64, F)]))
        for args, code in (((None, 0, n), INVALID), ((p + 2, 0, n), INVALID), ((p, 0, 0), INVALID), ((p, 0, n + 1), INVALID), ((p, n, 1), INVALID),
                           ((p, 1, 0xFFFFFFFF), INVALID)):
            assert lib.slrhip_set_vertices(ctx.handle, *args, None) == code, args
            assert b"slrhip_set_vertices" in lib.slrhip_last_error_string()
        ctx.synchronize()
    assert ctx.geometry_status() == 0
    assert_same_snapshot(snapshot(ctx), before_snap, "after the refusals")
    assert_same(everything(ctx, rays), before, "after the refusals")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["terrain8", "grid400"])
def test_without_the_flag_the_tree_is_the_hosts(contexts, name):
    """The flag is the only switch: a context without it uploads what it always did."""
    sc = base_scene(name)
    ctx = contexts(RGB, 1, 0)
    upload(ctx, sc)
    got, want = ctx.debug_tree(), binding.host_tree(sc)
    for k in ("builder", "num_nodes", "depth", "leaf_references", "num_triangles", "quantized"):
        assert got[k] == want[k], k
    for k in ("nodes", "nodes_q", "leaf_tris", "shade_tris"):
        assert (got[k] is None) == (want[k] is None)
        if got[k] is not None:
            same_bytes(got[k], want[k], "%s without the flag: %s" % (name, k))
    with pytest.raises(SlrHipError, match=r"slrhip_debug_geometry failed \(%d\)" % UNSUPPORTED):
        ctx.debug_geometry()
    # and with it, the same tree
    flagged = contexts(RGB, 0, DYNAMIC)
    upload(flagged, sc)
    with_flag = flagged.debug_tree()
    for k in ("nodes", "nodes_q", "leaf_tris", "shade_tris"):
        if got[k] is not None:
            same_bytes(with_flag[k], got[k], "%s with the flag: %s" % (name, k))
