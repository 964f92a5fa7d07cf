"""Every tree builder's OUTPUT against the scene, without a ray: the host SAH build (bvh.cpp), the spatial-split build (sbvh.cpp), the
two-level instanced build and the GPU LBVH build (bvh_device.hip), read back through slrhip_debug_host_tree / slrhip_debug_tree and
checked by tree_checks.check_tree — structure, float boxes (exact: min and max do not round), leaf records, and the 8-bit boxes of the
quantized nodes against the single-rounded plane the traversal evaluates.  A box one ulp too small or a triangle missing from every
leaf shows up here always, not only when a ray grazes it.

CPU: the validator's own self-test (seven mutations of a valid tree, each rejected by name), the host builders on the edge scenes, the
host quantizer on synthetic nodes (slrhip_debug_quantize_nodes).  GPU (MI355X): which builder really ran, the device-built trees,
device records against the host's, determinism, the device quantizer against the host's, a deep Morton prefix chain.

The quantizer's domain: finite coordinates of magnitude at most 2^60.  An extent that overflows to infinity (bmax - bmin) is outside
it and is not generated here.

Looseness (tree_checks.LOOSE_STEPS = 2, derived there): measured on the host quantizer's own output over the families below, on the
UNROUNDED plane origin + q * scale no plane can move more than 1 step inwards and still contain its float plane in any family, so 2
always breaks containment (the test prints the figure per family: 2 for the general family, 1 for the others).  On the ROUNDED plane
the same measurement gives 1 for the identical-children, subnormal and wide-extent families and 128 for the general, flat and large-offset ones:
where the extent is a few ulps of the origin, scale is a fraction of one ulp and up to 127 consecutive q give the same float, so no
small bound exists there and none is a fault of the quantizer.  The bound is therefore asserted on the unrounded plane."""
import functools
import time

import numpy as np
import pytest

from slr_amd import abi, binding, scenes
from tree_checks import LOOSE_STEPS, TreeError, check_quantized, check_tree, fma_f32, loosest_steps

SPLITS = abi.FLAG_BVH_SPATIAL_SPLITS
DEVICE = abi.FLAG_BVH_DEVICE_BUILD


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def cut_scene(sc, keep, name):
    """`sc` with the triangles `keep` only (the vertices stay)."""
    return abi.Scene(sc.vertices, sc.triangles[np.asarray(keep)], sc.materials, sc.spectra, sc.spectrum_data, sc.camera, name=name)


def moved_scene(sc, offset, name):
    """`sc` with `offset` added to every coordinate, rounded to float32 (at 2^20 the quarter-lattice coordinates stay exact; the
    needle's 1/128 does not and becomes one more zero-thickness triangle).  The validator works from these float32 positions."""
    v = sc.vertices.copy()
    v["position"] = (v["position"].astype(np.float64) + offset).astype(np.float32)
    return abi.Scene(v, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, name=name)


# of the 139-triangle terrain: the two coincident emitting quads (128 .. 131), a wall, the collinear triangle, the one with two equal
# vertices, the needle, one ground triangle — the first k of them make the k-triangle scenes (triangle 128 emits: the scene is valid)
SMALL_CUT = (128, 129, 130, 131, 132, 136, 137, 138, 5)


@functools.lru_cache(maxsize=None)
def scene(name):
    if name == "terrain8":
        return scenes.lattice_terrain(8)
    if name == "terrain23":
        return scenes.lattice_terrain(23)
    if name == "deck":
        return scenes.quad_deck()
    if name == "lattice_instanced":
        return scenes.lattice_instanced(8)
    if name == "cornell":
        return scenes.cornell_box_spheres(1.0, 16, 8)
    if name == "cornell48":
        return scenes.cornell_box_spheres(4.0 / 3.0, 48, 24)
    if name == "cornell_instanced":
        return scenes.cornell_instanced()
    if name.startswith("cut"):
        return cut_scene(scene("terrain8"), SMALL_CUT[:int(name[3:])], name)
    if name == "terrain8_far":
        return moved_scene(scene("terrain8"), 2.0 ** 20, name)
    if name == "terrain23_far":
        return moved_scene(scene("terrain23"), 2.0 ** 20, name)
    if name.startswith("terrain23_last"):          # the last n triangles: the emitter and the degenerate triangles are among them
        n, sc = int(name[len("terrain23_last"):]), scene("terrain23")
        return cut_scene(sc, np.arange(len(sc.triangles) - n, len(sc.triangles)), name)
    if name == "grid400":
        return scenes.lattice_grid(400)
    if name == "planar":
        return planar_scene()
    if name == "skewed":
        return skewed_scene()
    raise KeyError(name)


def planar_scene(cells=32):
    """The deck's quads spread in x and z only: cells^2 unit quads at y = 1 (2 048 triangles), so every centroid has the same y and
    one Morton axis has zero extent.  The first quad emits."""
    b = scenes.SceneBuilder()
    light = b.matte(b.spectrum_grey(0.8), emittance=b.spectrum_d65(1.0, scenes.D65_RGB))
    grey = b.matte(b.spectrum_grey(0.5))
    for k in range(cells * cells):
        x, z = float(k % cells), float(k // cells)
        b.add_quad([(x, 1, z), (x + 1, 1, z), (x + 1, 1, z + 1), (x, 1, z + 1)], (0, -1, 0), (1, 0, 0), light if k == 0 else grey)
    return b.build(scenes._lattice_camera(cells), name="planar_%d" % cells)


def skewed_scene(clusters=22, per_cluster=50):
    """1 100 triangles in 22 clusters whose positions and sizes halve 21 times on all three axes: cluster k holds 50 triangles of size
    2^-k next to the point 2^-k (1, 1, 1), so half of the Morton range holds one cluster, half of the rest the next, and so on — a deep
    prefix chain in the radix tree.  Powers of two: every coordinate is exact.  The first triangle emits."""
    b = scenes.SceneBuilder()
    light = b.matte(b.spectrum_grey(0.8), emittance=b.spectrum_d65(1.0, scenes.D65_RGB))
    grey = b.matte(b.spectrum_grey(0.5))
    rng = np.random.default_rng(11)
    up, east, flat = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0), [(0, 0), (1, 0), (1, 1)]
    for k in range(clusters):
        s = 2.0 ** -k
        for t in range(per_cluster):
            corner = s * (1.0 + rng.integers(0, 64, 3) / 128.0)
            tri = corner[None, :] + s * rng.integers(0, 17, (3, 3)) / 128.0
            b.add_mesh(tri, [up] * 3, [east] * 3, flat, [(0, 1, 2)], light if (k == 0 and t == 0) else grey)
    return b.build(scenes._lattice_camera(2), name="skewed_%d" % (clusters * per_cluster))


def validate(tree, sc, builder, splits=False, stats=None):
    assert tree["builder_name"] == builder, (sc.name, tree["builder_name"])
    return check_tree(tree, sc, spatial_splits=splits, stats=stats)


# ---- CPU: the validator rejects what it must ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _valid_terrain_tree():
    tree = binding.host_tree(scene("terrain8"))
    tree["nodes_q"] = binding.quantize_nodes(tree["nodes"])          # a 57-node tree is not quantized by the upload: quantize it here
    check_tree(tree, scene("terrain8"))
    return tree


def _mutable(tree):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tree.items()}


def _slots(tree, want_leaf):
    child = tree["nodes"]["child"]
    valid = child != abi.INVALID_CHILD
    leaf = (child & abi.LEAF_FLAG) != 0
    return np.argwhere(valid & (leaf == want_leaf))


def _ulp_up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def mutate_box_plane(t):
    n, c = _slots(t, True)[3]
    t["nodes"]["lo"][n, 0, c] = _ulp_up(t["nodes"]["lo"][n, 0, c])


def mutate_leaf_count(t):
    for n, c in _slots(t, True):
        word = int(t["nodes"]["child"][n, c])
        if (word >> abi.LEAF_COUNT_SHIFT) & 0xF in (2, 3):
            t["nodes"]["child"][n, c] = word - (1 << abi.LEAF_COUNT_SHIFT)
            t["nodes_q"]["child"][n, c] = t["nodes"]["child"][n, c]
            return
    raise AssertionError("no packet of two or three triangles")


def mutate_drop_triangle(t):
    for n, c in _slots(t, True):
        word = int(t["nodes"]["child"][n, c])
        if (word >> abi.LEAF_COUNT_SHIFT) & 0xF >= 2:
            first = word & abi.LEAF_INDEX_MASK
            t["leaf_tris"][first + 1] = t["leaf_tris"][first]          # the packet's second triangle is gone, the first is there twice
            return
    raise AssertionError("no packet of two triangles")


def mutate_duplicate_child(t):
    inner = _slots(t, False)
    (n0, c0), (n1, c1) = inner[-1], inner[-2]
    assert n0 != n1 or c0 != c1
    t["nodes"]["child"][n1, c1] = t["nodes"]["child"][n0, c0]
    t["nodes_q"]["child"][n1, c1] = t["nodes"]["child"][n0, c0]


def mutate_e1(t):
    t["leaf_tris"]["e1"][7, 2] = _ulp_up(t["leaf_tris"]["e1"][7, 2])


def _tight_plane(t, which):
    """A quantized plane that is tight: one step inwards and the single-rounded plane has left the float plane behind."""
    nodes, q = t["nodes"], t["nodes_q"]
    valid = (nodes["child"] != abi.INVALID_CHILD)[:, None, :] & (q["scale"][:, :, None] > 0)
    step = 1 if which == "qlo" else -1
    moved = q[which].astype(np.int32) + step
    plane = fma_f32(np.clip(moved, 0, 255), q["scale"][:, :, None], q["origin"][:, :, None])[0]
    tight = valid & (moved >= 0) & (moved <= 255) & ((plane > nodes["lo"]) if which == "qlo" else (plane < nodes["hi"]))
    assert tight.sum() >= 0.5 * valid.sum(), "most planes of a quantized terrain tree are tight"
    return tuple(np.argwhere(tight)[0])


def mutate_qlo(t):
    t["nodes_q"]["qlo"][_tight_plane(t, "qlo")] += 1


def mutate_qhi(t):
    t["nodes_q"]["qhi"][_tight_plane(t, "qhi")] -= 1


MUTATIONS = {
    "box_plane_one_ulp_inwards": (mutate_box_plane, ("leaf_box",)),
    "leaf_count_changed": (mutate_leaf_count, ("leaf_cover",)),
    "triangle_dropped_from_its_packet": (mutate_drop_triangle, ("tri_once",)),
    "child_index_duplicated": (mutate_duplicate_child, ("reach_once", "child_order")),
    "e1_one_ulp": (mutate_e1, ("leaf_tri_record",)),
    "qlo_byte_plus_one": (mutate_qlo, ("q_contain",)),
    "qhi_byte_minus_one": (mutate_qhi, ("q_contain",)),
}


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_validator_rejects_a_mutated_tree_by_name(name):
    """A valid host tree of the 139-triangle terrain (quantized here), one mutation each: the validator must refuse it and name the
    rule.  The unmutated tree passes (checked when it is built)."""
    mutate, rules = MUTATIONS[name]
    t = _mutable(_valid_terrain_tree())
    mutate(t)
    with pytest.raises(TreeError) as e:
        check_tree(t, scene("terrain8"))
    assert e.value.rule in rules, (name, e.value.rule, str(e.value))


def test_validator_rejects_boxes_that_are_all_0_to_255():
    """What the looseness rule is for: every child box quantized to the whole node box is conservative and useless."""
    t = _mutable(_valid_terrain_tree())
    valid = (t["nodes"]["child"] != abi.INVALID_CHILD)[:, None, :]
    t["nodes_q"]["qlo"][np.broadcast_to(valid, t["nodes_q"]["qlo"].shape)] = 0
    t["nodes_q"]["qhi"][np.broadcast_to(valid, t["nodes_q"]["qhi"].shape)] = 255
    with pytest.raises(TreeError) as e:
        check_tree(t, scene("terrain8"))
    assert e.value.rule == "q_loose"


def test_single_rounded_plane_is_not_a_float32_multiply_and_add():
    """fma_f32 on planes picked so that the roundings differ: q * s rounds in float32, the fma does not; and a sum on a float32
    rounding boundary in float64 is decided by the exact value."""
    s, o = np.float32(1.0) + np.float32(2.0 ** -23), np.float32(-3.0)
    got, _ = fma_f32(np.array([3]), s, o)
    assert got[0] == np.float32(3 * 2.0 ** -23) and np.float32(np.float32(3) * s) + o != got[0]
    s, o = np.float32(2.0 ** -24 + 2.0 ** -47), np.float32(1.0)       # 1 + 2^-24 + 2^-47: just above the midpoint of 1 and 1 + 2^-23
    got, redone = fma_f32(np.array([1]), s, o)
    assert got[0] == np.float32(1.0 + 2.0 ** -23) and redone == 0
    s, o = np.float32(2.0 ** -24), np.float32(1.0)                    # the midpoints themselves: redone exactly, ties to even
    got, redone = fma_f32(np.array([1, 3]), s, o)
    assert redone == 2 and got[0] == np.float32(1.0) and got[1] == np.float32(1.0 + 2.0 ** -22)
    got, redone = fma_f32(np.array([255]), np.float32(0.0), np.float32(-7.5))      # scale 0: the plane is the origin
    assert got[0] == np.float32(-7.5) and redone == 0


# ---- CPU: the host builders -------------------------------------------------------------------------------------------------------
HOST_SCENES = ["terrain8", "terrain23", "deck", "lattice_instanced", "cornell", "cornell_instanced", "cut1", "cut2", "cut4", "cut5", "cut9",
               "terrain8_far"]


@pytest.mark.parametrize("splits", [False, True], ids=["sah", "spatial_splits"])
@pytest.mark.parametrize("name", HOST_SCENES)
def test_host_built_tree_is_valid(name, splits):
    """The host read-out of each edge scene, with and without FLAG_BVH_SPATIAL_SPLITS (an instanced scene ignores the flag: its trees
    are object-split).  On the Cornell scene the spatial-split tree must really hold duplicated references."""
    sc = scene(name)
    tree = binding.host_tree(sc, SPLITS if splits else 0)
    instanced = len(sc.instances) > 0
    builder = "instanced" if instanced else ("host spatial splits" if splits else "host SAH")
    validate(tree, sc, builder, splits and not instanced)
    assert not tree["quantized"]
    if splits and name == "cornell":
        assert tree["leaf_references"] > tree["num_triangles"]
    if not (splits and not instanced):
        assert tree["leaf_references"] == len(sc.triangles)
    # the shading records name every triangle's material, and the emitters in light-list order
    assert (tree["shade_tris"]["material"] == sc.triangles["material"]).all()
    lights = tree["shade_tris"]["light"]
    assert (np.sort(lights[lights >= 0]) == np.arange((lights >= 0).sum())).all() and (lights >= 0).any()


def test_host_built_large_tree_is_quantized_and_valid():
    """lattice_grid(400): 320 011 triangles, past the 65 536 nodes from which the upload quantizes — the float tree and the
    quantized records of the real thing (0.2 s of host build, about 2 s of validation)."""
    sc = scene("grid400")
    stats = {}
    tree = binding.host_tree(sc)
    validate(tree, sc, "host SAH", stats=stats)
    assert tree["quantized"] and tree["num_nodes"] >= 65536 and tree["nodes_q"] is not None
    again = binding.quantize_nodes(tree["nodes"])
    assert again.tobytes() == tree["nodes_q"].tobytes()               # the quantizer read-out IS the upload's quantizer


def test_host_read_out_refuses_a_scene_the_device_builds():
    with pytest.raises(binding.SlrHipError, match=r"\(5\).*device build"):
        binding.host_tree(scene("terrain23"), DEVICE)
    assert binding.host_tree(scene("terrain8"), DEVICE)["builder_name"] == "host SAH"        # below 1 024 triangles the flag is not honoured


# ---- CPU: the host quantizer on synthetic nodes -------------------------------------------------------------------------------------
NODES_PER_FAMILY = 4096


def _assemble(rng, lo, hi):
    """QNode records from child boxes lo / hi [n, 3, 4]: 1 to 4 valid children per node (the rest empty: +inf / -inf, kInvalidChild),
    child words a mix of inner indices and leaf references."""
    n = len(lo)
    nodes = np.zeros(n, abi.qnode_dtype)
    valid = np.arange(4)[None, :] < rng.integers(1, 5, n)[:, None]
    lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
    nodes["lo"] = np.where(valid[:, None, :], lo, np.inf)
    nodes["hi"] = np.where(valid[:, None, :], hi, -np.inf)
    inner = rng.integers(1, 1 << 20, (n, 4)).astype(np.uint32)
    leafs = (abi.LEAF_FLAG | (rng.integers(1, 5, (n, 4)) << abi.LEAF_COUNT_SHIFT) | rng.integers(0, 1 << 20, (n, 4))).astype(np.uint32)
    nodes["child"] = np.where(valid, np.where(rng.random((n, 4)) < 0.5, inner, leafs), abi.INVALID_CHILD)
    return nodes


def _lattice_family(rng, origin, units):
    """Child planes origin + i * ulp(origin) with i in 0 .. units (exact in float32): origin [n, 3] float32, units [n, 3] int."""
    unit = np.spacing(np.abs(origin)).astype(np.float64)
    i = rng.integers(0, units[:, :, None, None] + 1, (len(origin), 3, 4, 2))
    i[:, :, 0, 0], i[:, :, 1, 1] = 0, units                          # the node box spans the whole extent where 2 children are valid
    planes = (origin.astype(np.float64)[:, :, None, None] + i * unit[:, :, None, None]).astype(np.float32)
    assert (planes.astype(np.float64) == origin.astype(np.float64)[:, :, None, None] + i * unit[:, :, None, None]).all()
    return planes[..., 0], planes[..., 1]


def family(name, n=NODES_PER_FAMILY):
    rng = np.random.default_rng([20240611, sorted(FAMILIES).index(name)])
    if name == "general":
        centre = rng.uniform(-100.0, 100.0, (n, 3, 1))
        size = 10.0 ** rng.uniform(-3.0, 2.0, (n, 3, 1))
        lo = centre + size * rng.uniform(-1.0, 1.0, (n, 3, 4))
        hi = np.where(rng.random((n, 3, 4)) < 0.1, lo, lo + size * rng.uniform(0.0, 1.0, (n, 3, 4)))      # one child box in ten has no thickness
        return _assemble(rng, lo.astype(np.float32), hi.astype(np.float32))
    if name == "flat_axes":
        nodes = family("general", n).copy()
        flat = np.arange(3)[None, :] < rng.integers(1, 4, n)[:, None]                                       # one, two or three flat axes
        flat = rng.permuted(flat, axis=1)
        plane = rng.uniform(-100.0, 100.0, (n, 3, 1)).astype(np.float32)
        valid = (nodes["child"] != abi.INVALID_CHILD)[:, None, :]
        for key in ("lo", "hi"):
            nodes[key] = np.where(flat[:, :, None] & valid, plane, nodes[key])
        return nodes
    if name == "identical_children":
        lo = np.repeat(rng.uniform(-100.0, 100.0, (n, 3, 1)), 4, axis=2)
        hi = lo + np.repeat(10.0 ** rng.uniform(-3.0, 2.0, (n, 3, 1)), 4, axis=2)
        return _assemble(rng, lo.astype(np.float32), hi.astype(np.float32))
    if name == "large_offset_small_extent":
        # origin in [2^10, 2^23) with at least 4 096 ulps of room to the next power of two, so that the lattice origin + i * ulp is exact
        exponent = rng.integers(10, 23, (n, 3))
        origin = (2.0 ** exponent * (1.0 + rng.integers(0, (1 << 23) - 4096, (n, 3)) / 2.0 ** 23)).astype(np.float32)
        lo, hi = _lattice_family(rng, origin, rng.integers(1, 4097, (n, 3)))
        flip = rng.random((n, 3, 1)) < 0.5                              # the same boxes mirrored to the negative side
        return _assemble(rng, np.where(flip, -hi, lo), np.where(flip, -lo, hi))
    if name == "subnormal_extent":
        small = (2.0 ** -126 * (1.0 + rng.integers(0, 1 << 22, (n, 3)) / 2.0 ** 23)).astype(np.float32)     # small normals: their ulp is 2^-149 too
        origin = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), small)
        origin = np.where(rng.random((n, 3)) < 0.25, -origin - np.float32(512 * 2.0 ** -149), origin).astype(np.float32)      # and from below zero
        units = rng.integers(1, 513, (n, 3))
        step = np.float64(2.0 ** -149)
        i = rng.integers(0, units[:, :, None, None] + 1, (n, 3, 4, 2))
        i[:, :, 0, 0], i[:, :, 1, 1] = 0, units
        planes = (origin.astype(np.float64)[:, :, None, None] + i * step).astype(np.float32)
        assert (planes.astype(np.float64) == origin.astype(np.float64)[:, :, None, None] + i * step).all()
        return _assemble(rng, planes[..., 0], planes[..., 1])
    if name == "extents_2^-100_to_2^60":
        size = 2.0 ** rng.uniform(-100.0, 60.0, (n, 3, 1))
        base = np.where(rng.random((n, 3, 1)) < 0.5, 0.0, size * rng.uniform(-1.0, 0.0, (n, 3, 1)))        # every coordinate within +-size
        lo = base + size * rng.uniform(0.0, 0.5, (n, 3, 4))
        hi = lo + size * rng.uniform(0.0, 0.5, (n, 3, 4))
        return _assemble(rng, lo.astype(np.float32), hi.astype(np.float32))
    raise KeyError(name)


FAMILIES = ("general", "flat_axes", "identical_children", "large_offset_small_extent", "subnormal_extent", "extents_2^-100_to_2^60")


@pytest.mark.parametrize("name", FAMILIES)
def test_host_quantizer_is_conservative_and_tight(name, capsys):
    """quantizeNodes itself on 4 096 synthetic nodes per family: every dequantized box contains its float box under the traversal's
    single rounding, no plane is loose, empty slots are 255 / 0, the child words are copied, and an axis with bmax > bmin never
    takes the flat branch (scale 0).  Finite coordinates up to 2^60; extents that overflow are outside the domain.

    subnormal_extent failed before the fix of quantizeNodes: a node box thinner than 128 subnormal units had (bmax - bmin) / 255
    round to 0, took the flat branch and put both planes at the origin, below bmax.  Recorded on the quantizer as it was: scale 0 on
    4 091 of the 12 258 axes with bmax > bmin, and
    "[q_contain] dequantized upper plane below the float box (8419 places, first at (0, 2, 0))"."""
    nodes = family(name)
    valid = np.broadcast_to((nodes["child"] != abi.INVALID_CHILD)[:, None, :], nodes["lo"].shape)
    for key in ("lo", "hi"):                                           # the domain
        assert np.isfinite(nodes[key][valid]).all() and np.abs(nodes[key][valid]).max() <= 2.0 ** 60
    assert (nodes["lo"][valid] <= nodes["hi"][valid]).all()
    q = binding.quantize_nodes(nodes)
    stats = {}
    bmin = np.where(valid, nodes["lo"], np.inf).min(axis=2)
    bmax = np.where(valid, nodes["hi"], -np.inf).max(axis=2)
    with capsys.disabled():
        print("\n%s: %d nodes, %d axes with an extent, %d flat; smallest loose_steps that passes: unrounded planes %d, rounded planes %d"
              % (name, len(nodes), (bmax > bmin).sum(), (bmax == bmin).sum(), loosest_steps(nodes, q), loosest_steps(nodes, q, rounded=True)))
    assert (q["origin"] == bmin).all()
    assert ((q["scale"] > 0) == (bmax > bmin)).all(), "a non-zero extent never takes the flat branch, a zero extent always does"
    check_quantized(nodes, q, LOOSE_STEPS, stats)
    if name == "flat_axes":
        assert (bmax == bmin).sum() >= len(nodes)
    if name == "subnormal_extent":
        assert ((bmax - bmin) < np.float32(128 * 2.0 ** -149)).sum() >= 1000           # the extents that used to round to scale 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def upload(sc, flags=0):
    ctx = binding.Context(flags=flags)
    try:
        ctx.upload_scene(sc)
        return ctx.debug_tree()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_the_summary_names_the_builder_that_ran():
    """FLAG_BVH_DEVICE_BUILD is honoured from 1 024 triangles on: the 1 069-triangle terrain, the deck and the Cornell spheres are
    built on the device; the 139-triangle terrain gets the host SAH build under the same flag, silently."""
    for name in ("terrain23", "deck", "cornell48"):
        ctx = binding.Context(flags=DEVICE)
        try:
            ctx.upload_scene(scene(name))
            assert ctx.debug_tree(summary_only=True)["builder_name"] == "device", name
        finally:
            ctx.close()
    for flags, want in ((DEVICE, "host SAH"), (0, "host SAH"), (SPLITS, "host spatial splits")):
        ctx = binding.Context(flags=flags)
        try:
            ctx.upload_scene(scene("terrain8"))
            assert ctx.debug_tree(summary_only=True)["builder_name"] == want, flags
            ctx.upload_scene(scene("lattice_instanced"))
            assert ctx.debug_tree(summary_only=True)["builder_name"] == "instanced", flags
        finally:
            ctx.close()


DEVICE_SCENES = ["terrain23", "terrain23_last1024", "terrain23_last1025", "deck", "terrain23_far", "cornell48", "planar"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEVICE_SCENES)
def test_device_built_tree_is_valid_and_its_records_equal_the_hosts(name):
    """The LBVH build's tree through the validator (every triangle in exactly one packet, packets contiguous, boxes exact), its
    ShadeTri records bit-equal to the host loop's (NaN for NaN on the degenerate triangles) and its LeafTri records equal to the host
    tree's as a multiset.  terrain23 is the smallest terrain the device build takes: degenerate and coincident triangles, 1 069 of
    them (no multiple of 256); the cuts sit on and one past the 1 024 threshold; the deck has all Morton codes equal; planar has one
    Morton axis without extent."""
    sc = scene(name)
    tree = upload(sc, DEVICE)
    validate(tree, sc, "device")
    host = binding.host_tree(sc)
    assert host["builder_name"] == "host SAH"
    assert tree["shade_tris"].tobytes() == host["shade_tris"].tobytes()
    if name.startswith("terrain23"):
        assert np.isnan(tree["shade_tris"]["gnx"]).sum() >= 2             # the collinear triangle and the one with two equal vertices
    by_tri = lambda a: a[np.argsort(a["tri"], kind="stable")].tobytes()
    assert by_tri(tree["leaf_tris"]) == by_tri(host["leaf_tris"])


@pytest.mark.gpu
def test_host_trees_read_back_from_the_device_are_the_host_read_outs():
    """slrhip_debug_tree on uploads that take the host builders gives the arrays slrhip_debug_host_tree gives, byte for byte, and the
    instanced scene's read-out agrees with slrhip_debug_top_level."""
    for name, flags in (("terrain8", 0), ("terrain8", SPLITS), ("lattice_instanced", 0), ("cornell_instanced", 0)):
        sc = scene(name)
        ctx = binding.Context(flags=flags)
        try:
            ctx.upload_scene(sc)
            tree = ctx.debug_tree()
            top = ctx.debug_top_level() if len(sc.instances) else None
        finally:
            ctx.close()
        host = binding.host_tree(sc, flags)
        validate(tree, sc, host["builder_name"], flags == SPLITS)
        for key, value in host.items():
            same = tree[key].tobytes() == value.tobytes() if isinstance(value, np.ndarray) else tree[key] == value
            assert same, (name, key)
        if top is not None:
            assert top["nodes"].tobytes() == tree["nodes"].tobytes() and top["top_nodes"] == tree["top_nodes"]
            assert top["boxes"].tobytes() == tree["instance_boxes"].tobytes()


@pytest.mark.gpu
def test_device_build_is_deterministic():
    """Two uploads of the 1 069-triangle terrain in two contexts: byte-identical node, leaf and shading arrays."""
    a, b = upload(scene("terrain23"), DEVICE), upload(scene("terrain23"), DEVICE)
    assert a["builder_name"] == b["builder_name"] == "device"
    for key in ("nodes", "leaf_tris", "shade_tris"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert (a["num_nodes"], a["depth"]) == (b["num_nodes"], b["depth"])


@pytest.mark.gpu
def test_device_quantizer_equals_the_host_quantizer():
    """The QNodeQ records k_collapse_emit writes against quantizeNodes of bvh.cpp on the same float nodes, bit for bit, on a
    device-built tree that the summary reports as quantized, and the quantized rules on them.  It was lattice_grid(400): its device
    tree has 94 925 nodes in 13 levels on the MI355X, past the 65 536 from which the nodes are quantized, so lattice_grid(640) was
    not needed.  0.3 s, of which the upload and the read-out take 0.01 s."""
    sc = scene("grid400")
    t0 = time.time()
    tree = upload(sc, DEVICE)
    t1 = time.time()
    assert tree["builder_name"] == "device" and tree["quantized"] and tree["num_nodes"] >= 65536, (tree["num_nodes"], tree["quantized"])
    host_q = binding.quantize_nodes(tree["nodes"])
    differ = np.nonzero((host_q.view(np.uint32).reshape(-1, 16) != tree["nodes_q"].view(np.uint32).reshape(-1, 16)).any(axis=1))[0]
    assert len(differ) == 0, "%d of %d quantized nodes differ, first node %d" % (len(differ), len(host_q), differ[0])
    validate(tree, sc, "device")
    print("device grid400: %d nodes, %d levels, upload + read-out %.2f s, checks %.2f s" % (tree["num_nodes"], tree["depth"], t1 - t0, time.time() - t1))


@pytest.mark.gpu
def test_skewed_scene_uploads_valid_or_is_refused_cleanly():
    """A deep Morton prefix chain (skewed_scene) under FLAG_BVH_DEVICE_BUILD must either upload and validate, or be refused with a
    non-zero code and a message, after which the context holds no scene (slrhip_render_begin: SLRHIP_ERR_NO_SCENE) and takes the same
    scene with the host build.  Nothing is traversed.  Outcome on the MI355X: it uploads — 324 nodes in 17 levels (52 of the 64 stack
    entries) — and validates; the refusal branch stays for a build that comes out deeper."""
    sc = scene("skewed")
    assert len(sc.triangles) == 1100
    ctx = binding.Context(flags=DEVICE)
    try:
        try:
            ctx.upload_scene(sc)
            outcome = "uploaded"
        except binding.SlrHipError as e:
            outcome = str(e)
            assert "failed (0)" not in outcome and len(outcome) > 40, outcome
            with pytest.raises(binding.SlrHipError, match=r"failed \(4\)"):          # SLRHIP_ERR_NO_SCENE
                ctx.render_begin(abi.RenderSettings(8, 8, 0.0, 0.0, 1.0, 1))
        if outcome == "uploaded":
            tree = ctx.debug_tree()
            validate(tree, sc, "device")
            print("skewed scene: uploaded, %d nodes, %d levels" % (tree["num_nodes"], tree["depth"]))
        else:
            print("skewed scene: refused: " + outcome)
    finally:
        ctx.close()
    if outcome != "uploaded":
        validate(upload(sc, 0), sc, "host SAH")
    validate(binding.host_tree(sc), sc, "host SAH")
