"""Ray traversal against a brute-force reference on the rays a general-position family never holds (helpers.special_rays): direction
components that are +0.0 or -0.0 (1 / dir = +-inf, and the slab product 0 * inf = NaN where the origin lies on a box plane), rays
through shared vertices and edges, origins on a surface, dist_min / dist_max exactly at the hit distance, zero-thickness boxes,
coincident and degenerate triangles, stacks deeper than their LDS part, batches that do not fill a wave or the ray ring.

The reference asks the tree-free question — of all triangles, which does this ray hit first? — with the kernels' own float32
arithmetic (helpers.brute_force_hits) on scenes whose coordinates are exact (scenes.lattice_terrain and its kin), so every ray
has ONE right answer and no ray is exempted on the device side.  CPU: the reference against the oracle's tree and against a
float64 evaluation, the scene generators, the families.  GPU (MI355X): slrhip_trace_rays (k_trace_batch),
slrhip_intersect_rays and slrhip_test_visibility (k_ring_ws with the query client: closest hit, any hit, the quantized and the instanced variants) on
every tree the upload builds.

Measured on the CPU (8 threads): the brute force takes 0.1 s on the 139-triangle terrain (6 532 rays), 0.6 s on the 1 069-triangle
terrain the device build takes (6 271 rays: every k-th of its family), 0.1 s on the instanced
scene (586 candidates), 0.6 s on the 8 192-triangle deck (1 516 rays) and 1.1 s on the 320 011-triangle grid (404 rays; 0.4 s more
for the 121 base rays of its intervals)."""
import functools

import numpy as np
import pytest

from helpers import (DIAGONALS, INTERVALS, bits, brute_force_hits, every_kth, ray_rows, rays_on_planes, special_rays, sub_family)
from slr_amd import abi, binding, scenes

MISS = abi.MISS
N = 8                                   # cells per side of the small lattice scenes
N23 = 23                                # ... and of the terrain that is large enough for the device build
GRID_N = 400
GRID_COORDS = (-0.5, 0.0, 0.5, 57.0, 113.5, 200.0, 286.5, 343.0, 399.5, 400.0, 400.5)       # of the 801 half-lattice values


class Case:
    """A scene, its family of special rays and the brute-force answer; built once, shared, read-only."""

    def __init__(self, sc, rows, tags, planes, all_miss=()):
        self.sc, self.rows, self.tags, self.planes, self.all_miss = sc, rows, tags, planes, all_miss
        self.family = sub_family(tags)
        self.ref = brute_force_hits(sc, rows)
        for a in (self.rows, self.tags, self.family) + tuple(v for v in vars(self.ref).values() if isinstance(v, np.ndarray)):
            a.flags.writeable = False


def _bounds(sc, first=0, count=None):
    p = sc.vertices["position"][sc.triangles["v"][first:None if count is None else first + count].reshape(-1)]
    return p.min(axis=0), p.max(axis=0)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "terrain":
        sc = scenes.lattice_terrain(N)
        return Case(sc, *special_rays(sc, N), _bounds(sc))
    if name == "terrain23":
        # the smallest terrain the device build takes (1 069 triangles; below 1 024 the upload builds on the host whatever the flag says)
        sc = scenes.lattice_terrain(N23)
        return Case(sc, *every_kth(*special_rays(sc, N23), 8192), _bounds(sc))
    if name == "instanced":
        # the terrain's own box, where the 0 * inf arises at the root of the MESH's tree: the first two placements are the identity
        sc = scenes.lattice_instanced(N)
        first, count = int(sc.instances[0]["first_triangle"]), int(sc.instances[0]["num_triangles"])
        return Case(sc, *special_rays(sc, N, first_triangle=first), _bounds(sc, first, count))
    if name == "deck":
        # one plane: no horizontal ray and no degenerate ray can hit anything (there is no second surface)
        sc = scenes.quad_deck()
        return Case(sc, *special_rays(sc, 4, horizontal=False), _bounds(sc), all_miss=("degenerate",))
    if name == "grid":
        sc = scenes.lattice_grid(GRID_N)
        return Case(sc, *every_kth(*special_rays(sc, GRID_N, coords=GRID_COORDS), 512), _bounds(sc))
    raise KeyError(name)


def assert_family_not_degenerate(c, what):
    """Conditions on the INPUT (the reference's answers), not measurements of the device."""
    ref = c.ref
    share = ref.hit.mean()
    assert 0.5 <= share <= 0.999, (what, "hit share", share)
    assert (ref.tie_size[ref.hit] > 1).mean() >= 0.2, (what, "hits with a tie set larger than one", (ref.tie_size[ref.hit] > 1).mean())
    assert rays_on_planes(c.rows, *c.planes).sum() >= 100, (what, "rays along a bounding plane", int(rays_on_planes(c.rows, *c.planes).sum()))
    for f in sorted(set(c.family)):
        m = c.family == f
        if f in c.all_miss:
            assert not ref.hit[m].any(), (what, f)
            continue
        assert ref.hit[m].any(), (what, f, "no hit")
        assert f == "surface" or (~ref.hit[m]).any(), (what, f, "no miss")


# ---- CPU: the scenes ----------------------------------------------------------------------------------------------------------
def test_lattice_scenes_are_exact_and_hold_their_special_triangles():
    sc = case("terrain").sc
    assert len(sc.triangles) == 2 * N * N + 11 == 139
    pos = sc.vertices["position"].astype(np.float64)
    quarter = pos * 4 == np.round(pos * 4)
    assert quarter.sum() == quarter.size - 1 and (np.abs(pos) < 16).all()                   # the needle's 6.0078125 is the one exception
    assert (pos * 128 == np.round(pos * 128)).all()
    p = pos[sc.triangles["v"]]
    lo, hi = p.min(axis=1), p.max(axis=1)
    assert ((hi - lo) == 0).any(axis=1).sum() >= 4 + 2 + 2 + 2                               # zero-thickness boxes: quads, walls, flat triangles
    area2 = np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    assert (area2 == 0).sum() == 2                                                          # collinear, two equal vertices
    assert (p[128:130] == p[130:132]).all()                                                 # the coincident quads
    assert (sc.materials["emittance"][sc.triangles["material"][128:132]] >= 0).all()
    h = pos[:(N + 1) ** 2, 1]
    assert set(np.unique(h * 4)) <= set(range(9)) and len(np.unique(h)) >= 5

    deck = case("deck").sc
    q = deck.vertices["position"][deck.triangles["v"]]
    assert len(deck.triangles) == 8192
    assert (q.min(axis=1) == q[0].min(axis=0)).all() and (q.max(axis=1) == q[0].max(axis=0)).all()       # every box is the same box
    assert (q[0::2] == q[0]).all() and (q[1::2] == q[1]).all()

    inst = case("instanced").sc
    assert len(inst.instances) == 6
    for rec in inst.instances:
        m, mi = (rec[k].astype(np.float64).reshape(4, 4).T for k in ("local_to_world", "world_to_local"))
        assert (m @ mi == np.eye(4)).all() and (np.abs(m[:3, :3]).sum(axis=0) == np.abs(m[:3, :3]).max(axis=0)).all()     # a scaled permutation
        assert set(np.abs(m[:3, :3]).reshape(-1)) <= {0.0, 0.5, 1.0, 2.0} and (m[:3, 3] == np.round(m[:3, 3])).all()
    assert (inst.instances[0]["local_to_world"] == inst.instances[1]["local_to_world"]).all()
    assert inst.instances[0]["first_triangle"] == inst.instances[1]["first_triangle"]


def test_grid_scene_is_the_terrain_at_400_cells():
    sc = case("grid").sc
    assert len(sc.triangles) == 2 * GRID_N * GRID_N + 11 == 320011
    pos = sc.vertices["position"].astype(np.float64)
    assert ((pos * 4 == np.round(pos * 4)).sum() == pos.size - 1) and pos.max() == GRID_N and pos.min() == 0.0


@pytest.mark.parametrize("name", ["terrain", "terrain23", "instanced", "deck", "grid"])
def test_families_are_not_degenerate(name):
    c = case(name)
    assert_family_not_degenerate(c, name)
    d = c.rows[:, 4:7]
    assert (np.signbit(d) & (d == 0)).any() and (~np.signbit(d) & (d == 0)).any()            # both zeros
    assert set(np.unique(np.abs(d[c.family == "axis_y"]).max(axis=1))) == {0.5, 1.0, 2.0}    # directions are not normalised
    assert len(c.rows) <= (520 if name == "grid" else 8192)
    cases = {t.split("/")[1] for t in c.tags if t.startswith("interval/")}
    assert cases == set(INTERVALS)
    assert {t for t in c.tags if t.startswith("diagonal/")} == {"diagonal/%g,%g,%g" % d for d in DIAGONALS}


# ---- CPU: the reference -----------------------------------------------------------------------------------------------------
def test_reference_equals_the_oracle_tree_on_rays_without_a_zero_component(oracle_rgb):
    """(a) Where no direction component is zero the oracle's tree trace (slr_oracle.cpp: BoundingBox3D::intersect + the same triangle
    test) and the brute force agree on every ray: triangle, distance bits, b0, b1, hit or miss.

    (c) Where a component IS zero they do not, and that is the oracle's slab test, not the reference: boxHit restates
    BoundingBox3D::intersect (Core/geometry.h:112-126: swap and compare), where a NaN slab product — direction (-0, -1, -0) from a
    point on the x = 0 plane — poisons the comparison and the box is skipped.  Measured on the 5 999 zero-component rays of this
    family: 440 hit / miss decisions and 61 distances differ, always in the same direction (the oracle misses triangles the
    triangle test accepts; it never hits where the brute force misses), and 50 more hits report another member of the tie set.
    Not asserted: boxHit restates the reference faithfully and stays as it is."""
    from oracle import binding as ob
    c = case("terrain")
    keep = (c.rows[:, 4:7] != 0).all(axis=1)
    assert keep.sum() >= 405
    rows, ref = c.rows[keep], c.ref
    rays = np.zeros(len(rows), ob.ray_dtype)
    rays["org"], rays["dir"], rays["dist_min"], rays["dist_max"] = rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7]
    got = oracle_rgb.scene(c.sc).trace(rays)
    hit, winner = ref.hit[keep], ref.winner[keep]
    assert ((got["triangle"] != MISS) == hit).all()
    assert 0.5 < hit.mean() < 1.0 and (ref.tie_size[keep] > 1).sum() >= 50
    assert (got["triangle"][hit] == ref.cand_tri[winner[hit]]).all()
    assert (bits(got["dist"][hit]) == bits(ref.tmin[keep][hit])).all()
    entry = _entries_of_winner(ref)[keep][hit]
    assert (bits(got["b0"][hit]) == bits(ref.tie_b0[entry])).all() and (bits(got["b1"][hit]) == bits(ref.tie_b1[entry])).all()


def _entries_of_winner(ref):
    """Per ray, the index of its winner among the tie entries (-1 on a miss)."""
    out = np.full(len(ref.hit), -1, np.int64)
    is_winner = ref.tie_cand == ref.winner[ref.tie_ray]
    out[ref.tie_ray[is_winner]] = np.nonzero(is_winner)[0]
    return out


def test_float64_evaluation_finds_the_inputs_free_of_rounding_ambiguity(capsys):
    """(b) The same formulas in float64 on the same (exact) inputs.  Accept / reject may differ only on the few rays that meet an
    edge exactly where 1 / det rounds (horizontal rays, det = 7 or 14): at most 1 % of the rays (measured: 22 of 6 532), and the
    accepted distances agree within 2 float32 ulp (measured: 1.14 ulp, 9.9e-8 relative).  Those rays STAY in the GPU tests: the
    float32 restatement is the law there."""
    c = case("terrain")
    a = brute_force_hits(c.sc, c.rows, keep_pairs=True)
    b = brute_force_hits(c.sc, c.rows, keep_pairs=True, dtype=np.float64)
    assert a.t.dtype == np.float32 and b.t.dtype == np.float64 and a.ok.shape == (len(c.rows), len(c.sc.triangles))
    ambiguous = (a.ok != b.ok).any(axis=1)
    both = a.ok & b.ok
    ulps = np.abs(a.t[both].astype(np.float64) - b.t[both]) / np.spacing(np.abs(a.t[both])).astype(np.float64)
    with capsys.disabled():
        print("\nfloat32 against float64: %d of %d rays have an ambiguous (ray, triangle) pair; accepted distances within %.3g ulp"
              % (ambiguous.sum(), len(c.rows), ulps.max()))
    assert ambiguous.sum() <= 0.01 * len(c.rows)
    assert both.sum() > 5000 and ulps.max() <= 2.0


def test_reference_interval_rules():
    """dist_max = t and dist_min = t keep the hit (the rule is `t < dist_min || t > dist_max` rejects), one ulp inside loses it."""
    c = case("terrain")
    ref, tags = c.ref, c.tags
    idx = {k: np.nonzero(tags == "interval/" + k)[0] for k in INTERVALS}
    n = len(idx["dmax=t"])
    assert n >= 289 and all(len(v) == n for v in idx.values())
    t = c.rows[idx["dmax=t"], 7]
    assert np.isfinite(t).all() and (t > 0).all() and (t * 8 == np.round(t * 8)).all()            # exact distances (det = +-1, +-2 or 16): heights interpolated at half-lattice points
    for k in ("dmax=t", "dmin=t", "dmin=dmax=t", "dmax=FLT_MAX", "dmin<0"):
        assert ref.hit[idx[k]].all() and (bits(ref.tmin[idx[k]]) == bits(t)).all(), k
        assert (ref.winner[idx[k]] == ref.winner[idx["dmax=t"]]).all() and (ref.tie_size[idx[k]] == ref.tie_size[idx["dmax=t"]]).all(), k
    assert not ref.hit[idx["dmax<t"]].any() and not ref.hit[idx["dmin>dmax"]].any()
    beyond = idx["dmin>t"]
    assert ref.hit[beyond].any() and (~ref.hit[beyond]).any() and (ref.tmin[beyond][ref.hit[beyond]] > t[ref.hit[beyond]]).all()


def test_reference_tie_rule_takes_the_largest_index():
    c = case("deck")
    hit = c.ref.hit
    assert hit.sum() > 500 and (c.ref.tie_size[hit] >= 4096).all()
    assert (c.ref.cand_tri[c.ref.winner[hit]] >= 8190).all()
    t = case("terrain")
    quads = _tie_set_inside(t.ref, 128, 132)
    assert quads.sum() >= 100 and (t.ref.cand_tri[t.ref.winner[quads]] >= 130).all()
    i = case("instanced")
    both = i.ref.hit & (i.ref.cand_inst[np.maximum(i.ref.winner, 0)] == 1)
    assert both.sum() > 1000 and not (i.ref.cand_inst[i.ref.winner[i.ref.hit]] == 0).any()      # placement 1 covers placement 0 exactly


def _tie_set_inside(ref, first, end):
    """Rays whose whole tie set lies in the triangles [first, end)."""
    inside = (ref.cand_tri[ref.tie_cand] >= first) & (ref.cand_tri[ref.tie_cand] < end)
    outside = np.bincount(ref.tie_ray[~inside], minlength=len(ref.hit))
    return ref.hit & (outside == 0)


def test_reference_gives_signed_zero_twins_the_same_answer():
    """The +0.0 and the -0.0 copy of an axis-parallel ray differ in no distance and no decision (only in the sign of a zero)."""
    c = case("terrain")
    for axis in "xyz":
        for sign in "+-":
            a, b = (np.nonzero(c.tags == "axis_%s/%s%s0" % (axis, sign, z))[0] for z in "+-")
            assert len(a) == len(b) >= 190 and (c.rows[a][:, :4] == c.rows[b][:, :4]).all() and (c.rows[a][:, 4:7] == c.rows[b][:, 4:7]).all()
            assert c.ref.hit[a].any() and (c.ref.hit[a] == c.ref.hit[b]).all()
            assert (c.ref.tmin[a] == c.ref.tmin[b]).all() and (c.ref.winner[a] == c.ref.winner[b]).all()
            assert (c.ref.tie_size[a] == c.ref.tie_size[b]).all()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def device_answers(ctx, rows):
    """The three entry points on the same rays: slrhip_trace_rays as slrhip_hit rows, slrhip_intersect_rays with instances,
    slrhip_test_visibility.  A non-zero query error word raises inside the binding; it is not caught."""
    tri, dist, b0, b1 = ctx.trace_rays(rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7])
    batch = np.zeros((len(rows), 4), np.float32)
    batch[:, 0], batch[:, 1], batch[:, 2], batch[:, 3] = tri.view(np.float32), dist, b0, b1
    hits, inst = ctx.intersect_rays(rows, want_instances=True)
    return batch, hits, inst, ctx.test_visibility(rows)


def assert_hits_equal_reference(ref, got, inst, what, exact=None):
    """Per ray, none exempted: hit or miss as the reference; on a hit the reported triangle (and instance, where `inst` is given)
    is a member of the tie set and dist, b0, b1 are bit-equal to the reference's values for that member — where the tie set has one
    member that is the whole record; on a miss the record is {MISS, inf, 0, 0} and the instance -1.  exact: rays on which the tie
    rule's winner is provable and the reported triangle (and instance) must be it."""
    tri = np.ascontiguousarray(got[:, 0]).view(np.uint32)
    miss = tri == MISS
    wrong = np.nonzero(miss == ref.hit)[0]
    assert len(wrong) == 0, "%s: hit / miss differs on %d of %d rays (first: ray %d)" % (what, len(wrong), len(miss), wrong[0])
    assert np.isposinf(got[miss, 1]).all() and (bits(got[miss, 2:4]) == 0).all(), what
    e_ray, e_tri, e_inst = ref.tie_ray, ref.cand_tri[ref.tie_cand], ref.cand_inst[ref.tie_cand]
    member = e_tri == tri[e_ray]
    if inst is not None:
        assert (inst[miss] == -1).all(), what
        member &= e_inst == inst[e_ray]
    outside = np.nonzero(ref.hit & (np.bincount(e_ray[member], minlength=len(miss)) == 0))[0]
    assert len(outside) == 0, "%s: %d rays report a triangle outside the tie set (first: ray %d, triangle %d)" % (what, len(outside), outside[0], tri[outside[0]])
    same = member & (bits(ref.tie_t) == bits(got[e_ray, 1])) & (bits(ref.tie_b0) == bits(got[e_ray, 2])) & (bits(ref.tie_b1) == bits(got[e_ray, 3]))
    bad = np.nonzero(ref.hit & (np.bincount(e_ray[same], minlength=len(miss)) == 0))[0]
    assert len(bad) == 0, "%s: dist / b0 / b1 differ in their bits on %d rays (first: ray %d, got %r)" % (what, len(bad), bad[0], got[bad[0]])
    if exact is not None:
        assert exact.any() and ref.hit[exact].all()
        assert (tri[exact] == ref.cand_tri[ref.winner[exact]]).all(), (what, "tie rule", int((tri[exact] != ref.cand_tri[ref.winner[exact]]).sum()))
        if inst is not None:
            assert (inst[exact] == ref.cand_inst[ref.winner[exact]]).all(), (what, "tie rule, instance")


# tree -> (case, config flags, the builder the summary of slrhip_debug_tree must name).  The device build takes scenes of at least
# 1 024 triangles: terrain_device_build runs on the 1 069-triangle terrain (on the 139-triangle one the flag is not honoured and the
# host build answers, which is what this entry tested, under this name, before the summary could tell).
TREES = {
    "terrain_host": ("terrain", 0, "host SAH"),
    "terrain_device_build": ("terrain23", abi.FLAG_BVH_DEVICE_BUILD, "device"),
    "terrain_spatial_splits": ("terrain", abi.FLAG_BVH_SPATIAL_SPLITS, "host spatial splits"),
    "instanced": ("instanced", 0, "instanced"),
    "deck_host": ("deck", 0, "host SAH"),
    "deck_device_build": ("deck", abi.FLAG_BVH_DEVICE_BUILD, "device"),
    "grid_quantized": ("grid", 0, "host SAH"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("tree", list(TREES))
def test_every_entry_point_equals_the_brute_force(tree):
    """k_trace_batch, the query kernel's closest-hit and any-hit (float, quantized and instanced nodes) against the brute force, ray for
    ray.  The exact tie rule is asserted where it is provable: on the deck (every box is the same box, every triangle is tested:
    the last layer wins, triangle >= 8 190) and on the terrain's rays whose tie set lies in the two coincident quads (identical
    boxes, t exact for det = 16: the second quad wins).  grid_quantized: 404 rays against 320 011 triangles, 1.1 s of brute force."""
    name, flags, builder = TREES[tree]
    c = case(name)
    assert_family_not_degenerate(c, tree)
    ctx = binding.Context(flags=flags)
    try:
        ctx.upload_scene(c.sc)          # both builders take the deck (host tree: 10 levels of four-wide nodes, up to 31 stack entries)
        assert ctx.debug_tree(summary_only=True)["builder_name"] == builder, tree
        if name == "grid":
            assert ctx.counters().bvh_nodes >= 65536          # the quantized tree
        batch, hits, inst, vis = device_answers(ctx, c.rows)
    finally:
        ctx.close()
    ref = c.ref
    exact = None
    if name == "deck":
        exact = ref.hit
        assert (ref.cand_tri[ref.winner[exact]] >= 8190).all()
    elif name in ("terrain", "terrain23"):
        quads = 2 * (N if name == "terrain" else N23) ** 2          # the two coincident quads follow the heightfield's triangles
        exact = _tie_set_inside(ref, quads, quads + 4)
    assert_hits_equal_reference(ref, batch, None, tree + " slrhip_trace_rays", exact)
    assert_hits_equal_reference(ref, hits, inst, tree + " slrhip_intersect_rays", exact)
    wrong = np.nonzero((vis != 0) == ref.hit)[0]
    assert len(wrong) == 0, "%s slrhip_test_visibility: %d of %d rays differ (first: ray %d)" % (tree, len(wrong), len(vis), wrong[0])
    assert set(np.unique(vis)) <= {0, 1}
    if len(c.sc.instances) == 0:
        assert (inst == -1).all()


PREFIXES = (1, 2, 63, 64, 65, 255, 257, 511, 512, 513, 4097)


@pytest.mark.gpu
def test_batch_shape_does_not_change_a_ray():
    """A ray's answer does not depend on the batch around it: prefixes of the terrain family that end inside a wave, a 128-ray
    producer chunk and the ray ring, and one deep deck ray among 4 096 immediate misses (the refill threshold), each bit-identical
    to the same rows inside the full batch.  Default tree, slrhip_intersect_rays and slrhip_test_visibility."""
    c = case("terrain")
    ctx = binding.Context()
    try:
        ctx.upload_scene(c.sc)
        full_hits, full_inst = ctx.intersect_rays(c.rows, want_instances=True)
        full_vis = ctx.test_visibility(c.rows)
        assert_hits_equal_reference(c.ref, full_hits, full_inst, "full batch")
        for n in PREFIXES:
            take = np.arange(n) % len(c.rows)                  # the family repeated as needed
            hits, inst = ctx.intersect_rays(c.rows[take], want_instances=True)
            vis = ctx.test_visibility(c.rows[take])
            assert hits.shape == (n, 4) and vis.shape == (n,)
            assert (hits.view(np.uint32) == full_hits[take].view(np.uint32)).all(), n
            assert (inst == full_inst[take]).all() and (vis == full_vis[take]).all(), n
    finally:
        ctx.close()

    d = case("deck")
    deep = int(np.nonzero((d.tags == "axis_y/-+0") & d.ref.hit)[0][0])
    away = ray_rows(np.tile([2.0, 9.0, 2.0], (4096, 1)), np.tile([0.0, 1.0, 0.0], (4096, 1)), 0.0, np.inf)      # above the deck, going up
    rows = np.concatenate([away[:2048], d.rows[deep:deep + 1], away[2048:]])
    ctx = binding.Context()
    try:
        ctx.upload_scene(d.sc)
        full_hits = ctx.intersect_rays(d.rows)
        full_vis = ctx.test_visibility(d.rows)
        hits, vis = ctx.intersect_rays(rows), ctx.test_visibility(rows)
    finally:
        ctx.close()
    assert (hits[2048].view(np.uint32) == full_hits[deep].view(np.uint32)).all() and vis[2048] == full_vis[deep] == 0
    assert hits[2048, 0].view(np.uint32) >= 8190 and hits[2048, 1] == d.ref.tmin[deep]
    others = np.arange(len(rows)) != 2048
    assert (hits[others, 0].view(np.uint32) == MISS).all() and (vis[others] == 1).all()
