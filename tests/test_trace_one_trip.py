"""The wave-specialised consumer (wsConsume, pt_trace_ws.h) fixes the kind of a lane's step — one node or ONE triangle — at the start of
the turn and fetches either with the same three loads: a lane that arrives at a leaf tests its first triangle in its
NEXT turn.  That is the schedule of float trees without instances; quantized and instanced trees keep the step that chains (the choice is
by tree class, measured).  Under either a ray visits the same nodes and tests the same triangles in the same order, so nothing a caller can
read may move.

Host: the compiler's resource remarks of every kernel that holds the consumer — at most 64 VGPRs, 8 waves per SIMD, and no more
scratch than the same instantiation had before the change (tests/golden/ws_one_trip_parent_kernels.json, from the parent commit by
the same command).

GPU: slrhip_intersect_rays and slrhip_test_visibility (k_ring_ws, the consumer) against slrhip_trace_rays (k_trace_batch: traverse(),
untouched) bit for bit and against helpers.brute_force_hits, on trees small enough to aim at single steps: `fans` are groups of up to
four triangles that share ONE bounding box (the four halves of a tilted unit square), which no builder can separate, so a group is a
leaf packet of known size; on the deck, an instanced scene whose meshes are single packets, the quantized grid, and batch shapes
around the wave and the refill threshold.  Traversal totals of counting contexts equal the parent library's
(tests/golden/ws_one_trip_parent_counts.json, recorded by running the parent commit's library on the inputs of count_case below);
frames equal the oracle as the parity suite defines it."""
import functools
import json
import os

import numpy as np
import pytest

from helpers import GOLDEN, assert_bit_equal, brute_force_hits, libm_tolerance, ray_rows
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes
from test_gpu_parity import TOL
from test_shade_occupancy import HIPCC, resource_remarks
from test_traversal_edges import assert_hits_equal_reference, case, device_answers

MISS = abi.MISS
PARENT_KERNELS = os.path.join(GOLDEN, "ws_one_trip_parent_kernels.json")
PARENT_COUNTS = os.path.join(GOLDEN, "ws_one_trip_parent_counts.json")


# ---- host: registers, scratch, occupancy ----------------------------------------------------------------------------------------
@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
@pytest.mark.parametrize("source", ["pt_trace_ws.hip", "pt_trace_indexed.hip"])
def test_consumer_kernels_keep_their_registers_and_scratch(source, tmp_path):
    want = json.load(open(PARENT_KERNELS))[source]
    got = resource_remarks(source, tmp_path)
    assert sorted(got) == sorted(want)
    assert len(got) == {"pt_trace_ws.hip": 18, "pt_trace_indexed.hip": 36}[source]          # every one of them holds wsConsume
    for name in sorted(want):
        r, p = got[name], want[name]
        print(name, "VGPRs %d (parent %d), scratch %d (parent %d), waves %d" % (r["VGPRs"], p["VGPRs"], r["ScratchSize"], p["ScratchSize"], r["Occupancy"]))
        assert r["VGPRs"] <= 64 and r["AGPRs"] == 0, (name, r)
        assert r["Occupancy"] == 8, (name, r)
        assert r["ScratchSize"] <= p["ScratchSize"], (name, r["ScratchSize"], p["ScratchSize"])


# ---- scenes whose leaf packets are known ----------------------------------------------------------------------------------------
HALVES = ((0, 1, 2), (1, 2, 3), (2, 3, 0), (3, 0, 1))       # of the square A B C D: v <= u, u + v >= 1, v >= u, u + v <= 1
# group -> which half each of its triangles is, in scene order.  Packets of 1, 2, 3 and 4; the 4-packets put the odd half first, second
# and last, so that a ray through the part of the square only the odd half covers is accepted by that member alone.
ONE_NODE = ((0,), (0, 2), (0, 2, 0), (0, 0, 0, 2))
TWO_LEVELS = ((0, 0, 0, 2), (2, 0, 2, 2), (0, 2, 0, 0), (0, 1, 2, 3), (3, 2, 1, 0), (0, 2, 0), (0, 2), (0,))
PITCH = 2.0


def fans(groups, name, instanced=False):
    """Group g: the halves groups[g] of the square A = (x, 1, 0), B = (x + 1, 1, 0), C = (x + 1, 2, 1), D = (x, 2, 1), x = PITCH * g — one
    plane (y = 1 + z), one bounding box [x, x + 1] x [1, 2] x [0, 1] for every half.  instanced: the groups are meshes at x = 0, each
    placed at its x by a translation (exact), after a loose emitter."""
    b = scenes.SceneBuilder()
    grey = b.matte(b.spectrum_grey(0.5))
    light = b.matte(b.spectrum_grey(0.8), emittance=b.spectrum_d65(1.0, scenes.D65_RGB))
    if instanced:
        b.add_quad([(0, 8, 0), (1, 8, 0), (1, 8, 1), (0, 8, 1)], (0, -1, 0), (1, 0, 0), light)
    for g, halves in enumerate(groups):
        x = 0.0 if instanced else PITCH * g
        corners = [(x, 1, 0), (x + 1, 1, 0), (x + 1, 2, 1), (x, 2, 1)]
        first = b.num_triangles()
        for j, h in enumerate(halves):
            b.add_mesh([corners[k] for k in HALVES[h]], [(0, 1, 0)] * 3, [(1, 0, 0)] * 3, [(0, 0), (1, 0), (0, 1)], [(0, 1, 2)],
                       light if g == 0 and j == 0 and not instanced else grey)
        if instanced:
            m = np.eye(4)
            m[0, 3] = PITCH * g
            b.add_instance(first, len(halves), m)
    return b.build(scenes._lattice_camera(4), name=name)


def fan_rays(groups):
    """Per group: rays straight down and slanted through a 7 x 7 lattice of the square (eighths: every (u, v) class of the halves, the
    diagonals included), closest-hit intervals and intervals that end before or begin after the plane; rays along +x through EVERY
    group's box that miss the plane (leaves popped one after the other, nothing accepted), rays that descend along +x and hit one
    group behind others, and rays that miss the root."""
    rows = []
    k = np.arange(1, 8) / 8.0
    u, v = (a.reshape(-1) for a in np.meshgrid(k, k, indexing="ij"))
    for g in range(len(groups)):
        x = PITCH * g
        p = np.stack([x + u, 1.0 + v, v], axis=1)                          # points of the plane y = 1 + z
        for d in ((0, -1, 0), (0.5, -1, 0.25), (-1, -2, 1), (0, 1, 0)):
            d = np.array(d, np.float64)
            rows.append(ray_rows(p - 2.0 * d, np.tile(d, (len(p), 1)), 0.0, np.inf))          # the plane at t = 2
        d = np.array((0, -1, 0), np.float64)
        rows.append(ray_rows(p - 2.0 * d, np.tile(d, (len(p), 1)), 0.0, 1.5))                  # ends before the plane
        rows.append(ray_rows(p - 2.0 * d, np.tile(d, (len(p), 1)), 2.5, np.inf))               # begins behind it
    span = PITCH * len(groups)
    z = np.array([0.125, 0.375, 0.5, 0.875])
    for y in (1.0625, 1.25, 1.75):                                           # through every box, beside the plane (y != 1 + z)
        zz = z[np.abs(1.0 + z - y) > 1e-6]
        rows.append(ray_rows(np.stack([np.full(len(zz), -1.0), np.full(len(zz), y), zz], axis=1), np.tile([1.0, 0.0, 0.0], (len(zz), 1)), 0.0, np.inf))
        rows.append(ray_rows(np.stack([np.full(len(zz), span + 1.0), np.full(len(zz), y), zz], axis=1), np.tile([-1.0, 0.0, 0.0], (len(zz), 1)), 0.0, np.inf))
    for slope in (0.0625, 0.125, 0.25):                                      # descending along +x and -x: through boxes, then a hit
        rows.append(ray_rows(np.stack([np.full(4, -1.0), np.full(4, 2.5), z], axis=1), np.tile([1.0, -slope, 0.0], (4, 1)), 0.0, np.inf))
        rows.append(ray_rows(np.stack([np.full(4, span + 1.0), np.full(4, 2.5), z], axis=1), np.tile([-1.0, -slope, 0.0], (4, 1)), 0.0, np.inf))
    rows.append(ray_rows(np.tile([0.5, 5.0, 0.5], (8, 1)), np.tile([0.0, 1.0, 0.0], (8, 1)), 0.0, np.inf))        # miss the root
    rows.append(ray_rows(np.tile([-3.0, 1.5, 0.5], (8, 1)), np.tile([-1.0, 0.25, 0.5], (8, 1)), 0.0, np.inf))
    return np.concatenate(rows)


def leaf_packets(tree):
    """[(node, first LeafTri, count)] of the packets a tree's nodes reference."""
    out = []
    for i, n in enumerate(tree["nodes"]):
        for c in n["child"]:
            c = int(c)
            count = (c >> abi.LEAF_COUNT_SHIFT) & 0xF
            if c != abi.INVALID_CHILD and c & abi.LEAF_FLAG and count not in (0, 15):
                out.append((i, c & abi.LEAF_INDEX_MASK, count))
    return out


class Fan:
    def __init__(self, groups, name, instanced=False):
        self.sc = fans(groups, name, instanced)
        self.rows = fan_rays(groups)
        self.ref = brute_force_hits(self.sc, self.rows, keep_pairs=True)
        self.tree = binding.host_tree(self.sc)
        for a in (self.rows,) + tuple(v for v in vars(self.ref).values() if isinstance(v, np.ndarray)):
            a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def fan(which):
    if which == "one node":
        return Fan(ONE_NODE, "fans_one_node")
    if which == "two levels":
        return Fan(TWO_LEVELS, "fans_two_levels")
    return Fan(ONE_NODE + ((2, 0, 2, 2),), "fans_instanced", instanced=True)


def first_acceptor(f):
    """Per ray and packet of 4: the position inside the packet of the first member (in the order the consumer tests them) that accepts
    the ray — what ends an any-hit ray — or -1.  From the brute force's per-pair verdicts; loose triangles only."""
    tri_of = f.tree["leaf_tris"]["tri"]
    cand = {int(t): k for k, t in enumerate(f.ref.cand_tri)}
    out = {}
    for _, first, count in leaf_packets(f.tree):
        if count == 4:
            ok = np.stack([f.ref.ok[:, cand[int(tri_of[first + j])]] for j in range(4)], axis=1)
            out[first] = np.where(ok.any(axis=1), ok.argmax(axis=1), -1)
    return out


def test_fan_trees_have_the_shapes_the_cases_aim_at():
    one, two, inst = fan("one node"), fan("two levels"), fan("instanced")
    assert one.tree["num_nodes"] == 1 and sorted(c for _, _, c in leaf_packets(one.tree)) == [1, 2, 3, 4]
    assert two.tree["depth"] == 2 and two.tree["num_nodes"] > 1
    assert sorted(c for _, _, c in leaf_packets(two.tree)) == sorted(len(g) for g in TWO_LEVELS)
    # every inner node of the two-level tree below the root holds packets only: a node step there ends on a leaf or pops one
    assert all((int(c) == abi.INVALID_CHILD or int(c) & abi.LEAF_FLAG) for n in two.tree["nodes"][1:] for c in n["child"])
    # any-hit rays accepted by the 1st, the 2nd and the last member of a 4-packet, and 4-packets that accept nothing
    for f in (one, two):
        seen = set()
        for pos in first_acceptor(f).values():
            seen |= set(int(p) for p in np.unique(pos))
        assert {-1, 0, 3} <= seen, seen
    assert 1 in set(int(p) for pos in first_acceptor(two).values() for p in np.unique(pos))
    # the instanced scene: every mesh is ONE packet under a root of its own — the instance's root leads straight to a leaf
    assert inst.tree["builder_name"] == "instanced" and inst.tree["num_instances"] == len(ONE_NODE) + 1
    for rec in inst.tree["instances"]:
        kids = [int(c) for c in inst.tree["nodes"][int(rec["root"])]["child"] if int(c) != abi.INVALID_CHILD]
        assert len(kids) == 1 and kids[0] & abi.LEAF_FLAG and (kids[0] >> abi.LEAF_COUNT_SHIFT) & 0xF == int(rec["num_triangles"])
    for f in (one, two, inst):
        share = f.ref.hit.mean()
        assert 0.3 <= share <= 0.9, share                                   # rays that miss everything, rays that hit
        assert (f.ref.tie_size[f.ref.hit] > 1).any()                        # coincident halves tie: the largest index must win


def same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def check_against_batch_and_brute_force(sc, rows, ref, what, flags=0, quantized=False):
    ctx = binding.Context(flags=flags)
    try:
        ctx.upload_scene(sc)
        if quantized:
            assert ctx.counters().bvh_nodes >= 65536
        batch, hits, inst, vis = device_answers(ctx, rows)
    finally:
        ctx.close()
    assert same_bits(hits, batch), "%s: slrhip_intersect_rays differs from slrhip_trace_rays on %d rays" % (
        what, int((hits.view(np.uint32) != batch.view(np.uint32)).any(axis=1).sum()))
    assert_hits_equal_reference(ref, hits, inst, what + " slrhip_intersect_rays")
    assert ((vis != 0) != ref.hit).all(), "%s slrhip_test_visibility: %d rays differ" % (what, int(((vis != 0) == ref.hit).sum()))
    return hits, inst, vis


# ---- GPU: single steps ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one node", "two levels", "instanced"])
def test_fans(which):
    """One node over packets of 1, 2, 3 and 4 (a ray's first node step ends on a leaf; the other packets come off the stack; a ray
    that misses every member pops the next); two levels (a node comes off the stack after a leaf); meshes that are one packet each."""
    f = fan(which)
    hits, inst, _ = check_against_batch_and_brute_force(f.sc, f.rows, f.ref, "fans, " + which)
    # coincident halves: the winner of a tie is the largest (instance, triangle) pair, in every bit of the record
    tied = f.ref.hit & (f.ref.tie_size > 1)
    assert (hits[tied, 0].view(np.uint32) == f.ref.cand_tri[f.ref.winner[tied]]).all()
    if which == "instanced":
        assert (inst[tied] == f.ref.cand_inst[f.ref.winner[tied]]).all()
        assert (inst[f.ref.hit] >= 0).sum() >= 100 and (inst[f.ref.hit] == -1).any()          # (the loose emitter above the fans)


@pytest.mark.gpu
def test_deck_64_rays():
    """Ten levels, every child of every node entered, the stack into its scratch part: 64 rays of the deck's family, hits and misses."""
    d = case("deck")
    hit, miss = np.nonzero(d.ref.hit)[0], np.nonzero(~d.ref.hit)[0]
    take = np.sort(np.concatenate([hit[np.linspace(0, len(hit) - 1, 48).astype(int)], miss[np.linspace(0, len(miss) - 1, 16).astype(int)]]))
    assert len(np.unique(take)) == 64
    rows = d.rows[take]
    ref = brute_force_hits(d.sc, rows)
    hits, _, _ = check_against_batch_and_brute_force(d.sc, rows, ref, "deck, 64 rays")
    assert (hits[ref.hit, 0].view(np.uint32) >= 8190).all()                 # every layer ties: the last one wins


@pytest.mark.gpu
def test_quantized_grid_404_rays():
    g = case("grid")
    assert len(g.rows) == 404
    check_against_batch_and_brute_force(g.sc, g.rows, g.ref, "quantized grid", quantized=True)


@pytest.mark.gpu
def test_batch_shapes_around_the_wave_and_the_refill_threshold():
    """1, 63, 64, 65, 129 and 4 097 rays: a deep deck ray in the middle of immediate misses, each row bit-equal to its row in the
    full batch."""
    d = case("deck")
    deep = int(np.nonzero((d.tags == "axis_y/-+0") & d.ref.hit)[0][0])
    full = np.concatenate([d.rows, fan_rays(((0,),))])                       # the deck's family and rays that have nothing to do with it
    away = ray_rows([[2.0, 9.0, 2.0]], [[0.0, 1.0, 0.0]], 0.0, np.inf)      # above the deck, going up
    ctx = binding.Context()
    try:
        ctx.upload_scene(d.sc)
        full_hits, full_vis = ctx.intersect_rays(full), ctx.test_visibility(full)
        assert full_hits[deep, 0].view(np.uint32) >= 8190 and full_vis[deep] == 0
        for n in (1, 63, 64, 65, 129, 4097):
            at = n // 2
            rows = np.repeat(away, n, axis=0)
            rows[at] = d.rows[deep]
            hits, vis = ctx.intersect_rays(rows), ctx.test_visibility(rows)
            assert hits.shape == (n, 4) and vis.shape == (n,)
            assert same_bits(hits[at], full_hits[deep]) and vis[at] == 0, n
            others = np.arange(n) != at
            assert (hits[others, 0].view(np.uint32) == MISS).all() and (vis[others] == 1).all(), n
            take = np.arange(n) % len(full)                                  # and a prefix of the full batch, repeated as needed
            hits, vis = ctx.intersect_rays(full[take]), ctx.test_visibility(full[take])
            assert same_bits(hits, full_hits[take]) and (vis == full_vis[take]).all(), n
    finally:
        ctx.close()


# ---- GPU: step counts -------------------------------------------------------------------------------------------------------------
COUNT_CASES = {"spheres": (lambda: scenes.cornell_box_spheres(64 / 36, 8, 4, "matte"), 64, 36, 8, 61),
               "box": (lambda: scenes.tiny_box(48 / 36), 48, 36, 4, 62)}


def count_case(name):
    """The traversal totals and the ray counters of one render in a counting context: what the parent's figures were recorded with."""
    make, w, h, spp, seed = COUNT_CASES[name]
    c = Context(flags=abi.FLAG_COUNT_TRAVERSAL)
    try:
        c.render_image(make(), ob.settings(w, h, seed=seed), spp)
        p, k = c.profile(), c.counters()
        return {"nodes": [int(v) for v in p.nodes], "triangles": [int(v) for v in p.triangles], "rays": [int(v) for v in p.rays],
                "samples": int(k.samples), "extension_rays": int(k.extension_rays), "shadow_rays": int(k.shadow_rays)}
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COUNT_CASES))
def test_traversal_totals_equal_the_parents(name):
    want = json.load(open(PARENT_COUNTS))[name]
    got = count_case(name)
    print(name, got)
    assert min(want["nodes"] + want["triangles"]) > 0 and want["samples"] == COUNT_CASES[name][1] * COUNT_CASES[name][2] * COUNT_CASES[name][3]
    assert got == want


# ---- GPU: frames ------------------------------------------------------------------------------------------------------------------
def frame(sc, st, spp, **kw):
    c = Context(**kw)
    try:
        fb = c.render_image(sc, st, spp)
        k = c.counters()
        return fb, (int(k.extension_rays), int(k.shadow_rays))
    finally:
        c.close()


@pytest.mark.gpu
def test_frames_equal_the_oracle(oracle_rgb):
    """Lambert + mirror and the instanced box (no float libm on a path): every bit and both ray counts; Ward lobes: the parity suite's
    tolerance for them, and every bit of the frame the tail kernel (traverse()) renders."""
    for what, sc, st, spp in (("spheres 64 x 36 x 64", scenes.cornell_box_spheres(64 / 36, 8, 4, "matte"), ob.settings(64, 36, seed=63), 64),
                              ("instanced 48 x 36 x 8", scenes.cornell_instanced(48 / 36, 10, 5), ob.settings(48, 36, seed=64), 8)):
        want, ctr = oracle_rgb.scene(sc).render(st, spp)
        fb, rays = frame(sc, st, spp)
        assert rays == (int(ctr.extension_rays), int(ctr.shadow_rays)), (what, rays)
        assert_bit_equal(fb, want, what + " vs the oracle")
    sc, st = scenes.cornell_lobes("ward", 48 / 36, segments=8, rings=4), ob.settings(48, 36, seed=65)
    want, _ = oracle_rgb.scene(sc).render(st, 8)
    fb, rays = frame(sc, st, 8, stripes=1)
    tail, tail_rays = frame(sc, st, 8, stripes=1, flags=abi.FLAG_TAIL_KERNEL)
    assert rays == tail_rays
    assert_bit_equal(fb, tail, "ward 48 x 36 x 8: wavefront iterations vs the tail kernel")
    libm_tolerance(fb, want, "ward 48 x 36 x 8 vs oracle", within=TOL["rgb_ward"])
