"""A validator for the trees the upload builds (slrhip_debug_tree / slrhip_debug_host_tree; slr_amd.binding._read_tree's dict): the
structure, the float boxes, the quantized boxes and the leaf records, checked against the scene alone — no ray is traced.  Vectorised
numpy, level by level; a violated rule raises TreeError, whose `rule` names it (the RULES below)."""
from fractions import Fraction

import numpy as np

from slr_amd import abi

RULES = ("root", "child_range", "child_order", "reach_once", "depth", "stack", "empty_slot", "slot_order", "leaf_count", "leaf_range",
         "leaf_cover", "leaf_tri_range", "tri_once", "references", "instance_once", "mesh_range", "leaf_tri_record", "leaf_box", "inner_box",
         "instance_box", "split_inner_box", "split_vertex", "q_child", "q_empty", "q_contain", "q_loose")
# q_loose: how many steps inwards a quantized plane may be moved at most before the UNROUNDED plane origin + q * scale leaves the float
# box behind.  quantizeNodes takes l = floor((lo - origin) / scale) in float32: the subtraction and the division round once each, a
# relative error below 2^-22 on a quotient of at most 255, so l >= l* - 1 for the exact l*; its correction loop lowers l only where the
# ROUNDED plane lies above lo, which (rounding is monotone) cannot happen for l <= l*.  So l >= l* - 1 and the exact plane of l + 2 >=
# l* + 1 lies strictly above lo; the same for h from above.  On the rounded plane no such bound exists: with a large origin and a small
# extent the planes form a staircase (scale below one ulp of the origin), where dozens of steps give the same float.
LOOSE_STEPS = 2


class TreeError(AssertionError):
    def __init__(self, rule, message):
        assert rule in RULES, rule
        super().__init__("[%s] %s" % (rule, message))
        self.rule = rule


def _fail_if(mask, rule, what):
    mask = np.asarray(mask)
    if mask.any():
        where = np.argwhere(mask)
        raise TreeError(rule, "%s (%d places, first at %s)" % (what, len(where), tuple(int(v) for v in where[0])))


def fma_f32(q, scale, origin):
    """fma(q, scale, origin) in float32 with ONE rounding, as the traversal evaluates a quantized plane: q * scale is exact in float64
    (8 + 24 bits); the float64 sum with the origin rounds to 53 bits, and rounding that again to float32 is wrong only where it lies
    exactly on a float32 rounding boundary (a midpoint of two neighbours) — those planes are redone in exact rational arithmetic.
    Returns (planes float32, number redone)."""
    q, scale, origin = np.broadcast_arrays(np.asarray(q, np.float64), np.asarray(scale, np.float32), np.asarray(origin, np.float32))
    total = q * scale.astype(np.float64) + origin.astype(np.float64)
    with np.errstate(over="ignore"):
        r = total.astype(np.float32)
    d = total - r.astype(np.float64)                                              # exact: both are multiples of total's last place
    other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    with np.errstate(invalid="ignore"):
        half = (other.astype(np.float64) - r.astype(np.float64)) * 0.5
        boundary = np.isfinite(total) & (d != 0) & (d == half)
    out = r.copy()
    for idx in zip(*np.nonzero(boundary)):
        exact = Fraction(float(q[idx])) * Fraction(float(scale[idx])) + Fraction(float(origin[idx]))
        a, b = r[idx], other[idx]
        mid = (Fraction(float(a)) + Fraction(float(b))) / 2
        if exact == mid:
            out[idx] = a if (a.view(np.uint32) & 1) == 0 else b                    # ties to even
        else:
            out[idx] = a if (abs(exact - Fraction(float(a))) < abs(exact - Fraction(float(b)))) else b
    return out, int(boundary.sum())


def check_quantized(nodes, nodes_q, loose_steps=LOOSE_STEPS, stats=None):
    """The quantized records of `nodes`: child words copied, empty slots 255 / 0, every dequantized box (single-rounded planes) contains
    the float box, and no plane is looser than `loose_steps` (see LOOSE_STEPS; a plane that cannot move that far inside 0 .. 255, and an
    axis of scale 0, are exempt)."""
    if len(nodes_q) != len(nodes):
        raise TreeError("q_child", "%d quantized nodes for %d nodes" % (len(nodes_q), len(nodes)))
    _fail_if(nodes_q["child"] != nodes["child"], "q_child", "child word differs from the float node's")
    valid = (nodes["child"] != abi.INVALID_CHILD)[:, None, :]                       # [node, axis, child]
    qlo, qhi = nodes_q["qlo"], nodes_q["qhi"]
    _fail_if(~valid & ((qlo != 255) | (qhi != 0)), "q_empty", "empty slot not encoded as 255 / 0")
    scale, origin = nodes_q["scale"][:, :, None], nodes_q["origin"][:, :, None]
    plo, n1 = fma_f32(qlo, scale, origin)
    phi, n2 = fma_f32(qhi, scale, origin)
    if stats is not None:
        stats["planes_redone_exactly"] = stats.get("planes_redone_exactly", 0) + n1 + n2
    _fail_if(valid & ~(plo <= nodes["lo"]), "q_contain", "dequantized lower plane above the float box")
    _fail_if(valid & ~(phi >= nodes["hi"]), "q_contain", "dequantized upper plane below the float box")
    # looseness on the unrounded plane (float64: q * scale exact, the sum within 2^-53)
    s64, o64 = scale.astype(np.float64), origin.astype(np.float64)
    movable = valid & (scale > 0)
    lo_in = (qlo.astype(np.float64) + loose_steps) * s64 + o64
    hi_in = (qhi.astype(np.float64) - loose_steps) * s64 + o64
    _fail_if(movable & (qlo.astype(np.int32) + loose_steps <= 255) & ~(lo_in > nodes["lo"]), "q_loose",
             "lower plane still inside the box %d steps further in" % loose_steps)
    _fail_if(movable & (qhi.astype(np.int32) - loose_steps >= 0) & ~(hi_in < nodes["hi"]), "q_loose",
             "upper plane still inside the box %d steps further in" % loose_steps)


def loosest_steps(nodes, nodes_q, rounded=False, limit=256):
    """Measurement behind LOOSE_STEPS: the largest number of steps any movable plane of `nodes_q` can go inwards and still contain its
    float plane, plus one (= the smallest loose_steps check_quantized would accept); on the unrounded planes, or the rounded ones."""
    valid = (nodes["child"] != abi.INVALID_CHILD)[:, None, :] & (nodes_q["scale"][:, :, None] > 0)
    scale, origin = nodes_q["scale"][:, :, None], nodes_q["origin"][:, :, None]
    worst, pending_lo, pending_hi = 0, valid.copy(), valid.copy()
    for k in range(1, limit):
        ql, qh = nodes_q["qlo"].astype(np.int32) + k, nodes_q["qhi"].astype(np.int32) - k
        if rounded:
            lo_in, hi_in = fma_f32(np.minimum(ql, 255), scale, origin)[0], fma_f32(np.maximum(qh, 0), scale, origin)[0]
        else:
            lo_in = ql * scale.astype(np.float64) + origin.astype(np.float64)
            hi_in = qh * scale.astype(np.float64) + origin.astype(np.float64)
        pending_lo &= (ql <= 255) & (lo_in <= nodes["lo"])
        pending_hi &= (qh >= 0) & (hi_in >= nodes["hi"])
        if not (pending_lo.any() or pending_hi.any()):
            return k
        worst = k
    return worst + 1


class _Walk:
    """One tree inside the node array, walked level by level from `root`."""

    def __init__(self, nodes, root, num_nodes):
        self.levels = []                                     # node indices per level
        frontier = np.array([root], np.int64)
        while len(frontier):
            self.levels.append(frontier)
            child = nodes["child"][frontier]
            inner = (child != abi.INVALID_CHILD) & ((child & abi.LEAF_FLAG) == 0)
            _fail_if(inner & (child >= num_nodes), "child_range", "inner child index beyond the node array")
            _fail_if(inner & (child <= frontier[:, None]), "child_order", "inner child index not larger than its parent's")
            frontier = child[inner].astype(np.int64)
            if len(self.levels) > 64:
                raise TreeError("stack", "more than 64 levels")
        self.visited = np.concatenate(self.levels)


def _tri_boxes(scene):
    p = scene.vertices["position"][scene.triangles["v"]]              # [tri, vertex, axis] float32
    return p, p.min(axis=1), p.max(axis=1)


def check_tree(tree, scene, spatial_splits=False, loose_steps=LOOSE_STEPS, stats=None):
    """Every rule of this module on `tree` (a read-out's dict) against `scene` (an abi.Scene).  spatial_splits: the tree may reference a
    triangle more than once with clipped boxes.  No rule is dropped for any builder: in particular no builder puts a valid slot behind
    an empty one."""
    nodes, leaf_tris = tree["nodes"], tree["leaf_tris"]
    num_nodes, num_leaf, num_tris, num_inst = len(nodes), len(leaf_tris), len(scene.triangles), len(scene.instances)
    if num_nodes == 0 or tree["num_nodes"] != num_nodes or tree["num_triangles"] != num_tris or tree["leaf_references"] != num_leaf:
        raise TreeError("root", "summary and arrays disagree, or no node")
    child = nodes["child"]
    valid = child != abi.INVALID_CHILD
    leaf = valid & ((child & abi.LEAF_FLAG) != 0)
    count = (child >> abi.LEAF_COUNT_SHIFT) & 0xF
    first = (child & abi.LEAF_INDEX_MASK).astype(np.int64)
    is_inst = leaf & (count == 0)
    is_packet = leaf & (count != 0)

    # ---- shape ----
    top = _Walk(nodes, 0, num_nodes)
    walks, depth = [top], len(top.levels)
    instanced = num_inst > 0
    roots = np.zeros(0, np.int64)
    if instanced:
        if len(tree["instances"]) != num_inst or tree["num_instances"] != num_inst:
            raise TreeError("root", "instance records and scene disagree")
        roots = np.unique(tree["instances"]["root"].astype(np.int64))
        _fail_if(roots >= num_nodes, "child_range", "instance root beyond the node array")
        mesh_walks = [_Walk(nodes, int(r), num_nodes) for r in roots]
        walks += mesh_walks
        depth += 1 + max(len(w.levels) for w in mesh_walks)
        if tree["top_nodes"] != len(top.visited):
            raise TreeError("reach_once", "the top level reaches %d nodes, the summary says %d" % (len(top.visited), tree["top_nodes"]))
    visited = np.concatenate([w.visited for w in walks])
    reached = np.bincount(visited, minlength=num_nodes)
    _fail_if(reached != 1, "reach_once", "node not reached exactly once from the root" + ("s" if instanced else ""))
    if depth != tree["depth"]:
        raise TreeError("depth", "%d levels, the summary reports %d" % (depth, tree["depth"]))
    if 3 * depth + 1 > 64:
        raise TreeError("stack", "3 * %d + 1 entries exceed the 64-entry traversal stack" % depth)

    # ---- empty slots ----
    _fail_if(~valid[:, None, :] & ~(np.isposinf(nodes["lo"]) & np.isneginf(nodes["hi"])), "empty_slot", "empty slot without the inverted box")
    _fail_if(valid[:, 1:] & ~valid[:, :-1], "slot_order", "valid slot behind an empty one")

    # ---- leaves ----
    in_top = np.zeros(num_nodes, bool)
    in_top[top.visited] = True
    _fail_if(leaf & (count > abi.MAX_LEAF_TRIS), "leaf_count", "leaf count beyond kMaxLeafTris")
    _fail_if(is_inst & ~(instanced & in_top)[:, None], "leaf_count", "leaf count 0 outside an instanced top level")
    _fail_if(is_inst & (first >= max(num_inst, 0)), "leaf_count", "instance index out of range")
    _fail_if(is_packet & (first + count > num_leaf), "leaf_range", "leaf packet beyond the LeafTri array")
    pn, pc = np.nonzero(is_packet)
    order = np.argsort(first[pn, pc], kind="stable")
    pn, pc = pn[order], pc[order]
    pfirst, pcount = first[pn, pc], count[pn, pc].astype(np.int64)
    ends = pfirst + pcount
    if num_leaf and (len(pfirst) == 0 or pfirst[0] != 0 or ends[-1] != num_leaf or (pfirst[1:] != ends[:-1]).any()):
        bad = np.nonzero(pfirst[1:] != ends[:-1])[0]
        raise TreeError("leaf_cover", "leaf packets overlap or leave LeafTri records out (%d packets, first break after packet %s)"
                        % (len(pfirst), int(bad[0]) if len(bad) else "none: the ends"))
    if num_leaf == 0 and len(pfirst):
        raise TreeError("leaf_cover", "packets without LeafTri records")
    tri = leaf_tris["tri"].astype(np.int64)
    _fail_if(tri >= num_tris, "leaf_tri_range", "LeafTri.tri beyond the triangle count")
    refs = np.bincount(tri, minlength=num_tris)
    if spatial_splits:
        _fail_if(refs < 1, "tri_once", "triangle referenced by no leaf")
    else:
        _fail_if(refs != 1, "tri_once", "triangle not referenced exactly once")
    if int(refs.sum()) != tree["leaf_references"]:
        raise TreeError("references", "%d references, the summary reports %d" % (refs.sum(), tree["leaf_references"]))
    packet_of = np.repeat(np.arange(len(pfirst)), pcount)              # LeafTri record -> its packet (records are covered in order)
    if instanced:
        in_n, in_c = np.nonzero(is_inst)
        _fail_if(np.bincount(first[in_n, in_c], minlength=num_inst) != 1, "instance_once", "instance not referenced exactly once")
        inst = tree["instances"]
        same = (inst["first_triangle"] == scene.instances["first_triangle"]) & (inst["num_triangles"] == scene.instances["num_triangles"])
        _fail_if(~same, "mesh_range", "DevInstance triangle range differs from the scene's")
        # every LeafTri of a mesh's tree names a triangle of that mesh's range; the top level's name loose triangles only
        owner = np.full(num_nodes, -1, np.int64)
        for r, w in zip(roots, walks[1:]):
            owner[w.visited] = r
        lo_of = np.full(num_nodes, -1, np.int64)
        hi_of = np.full(num_nodes, -1, np.int64)
        lo_of[inst["root"]], hi_of[inst["root"]] = inst["first_triangle"], inst["first_triangle"].astype(np.int64) + inst["num_triangles"]
        rec_owner = owner[pn][packet_of]
        instanced_tri = np.zeros(num_tris, bool)
        for rec in scene.instances:
            instanced_tri[int(rec["first_triangle"]):int(rec["first_triangle"]) + int(rec["num_triangles"])] = True
        in_mesh = rec_owner >= 0
        safe = np.maximum(rec_owner, 0)
        _fail_if(in_mesh & ((tri < lo_of[safe]) | (tri >= hi_of[safe])), "mesh_range", "mesh tree references a triangle outside its mesh")
        _fail_if(~in_mesh & instanced_tri[tri], "mesh_range", "the top level references an instanced triangle")

    # ---- LeafTri contents ----
    p, tlo, thi = _tri_boxes(scene)
    want = (p[tri, 0], p[tri, 1] - p[tri, 0], p[tri, 2] - p[tri, 0])
    for name, w in zip(("v0", "e1", "e2"), want):
        _fail_if(np.ascontiguousarray(leaf_tris[name]).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32), "leaf_tri_record",
                 "LeafTri.%s is not the float32 %s of its triangle" % (name, {"v0": "p0", "e1": "p1 - p0", "e2": "p2 - p0"}[name]))

    # ---- boxes ----
    lo, hi = nodes["lo"], nodes["hi"]                                    # [node, axis, child]
    slot_lo, slot_hi = lo[pn, :, pc], hi[pn, :, pc]                      # [packet, axis]
    if len(pfirst):
        union_lo, union_hi = np.minimum.reduceat(tlo[tri], pfirst, axis=0), np.maximum.reduceat(thi[tri], pfirst, axis=0)
        if not spatial_splits:
            _fail_if(slot_lo != union_lo, "leaf_box", "leaf box is not the union of its triangles' boxes (lower planes)")
            _fail_if(slot_hi != union_hi, "leaf_box", "leaf box is not the union of its triangles' boxes (upper planes)")
    nn, nc = np.nonzero(valid & ~leaf)
    kid = child[nn, nc].astype(np.int64)
    kid_lo, kid_hi = lo[kid].min(axis=2), hi[kid].max(axis=2)            # empty slots are +inf / -inf: the union of the valid ones
    if spatial_splits:
        _fail_if(lo[nn, :, nc] > kid_lo, "split_inner_box", "inner child's box does not contain its node's child boxes (lower planes)")
        _fail_if(hi[nn, :, nc] < kid_hi, "split_inner_box", "inner child's box does not contain its node's child boxes (upper planes)")
    else:
        _fail_if(lo[nn, :, nc] != kid_lo, "inner_box", "inner child's box is not the union of its node's child boxes (lower planes)")
        _fail_if(hi[nn, :, nc] != kid_hi, "inner_box", "inner child's box is not the union of its node's child boxes (upper planes)")
    if instanced:
        boxes = tree["instance_boxes"]
        k = first[in_n, in_c]
        _fail_if(lo[in_n, :, in_c] != boxes[k, 0, :3], "instance_box", "instance child's box is not the instance's world box (lower planes)")
        _fail_if(hi[in_n, :, in_c] != boxes[k, 1, :3], "instance_box", "instance child's box is not the instance's world box (upper planes)")
    if spatial_splits and len(pfirst):
        # the box a leaf's content is actually confined to: its own, cut by every ancestor's (top-down, level by level)
        eff_lo, eff_hi = np.full((num_nodes, 3), -np.inf, np.float32), np.full((num_nodes, 3), np.inf, np.float32)
        for level in top.levels:
            c = child[level]
            inner = (c != abi.INVALID_CHILD) & ((c & abi.LEAF_FLAG) == 0)
            ln, lc = np.nonzero(inner)
            eff_lo[c[ln, lc]] = np.maximum(lo[level[ln], :, lc], eff_lo[level[ln]])
            eff_hi[c[ln, lc]] = np.minimum(hi[level[ln], :, lc], eff_hi[level[ln]])
        rec_lo = np.maximum(slot_lo, eff_lo[pn])[packet_of]              # [LeafTri record, axis]
        rec_hi = np.minimum(slot_hi, eff_hi[pn])[packet_of]
        inside = ((p[tri] >= rec_lo[:, None, :]) & (p[tri] <= rec_hi[:, None, :])).all(axis=2)      # [record, vertex]
        held = np.zeros((num_tris, 3), np.int64)
        np.add.at(held, tri, inside)
        _fail_if(held < 1, "split_vertex", "triangle vertex in no leaf box (cut by its ancestors) that references the triangle")

    # ---- quantized nodes ----
    if tree.get("nodes_q") is not None:
        check_quantized(nodes, tree["nodes_q"], loose_steps, stats)
    return dict(levels=depth, packets=len(pfirst))
