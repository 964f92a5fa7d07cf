"""Re-seating the top-level tree on the device after instances have moved (slrhip_rebuild_top_level, slrhip_top_level_cost).

CPU: the exports; the sort key (slrhip_top_level_key: the function the kernels call) against a float32 numpy restatement, bit for bit;
the plan (leaf slots depth-first, canonical references) against a recursive walk; the whole operation on host trees
(slrhip_debug_top_level_reseat) against the tree validator, numpy's stable sort of numpy's keys, and itself applied twice; the cost
against a float64 restatement, and its fall where re-seating helps; every refusal.

GPU: the device's node array after the call equals the host twin applied to the read-out taken before it; the context renders, answers
queries and fills feature buffers bit for bit as before the call and as a fresh upload of the moved scene does; a second call changes
nothing; both device paths run (one workgroup up to kTopSeatGroup primitives, a device radix sort above).  The yardstick is the fresh
upload and the host twin; no tolerance is involved."""
import ctypes as C
import functools
import sys

import numpy as np
import pytest

import test_instance_update as T
import tree_checks
from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, SlrHipError
from test_instance_update import contexts  # noqa: F401  (the module-scoped fixture)

F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
LEAF, INVALID_CHILD, COUNT_SHIFT, INDEX_MASK = T.LEAF, T.INVALID_CHILD, T.COUNT_SHIFT, T.INDEX_MASK
SCENES = T.SCENES + ["wide"]
CPU_MOVES = ["none", "perturb", "permute", "partial"]
GPU_MOVES = ["none", "perturb", "permute", "shrink_and_back", "partial"]
sys.setrecursionlimit(max(sys.getrecursionlimit(), 4000))


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name == "wide":
        return scenes.instanced_grid(tiles_x=80, tiles_z=64, cells=2, aspect=1.0)      # 5 120 instances + 1 loose packet > kTopSeatGroup
    return T.base_scene(name)


@functools.lru_cache(maxsize=None)
def moved(name, move):
    """test_instance_update.moved for the four scenes, and the move "none": (records after the move, first, count)."""
    if move == "none":
        rec = T.records(base_scene(name))
        return rec, 0, len(rec)
    if name != "wide":
        return T.moved(name, move)
    sc = base_scene(name)
    rec, n = T.records(sc), len(sc.instances)
    rng = np.random.default_rng(5)
    small = rng.uniform(-0.03, 0.03, (n, 3))
    if move == "perturb":
        return T.translated(rec, small), 0, n
    if move == "permute":
        out = rec.copy()
        key = sc.instances["first_triangle"]
        for mesh in np.unique(key):
            idx = np.nonzero(key == mesh)[0]
            out[idx] = rec[np.roll(rng.permutation(idx), 1)] if len(idx) > 2 else rec[idx[::-1]]
        return out, 0, n
    if move == "shrink_and_back":
        return T.scaled(rec, 0.5), 0, n
    assert move == "partial"
    first, count = n // 3, max(1, n // 2)
    out = rec.copy()
    out[first:first + count] = T.translated(rec, 2.0 * small)[first:first + count]
    return out, first, count


# ---------------------------------------------------------------- numpy restatements ---------------------------------------------------------
def words_of(nodes):
    """[n, 32] uint32 words of qnode_dtype records (a copy)."""
    return np.array(nodes, copy=True).view(np.uint32).reshape(len(nodes), 32)


def planes_of(words):
    """A float32 view [node, plane (minx miny minz maxx maxy maxz), child] of node words."""
    return words[:, :24].view(F).reshape(-1, 6, 4)


def is_leaf(ref):
    return ref != INVALID_CHILD and bool(ref & LEAF)


def is_instance(ref):
    return is_leaf(ref) and ((ref >> COUNT_SHIFT) & 15) == 0


def numpy_plan(words, top_nodes):
    """Leaf slots depth-first from node 0 (a recursive walk), and their child words ascending."""
    slots = []

    def walk(node):
        for c in range(4):
            ref = int(words[node, 24 + c])
            if ref == INVALID_CHILD:
                continue
            if ref & LEAF:
                slots.append(node * 4 + c)
            else:
                assert node < ref < top_nodes
                walk(ref)
    walk(0)
    slots = np.array(slots, np.uint32)
    return slots, np.sort(words[slots >> 2, 24 + (slots & 3)])


def primitive_boxes(words, slots, refs, inst_boxes):
    """[primitive, 2, 3] float32 in canonical order: an instance's world box, a packet's slot box."""
    n_inst = len(inst_boxes)
    boxes = np.zeros((len(refs), 2, 3), F)
    boxes[:n_inst] = inst_boxes[:, :, :3]
    planes = planes_of(words)
    for s in slots:
        ref = words[s >> 2, 24 + (s & 3)]
        if not is_instance(int(ref)):
            boxes[np.searchsorted(refs, ref)] = planes[s >> 2, :, s & 3].reshape(2, 3)
    return boxes


def numpy_axis(lo, hi, slo, shi):
    """One axis of the key, float32 operation by operation."""
    lo, hi, slo, shi = (np.asarray(a, F) for a in (lo, hi, slo, shi))
    with np.errstate(all="ignore"):
        c = (lo + hi) * F(0.5)
        e = shi - slo
        x = np.where(e > 0, (c - slo) / e, F(0))
        assert c.dtype == F and e.dtype == F and x.dtype == F
        q = np.where(x >= 0, np.minimum(np.floor(x * F(2097152.0)), F(2097151.0)), F(0))
    return q.astype(np.uint32)


def numpy_keys(boxes, slo=None, shi=None):
    """uint64 keys of boxes [n, 2, 3] in the scene box (default: their union): bit 3 i + 2 = bit i of q.x, 3 i + 1 of q.y, 3 i of q.z."""
    boxes = np.asarray(boxes, F)
    if slo is None:
        slo, shi = np.fmin.reduce(boxes[:, 0], axis=0), np.fmax.reduce(boxes[:, 1], axis=0)
    q = [numpy_axis(boxes[:, 0, a], boxes[:, 1, a], slo[a], shi[a]).astype(np.uint64) for a in range(3)]
    key = np.zeros(len(boxes), np.uint64)
    for i in range(21):
        for a, shift in ((0, 2), (1, 1), (2, 0)):
            key |= ((q[a] >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + shift)
    return key


def numpy_refit(words, top_nodes, inst_boxes):
    """The plain refit (pt_refit.h's rule) on node words in place: instance children take their boxes, inner children the union of
    the valid children of the node they name, deepest first."""
    planes = planes_of(words)
    for node in range(top_nodes - 1, -1, -1):
        for c in range(4):
            ref = int(words[node, 24 + c])
            if ref == INVALID_CHILD:
                continue
            if is_instance(ref):
                planes[node, :, c] = inst_boxes[ref & INDEX_MASK, :, :3].reshape(6)
            elif not ref & LEAF:
                valid = words[ref, 24:28] != INVALID_CHILD
                planes[node, :3, c] = planes[ref, :3][:, valid].min(axis=1)
                planes[node, 3:, c] = planes[ref, 3:][:, valid].max(axis=1)
    return words


def numpy_cost(words, top_nodes):
    """1 + sum of the inner-child box areas / the root box's area, float64, summed in node order then child order."""
    planes = planes_of(words[:top_nodes]).astype(np.float64)
    child = words[:top_nodes, 24:28]

    def area(lo, hi):
        d = np.maximum(hi - lo, 0.0)
        return 2.0 * ((d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2]) + d[..., 2] * d[..., 0])
    valid0 = child[0] != INVALID_CHILD
    root = area(planes[0, :3][:, valid0].min(axis=1), planes[0, 3:][:, valid0].max(axis=1))
    if not root > 0:
        return 1.0
    inner = (child != INVALID_CHILD) & ((child & LEAF) == 0)
    areas = area(planes[:, :3].transpose(0, 2, 1), planes[:, 3:].transpose(0, 2, 1))      # [node, child]
    total = 0.0
    for a in areas[inner]:                                                                # (row-major: node order, then child order)
        total += float(a)
    return 1.0 + total / float(root)


@functools.lru_cache(maxsize=None)
def host_tree(name):
    return binding.host_tree(base_scene(name))


@functools.lru_cache(maxsize=None)
def moved_boxes(name, move):
    """[n, 2, 4] float32: the instances' world boxes after the move, through slrhip_instance_world_box and the host tree's mesh boxes."""
    sc, tree = base_scene(name), host_tree(name)
    rec = moved(name, move)[0]
    mesh = T.mesh_boxes_of(sc)
    out = np.zeros((len(rec), 2, 4), F)
    for k in range(len(rec)):
        lo, hi = binding.instance_world_box(mesh[k][0], mesh[k][1], rec[k, :16])
        out[k, 0, :3], out[k, 1, :3] = lo, hi
    if move == "none":
        assert np.array_equal(out.view(np.uint32), tree["instance_boxes"].view(np.uint32)), "the boxes restated here are not the upload's"
    return out


@functools.lru_cache(maxsize=None)
def refitted(name, move):
    """Node words of the host tree after the move and a plain refit: what the device holds after set_instance_transforms."""
    tree = host_tree(name)
    words = numpy_refit(words_of(tree["nodes"]), tree["top_nodes"], moved_boxes(name, move))
    if move == "none":
        assert np.array_equal(words, words_of(tree["nodes"])), "a refit of the uploaded tree changed it"
    words.setflags(write=False)
    return words


@functools.lru_cache(maxsize=None)
def reseated(name, move):
    """(node words, keys, order) of top_level_reseat on refitted(name, move)."""
    words, keys, order = binding.top_level_reseat(refitted(name, move), host_tree(name)["top_nodes"], moved_boxes(name, move))
    words.setflags(write=False)
    return words, keys, order


def as_tree(name, move, words):
    """A read-out's dict for tree_checks.check_tree: the host tree with other node words and the moved instances' boxes."""
    tree = dict(host_tree(name))
    tree["nodes"] = np.ascontiguousarray(words).reshape(-1).view(abi.qnode_dtype)
    tree["instance_boxes"] = moved_boxes(name, move)
    return tree


# ---------------------------------------------------------------- CPU --------------------------------------------------------------------
def test_exports_and_prototypes():
    lib = binding.load_library()
    names = ("slrhip_rebuild_top_level", "slrhip_top_level_cost", "slrhip_top_level_key", "slrhip_debug_top_level_rebuild_check",
             "slrhip_debug_top_level_plan", "slrhip_debug_top_level_reseat", "slrhip_debug_top_level_cost", "slrhip_debug_top_level_rebuild")
    import os
    header = open(os.path.join(T.ROOT, "include", "slrhip.h")).read()
    debug = open(os.path.join(T.ROOT, "include", "slrhip_debug.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in binding.EXPORTS, name
        assert ("int %s(" % name) in (debug if "_debug_" in name else header), name
    assert "#define SLRHIP_VERSION 7 " in header and lib.slrhip_version() == 7
    assert "#define SLRHIP_TOP_SEAT_GROUP %du" % abi.TOP_SEAT_GROUP in header
    for method in ("rebuild_top_level", "top_level_cost", "debug_top_level_rebuild"):
        assert callable(getattr(Context, method))
    for fn in ("top_level_key", "top_level_plan", "top_level_reseat", "top_level_cost_of", "top_level_rebuild_check"):
        assert callable(getattr(binding, fn))


@pytest.mark.parametrize("name", SCENES)
def test_key_equals_the_numpy_restatement_on_the_scenes(name):
    tree = host_tree(name)
    words = words_of(tree["nodes"])
    slots, refs = binding.top_level_plan(words, tree["top_nodes"])
    boxes = primitive_boxes(words, slots, refs, tree["instance_boxes"])
    slo, shi = boxes[:, 0].min(axis=0), boxes[:, 1].max(axis=0)
    want = numpy_keys(boxes)
    got = np.array([binding.top_level_key(b[0], b[1], slo, shi) for b in boxes], np.uint64)
    assert np.array_equal(got, want), (name, np.nonzero(got != want)[0][:8])
    assert len(np.unique(want)) > len(want) // 2 and int(want.max()) < 1 << 63


def test_key_on_corners_flat_axes_large_and_non_finite_boxes():
    slo, shi = np.array([-3.0, 0.5, 10.0], F), np.array([5.0, 0.5, 14.0], F)               # y: an axis of zero extent
    mid = (slo + shi) * F(0.5)
    nan, inf = F(np.nan), F(np.inf)
    cases = [(slo, slo, slo, shi), (shi, shi, slo, shi), (mid, mid, slo, shi), (slo, shi, slo, shi),
             # coordinates near 1e6: one ulp is 1 / 16, the centre and the quotient round
             ((1.0e6, 1.0e6 + 0.25, 999999.9), (1.0e6 + 3.0, 1.0e6 + 0.5, 1000000.1), (999990.0, 1.0e6, 999999.0), (1000010.0, 1.0e6 + 1.0, 1000001.0)),
             # outside the scene box: below clamps to 0 by the sign test, above to the last cell
             ((-9, 0, 0), (-8, 0, 0), slo, shi), ((50, 0, 50), (60, 0, 60), slo, shi),
             # non-finite boxes: 0 on that axis
             ((nan, 0.5, 11.0), (1.0, 0.5, 12.0), slo, shi), ((0.0, nan, nan), (1.0, nan, nan), slo, shi),
             ((-inf, 0.5, 11.0), (inf, 0.5, 12.0), slo, shi), ((0.0, 0.5, 11.0), (1.0, 0.5, 12.0), (nan, 0.5, 10.0), (5.0, 0.5, 14.0)),
             ((0.0, 0.5, 11.0), (1.0, 0.5, 12.0), (-inf, 0.5, 10.0), (inf, 0.5, 14.0))]
    rng = np.random.default_rng(11)
    for _ in range(200):
        a, b = rng.uniform(-100, 100, 3).astype(F), rng.uniform(0, 5, 3).astype(F)
        cases.append((a, a + b, (-100, -100, -100), (105, 105, 105)))
    for lo, hi, a, b in cases:
        box = np.array([lo, hi], F)[None]
        want = int(numpy_keys(box, np.asarray(a, F), np.asarray(b, F))[0])
        assert binding.top_level_key(lo, hi, a, b) == want, (lo, hi, a, b)
    q = lambda lo, hi, axis: int(numpy_axis(F(lo), F(hi), slo[axis], shi[axis]))
    assert q(slo[0], slo[0], 0) == 0 and q(shi[0], shi[0], 0) == 2097151 and q(mid[0], mid[0], 0) == 1 << 20 and q(0.5, 0.5, 1) == 0
    assert binding.top_level_key(shi, shi, slo, shi) == sum(1 << (3 * i + s) for i in range(21) for s in (0, 2))      # x and z full, y 0
    assert binding.top_level_key((nan, 0.5, 14.0), (nan, 0.5, 14.0), slo, shi) == sum(1 << (3 * i) for i in range(21))
    assert binding.top_level_key((-inf, 0.5, 10.0), (inf, 0.5, 10.0), slo, shi) == 0
    lib = binding.load_library()
    key = C.c_uint64(0)
    assert lib.slrhip_top_level_key(None, None, None, None, C.byref(key)) == INVALID


@pytest.mark.parametrize("name", SCENES)
def test_plan_lists_every_leaf_slot_depth_first(name):
    tree = host_tree(name)
    words, tn = words_of(tree["nodes"]), tree["top_nodes"]
    slots, refs = binding.top_level_plan(words, tn)
    want_slots, want_refs = numpy_plan(words, tn)
    assert np.array_equal(slots, want_slots) and np.array_equal(refs, want_refs)
    child = words[:tn, 24:28]
    leaf = (child != INVALID_CHILD) & ((child & LEAF) != 0)
    assert len(slots) == int(leaf.sum()) == len(np.unique(slots)) and leaf[slots >> 2, slots & 3].all()
    assert (np.diff(refs.astype(np.int64)) > 0).all()
    n = len(base_scene(name).instances)
    assert np.array_equal(refs[:n], LEAF | np.arange(n, dtype=np.uint32)) and (((refs[n:] >> COUNT_SHIFT) & 15) >= 1).all()
    if name == "wide":
        assert len(refs) == 5121 > abi.TOP_SEAT_GROUP >= len(binding.top_level_plan(words_of(host_tree("grid")["nodes"]), host_tree("grid")["top_nodes"])[0])
    with pytest.raises(SlrHipError, match=r"slrhip_debug_top_level_plan failed \(%d\)" % INVALID):
        binding.top_level_plan(words[tn:], 1)                     # a mesh tree's node: no instance leaves 0 .. n - 1, or no top level at all


@pytest.mark.parametrize("move", CPU_MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_reseat_on_the_host_tree(name, move):
    sc, tree = base_scene(name), host_tree(name)
    tn = tree["top_nodes"]
    before = refitted(name, move)
    after, keys, order = reseated(name, move)
    rec = moved(name, move)[0]
    tree_checks.check_tree(as_tree(name, move, before), T.with_records(sc, rec))
    tree_checks.check_tree(as_tree(name, move, after), T.with_records(sc, rec))
    # what stays
    child_b, child_a = before[:tn, 24:28], after[:tn, 24:28]
    leaf = (child_b != INVALID_CHILD) & ((child_b & LEAF) != 0)
    assert np.array_equal(leaf, (child_a != INVALID_CHILD) & ((child_a & LEAF) != 0))
    assert np.array_equal(child_b[~leaf], child_a[~leaf]), "an inner or empty child word changed"
    assert np.array_equal(np.sort(child_b[leaf]), np.sort(child_a[leaf])), "the leaf words are not the same multiset"
    assert np.array_equal(before[:, 28:], after[:, 28:]) and np.array_equal(before[tn:], after[tn:])
    empty = child_b == INVALID_CHILD
    assert np.array_equal(planes_of(before[:tn]).transpose(0, 2, 1)[empty].view(np.uint32), planes_of(after[:tn]).transpose(0, 2, 1)[empty].view(np.uint32))
    # the order: numpy's stable sort of numpy's keys, seated into the slots depth-first
    slots, refs = numpy_plan(before, tn)
    boxes = primitive_boxes(before, slots, refs, moved_boxes(name, move))
    want_keys = numpy_keys(boxes)
    want_order = np.argsort(want_keys, kind="stable").astype(np.uint32)
    assert np.array_equal(keys, want_keys) and np.array_equal(order, want_order)
    assert np.array_equal(after[slots >> 2, 24 + (slots & 3)], refs[want_order])
    assert np.array_equal(planes_of(after)[slots >> 2, :, slots & 3].view(np.uint32), boxes[want_order].reshape(-1, 6).view(np.uint32))
    if name == "lattice" and move == "none":
        assert len(np.unique(want_keys)) < len(want_keys), "the coincident placements should give an equal pair of keys"
    # a second application changes no word
    again, keys2, order2 = binding.top_level_reseat(after, tn, moved_boxes(name, move))
    assert np.array_equal(again, after) and np.array_equal(keys2, keys) and np.array_equal(order2, order)


@pytest.mark.parametrize("name", SCENES)
def test_cost_equals_the_numpy_restatement_and_falls_where_reseating_helps(name):
    tn = host_tree(name)["top_nodes"]
    cost = {}
    for move in CPU_MOVES:
        for state, words in (("refit", refitted(name, move)), ("reseated", reseated(name, move)[0])):
            cost[move, state] = binding.top_level_cost_of(words, tn)
            assert cost[move, state] == numpy_cost(words, tn), (name, move, state)
            assert cost[move, state] >= 1.0
    print(name, {k: round(v, 2) for k, v in cost.items()})
    if name in ("grid", "wide"):
        assert cost["permute", "reseated"] < cost["permute", "refit"]
        assert cost["permute", "refit"] > 10.0 * cost["none", "refit"]          # the damage the call is for
    flat = np.zeros((1, 32), np.uint32)
    flat[0, 24:28] = INVALID_CHILD
    assert binding.top_level_cost_of(flat, 1) == 1.0                           # a root of zero area


def test_refusals_through_the_check_twin():
    lib = binding.load_library()
    binding.top_level_rebuild_check(True, 1)
    binding.top_level_rebuild_check(True, 5000)
    for args, code, text in (((False, 0), NO_SCENE, "no scene uploaded"), ((False, 7), NO_SCENE, "no scene uploaded"),
                             ((True, 0), UNSUPPORTED, "the scene has no instances")):
        with pytest.raises(SlrHipError) as e:
            binding.top_level_rebuild_check(*args)
        assert str(e.value) == "slrhip_debug_top_level_rebuild_check failed (%d): slrhip_rebuild_top_level: %s" % (code, text)
    cost = C.c_double(0)
    assert lib.slrhip_rebuild_top_level(None, None) == INVALID and b"slrhip_rebuild_top_level: null context" in lib.slrhip_last_error_string()
    assert lib.slrhip_top_level_cost(None, C.byref(cost), None) == INVALID
    assert lib.slrhip_debug_top_level_rebuild(None, 0, None, 0) == INVALID
    assert lib.slrhip_debug_top_level_cost(None, 1, C.byref(cost)) == INVALID
    assert lib.slrhip_debug_top_level_reseat(None, 1, None, 0, None, None) == INVALID


# ---------------------------------------------------------------- GPU --------------------------------------------------------------------
def assert_same_nodes(got, want, what):
    """Planes as float values, every other word by bytes."""
    assert got.shape == want.shape
    assert np.array_equal(got[:, :24].view(F), want[:, :24].view(F)), "%s: %d planes differ" % (what, (got[:, :24].view(F) != want[:, :24].view(F)).sum())
    assert np.array_equal(got[:, 24:], want[:, 24:]), "%s: %d child or pad words differ" % (what, (got[:, 24:] != want[:, 24:]).sum())


def place(ctx, name, move):
    """Upload the scene and apply the move; returns the records in place."""
    ctx.upload_scene(base_scene(name))
    rec, lo, count = moved(name, move)
    if move != "none":
        ctx.set_instance_transforms(rec[lo:lo + count], first=lo)
        assert ctx.instances_status() == 0
    return rec


def expected_path(name):
    return "radix" if name == "wide" else "group"


@pytest.mark.gpu
@pytest.mark.parametrize("move", GPU_MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_rebuild_equals_the_host_twin_and_changes_no_result(contexts, name, move):
    sc = base_scene(name)
    ctx, fresh = contexts(), contexts(which=1)
    rec = place(ctx, name, move)
    what = "%s %s" % (name, move)
    assert ctx.debug_top_level_rebuild()["primitives"] == 0                    # the tables are the first call's
    before = ctx.debug_top_level()
    first = T.everything(ctx)
    ctx.rebuild_top_level()
    after = ctx.debug_top_level()
    out = ctx.debug_top_level_rebuild()
    tn = before["top_nodes"]
    want, keys, order = binding.top_level_reseat(before["nodes"], tn, before["boxes"])
    assert_same_nodes(after["nodes"], want, what)
    assert np.array_equal(out["keys"], keys) and np.array_equal(out["order"], order), what
    slots, refs = binding.top_level_plan(before["nodes"], tn)
    assert np.array_equal(out["slots"], slots) and np.array_equal(out["refs"], refs) and out["primitives"] == len(refs)
    assert out["seat_group"] == abi.TOP_SEAT_GROUP and out["num_instances"] == len(sc.instances)
    if name == "wide":
        assert out["primitives"] > out["seat_group"] >= len(base_scene("grid").instances) + 1
    assert out["path"] == expected_path(name) and out["launches"] >= 2, out
    tree_checks.check_tree(ctx.debug_tree(), T.with_records(sc, rec))
    for k in ("instances", "boxes", "mesh_boxes", "levels"):
        assert np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)), (what, k)
    if move == "permute" and name in ("grid", "wide"):
        assert not np.array_equal(after["nodes"], before["nodes"])
    got = T.everything(ctx)
    T.assert_same(got, first, what + ": before and after the rebuild")
    fresh.upload_scene(T.with_records(sc, rec))
    T.assert_same(got, T.everything(fresh), what + ": against a fresh upload")
    if name == "lattice":
        frame, ctr = ob.load("oracle", abi.MODE_RGB).scene(T.with_records(sc, rec)).render(T.settings(), T.SPP)
        assert_bit_equal(got["frame"], frame, what + " vs the oracle")
        assert int(got["counters"][1]) == int(ctr.extension_rays) and int(got["counters"][2]) == int(ctr.shadow_rays)
    ctx.rebuild_top_level()
    T.assert_same_top(ctx.debug_top_level(), after, what + ": a second rebuild")
    again = ctx.debug_top_level_rebuild()
    assert np.array_equal(again["keys"], keys) and np.array_equal(again["order"], order) and again["path"] == out["path"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", T.SCENES)
def test_instances_keep_moving_after_a_rebuild(contexts, name):
    sc = base_scene(name)
    ctx, fresh = contexts(), contexts(which=1)
    place(ctx, name, "permute")
    ctx.rebuild_top_level()
    original = ctx.debug_top_level()
    rec = T.translated(moved(name, "permute")[0], np.random.default_rng(8).integers(-1, 2, (len(sc.instances), 3)).astype(np.float64)
                       if name == "lattice" else np.random.default_rng(8).uniform(-0.03, 0.03, (len(sc.instances), 3)))
    ctx.set_instance_transforms(rec)
    assert ctx.instances_status() == 0
    T.check_invariant(sc, ctx.debug_top_level(), original, rec, name + " moved after a rebuild")
    fresh.upload_scene(T.with_records(sc, rec))
    T.assert_same(T.everything(ctx), T.everything(fresh), name + " moved after a rebuild")


@pytest.mark.gpu
def test_spectral_context(contexts):
    sc = base_scene("cornell")
    ctx, fresh = contexts(abi.MODE_SPECTRAL), contexts(abi.MODE_SPECTRAL, 1)
    rec = place(ctx, "cornell", "permute")
    first = T.everything(ctx)
    ctx.rebuild_top_level()
    fresh.upload_scene(T.with_records(sc, rec))
    got = T.everything(ctx)
    T.assert_same(got, first, "spectral cornell permute: before and after")
    T.assert_same(got, T.everything(fresh), "spectral cornell permute: fresh upload")


@pytest.mark.gpu
def test_rebuild_between_two_render_calls_resets_nothing(contexts):
    ctx, other = contexts(), contexts(which=1)
    place(ctx, "grid", "permute")
    place(other, "grid", "permute")
    other.render_begin(T.settings())
    other.render(0, 8)
    want = other.read_framebuffer()
    ctx.render_begin(T.settings())
    ctx.render(0, 4)
    ctx.rebuild_top_level()
    ctx.render(4, 4)
    got = ctx.read_framebuffer()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got.max() > 0
    a, b = ctx.counters(), other.counters()
    assert (a.samples, a.extension_rays, a.shadow_rays) == (b.samples, b.extension_rays, b.shadow_rays)


@pytest.mark.gpu
def test_rebuild_lowers_the_traversal_counts_and_the_cost_on_the_permuted_grid(contexts):
    ctx = contexts(flags=abi.FLAG_COUNT_TRAVERSAL)
    ctx.upload_scene(base_scene("grid"))
    uploaded = ctx.top_level_cost()
    place(ctx, "grid", "permute")

    def look():
        ctx.render_begin(T.settings())
        ctx.render(0, T.SPP)
        p = ctx.profile()
        top = ctx.debug_top_level()
        cost = ctx.top_level_cost()
        assert cost == binding.top_level_cost_of(top["nodes"], top["top_nodes"])
        return sum(p.nodes), list(p.triangles), list(p.rays), cost, ctx.read_framebuffer()
    refit = look()
    assert look()[:4] == refit[:4]                                             # the counts are deterministic
    ctx.rebuild_top_level()
    rebuilt = look()
    print("nodes visited: refit only %d, rebuilt %d; cost: uploaded %.2f, refit only %.2f, rebuilt %.2f" % (refit[0], rebuilt[0], uploaded, refit[3], rebuilt[3]))
    assert 0 < rebuilt[0] < refit[0] and rebuilt[2] == refit[2]
    assert uploaded < rebuilt[3] < refit[3]
    assert np.array_equal(rebuilt[4].view(np.uint32), refit[4].view(np.uint32))


@pytest.mark.gpu
def test_refusals_change_nothing_and_an_upload_drops_the_state(contexts):
    lib = binding.load_library()
    empty = Context(device=0)
    try:
        for call in (empty.rebuild_top_level, empty.top_level_cost, empty.debug_top_level_rebuild):
            with pytest.raises(SlrHipError, match=r"failed \(%d\).*no scene uploaded" % NO_SCENE):
                call()
        flat = T.base_scene("flat")
        empty.upload_scene(flat)

        def look():
            empty.render_begin(T.settings())
            empty.render(0, T.SPP)
            k = empty.counters()
            return dict(frame=empty.read_framebuffer(), counters=np.array([k.samples, k.extension_rays, k.shadow_rays], np.uint64), rays=empty.camera_rays(0)[0])
        first = look()
        for call in (empty.rebuild_top_level, empty.top_level_cost, empty.debug_top_level_rebuild):
            with pytest.raises(SlrHipError, match=r"failed \(%d\).*the scene has no instances" % UNSUPPORTED):
                call()
        T.assert_same(look(), first, "flat scene after the refusals")
    finally:
        empty.close()
    ctx = contexts()
    place(ctx, "cornell", "permute")
    ctx.rebuild_top_level()
    n_cornell = ctx.debug_top_level_rebuild()["primitives"]
    top = ctx.debug_top_level()
    first = T.everything(ctx)
    room = np.zeros(64, np.uint32)
    assert lib.slrhip_top_level_cost(ctx.handle, None, None) == INVALID and lib.slrhip_debug_top_level_rebuild(ctx.handle, 9, room.ctypes.data, 64) == INVALID
    assert lib.slrhip_debug_top_level_rebuild(ctx.handle, 1, room.ctypes.data, 1) == INVALID and not room.any()
    T.assert_same_top(ctx.debug_top_level(), top, "after the refusals")
    T.assert_same(T.everything(ctx), first, "after the refusals")
    # another instanced scene: the state was dropped, and the next call builds it for the new scene
    rec = place(ctx, "grid", "permute")
    assert ctx.debug_top_level_rebuild()["primitives"] == 0
    before = ctx.debug_top_level()
    ctx.rebuild_top_level()
    out = ctx.debug_top_level_rebuild()
    assert out["primitives"] == len(rec) + (out["primitives"] - out["num_instances"]) != n_cornell and out["num_instances"] == len(rec)
    want, keys, order = binding.top_level_reseat(before["nodes"], before["top_nodes"], before["boxes"])
    assert_same_nodes(ctx.debug_top_level()["nodes"], want, "grid after cornell")
    assert np.array_equal(out["keys"], keys) and np.array_equal(out["order"], order)


# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process: the checks on a torch stream run in a
# fresh child process that imports torch BEFORE libslrhip.so is loaded.
@pytest.mark.gpu
def test_later_calls_on_a_torch_stream_can_be_captured_in_a_graph():
    """Both device paths: a later call allocates nothing and does not synchronise, so it replays from a graph with the eager result."""
    import os
    import subprocess
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_top_level_rebuild as R\nR._graph_check()\n" % (T.ROOT, os.path.join(T.ROOT, "tests")))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=T.ROOT, capture_output=True, text=True, timeout=600)
    assert "OK _graph_check" in p.stdout, p.stdout[-4000:] + "\n" + p.stderr[-3000:]


def _graph_check():
    import torch
    ctx = Context(device=0)
    try:
        for name in ("grid", "wide"):
            rec, perm = T.records(base_scene(name)), moved(name, "permute")[0]
            ctx.upload_scene(base_scene(name))
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                t = torch.from_numpy(perm.copy()).cuda()
                back = torch.from_numpy(rec.copy()).cuda()
                ctx.set_instance_transforms(t, stream=side)
                ctx.rebuild_top_level(side)                               # the first call: builds the tables, synchronises
                want, info = ctx.debug_top_level(), ctx.debug_top_level_rebuild()
                assert info["path"] == expected_path(name)
                ctx.set_instance_transforms(back, stream=side)            # somewhere else, in between
                ctx.rebuild_top_level(side)
                side.synchronize()
                assert not np.array_equal(ctx.debug_top_level()["nodes"], want["nodes"])
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=side):
                    s = torch.cuda.current_stream()
                    ctx.set_instance_transforms(t, stream=s)
                    ctx.rebuild_top_level(s)
                g.replay()
                torch.cuda.synchronize()
            assert ctx.instances_status(side) == 0
            T.assert_same_top(ctx.debug_top_level(), want, name + " replayed from a graph")
            again = ctx.debug_top_level_rebuild()
            assert np.array_equal(again["keys"], info["keys"]) and np.array_equal(again["order"], info["order"])
        print("OK _graph_check", flush=True)
    finally:
        ctx.close()
