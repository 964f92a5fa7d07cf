"""Moving instances and the camera without a scene upload (slrhip_set_instance_transforms, slrhip_set_camera).

CPU: the exports and the record layout; every refusal through the context-free check; the instance-box arithmetic
(slrhip_instance_world_box: the function the upload and the kernel call) against a numpy restatement of the host build's loop, bit for bit.

GPU: an update with the uploaded matrices changes no bit of the top level; after every update the top-level tree holds, child by child,
exactly the boxes its rule names (an instance's world box, a packet's old box, the union of the named node's children — equal, not
merely containing), with references and mesh trees untouched; and a context that was updated renders, answers queries and fills feature
buffers bit for bit as a context freshly uploaded with the moved scene does.  The yardstick throughout is the fresh upload (and, on the
exact lattice scene, the oracle); no tolerance is involved."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, DeviceBlocks, SlrHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
SIZE, SPP = 32, 8
LEAF, INVALID_CHILD, COUNT_SHIFT, INDEX_MASK = 0x80000000, 0xFFFFFFFF, 27, (1 << 27) - 1
SCENES = ["lattice", "cornell", "grid"]
MOVES = ["perturb", "permute", "shrink_and_back", "partial"]


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name == "lattice":
        return scenes.lattice_instanced()
    if name == "cornell":
        return scenes.cornell_instanced(1.0, 10, 5, copies=24)
    if name == "grid":
        return scenes.instanced_grid(tiles_x=25, tiles_z=50, cells=4, aspect=1.0)
    assert name == "flat"
    return scenes.cornell_box_spheres(1.0, 8, 4, "glass")


def settings(seed=9):
    return ob.settings(SIZE, SIZE, seed=seed)


def records(sc):
    """[n, 32] float32: local_to_world, world_to_local of the scene's instances."""
    return np.concatenate([sc.instances["local_to_world"], sc.instances["world_to_local"]], axis=1).astype(F)


def with_records(sc, rec=None, camera=None):
    """The scene with the instance matrices of `rec` and / or another camera: what a fresh context uploads."""
    inst = sc.instances.copy()
    if rec is not None:
        inst["local_to_world"], inst["world_to_local"] = rec[:, :16], rec[:, 16:]
    assert sc.env is None and len(sc.textures) == 0
    return abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, camera if camera is not None else sc.camera, None,
                     sc.name + "_moved", instances=inst if len(inst) else None)


def _mats(rec):
    """float64 4x4 matrices (row, column) of column-major records: (local_to_world, world_to_local) [n, 4, 4]."""
    r = rec.astype(np.float64)
    return r[:, :16].reshape(-1, 4, 4).transpose(0, 2, 1), r[:, 16:].reshape(-1, 4, 4).transpose(0, 2, 1)


def _records(l2w, w2l):
    return np.concatenate([l2w.transpose(0, 2, 1).reshape(-1, 16), w2l.transpose(0, 2, 1).reshape(-1, 16)], axis=1).astype(F)


def translated(rec, d):
    """World translations d [n, 3] after each placement: T(d) L and W T(-d), rounded to float32 once (both routes get the same bits)."""
    l2w, w2l = _mats(rec)
    t, ti = np.tile(np.eye(4), (len(rec), 1, 1)), np.tile(np.eye(4), (len(rec), 1, 1))
    t[:, :3, 3], ti[:, :3, 3] = d, -np.asarray(d, np.float64)
    return _records(t @ l2w, w2l @ ti)


def scaled(rec, s):
    """A local scale s (a power of two: exact) before each placement: L S(s) and S(1 / s) W."""
    l2w, w2l = _mats(rec)
    return _records(l2w @ np.diag([s, s, s, 1.0]), np.diag([1 / s, 1 / s, 1 / s, 1.0]) @ w2l)


def moved(name, move):
    """(records of every instance after the move, first, count): what the update call is given is rows first .. first + count."""
    sc = base_scene(name)
    rec, n = records(sc), len(sc.instances)
    rng = np.random.default_rng(5)
    # the lattice scene keeps exact matrices (integer translations), so that its frames stay bit-exact against the oracle
    small = rng.integers(-1, 2, (n, 3)).astype(np.float64) if name == "lattice" else rng.uniform(-0.03, 0.03, (n, 3))
    if move == "perturb":
        return translated(rec, small), 0, n
    if move == "permute":
        # placements change hands among the instances of one mesh: every instance lands somewhere else in the scene
        out = rec.copy()
        key = sc.instances["first_triangle"]
        for mesh in np.unique(key):
            idx = np.nonzero(key == mesh)[0]
            out[idx] = rec[np.roll(rng.permutation(idx), 1)] if len(idx) > 2 else rec[idx[::-1]]
        return out, 0, n
    if move == "shrink_and_back":
        return scaled(rec, 0.5), 0, n
    assert move == "partial"
    first, count = n // 3, max(1, n // 2)
    out = rec.copy()
    out[first:first + count] = translated(rec, 2.0 * small)[first:first + count]
    return out, first, count


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(mode=abi.MODE_RGB, which=0, flags=0):
        key = (mode, which, flags)
        if key not in made:
            made[key] = Context(device=0, mode=mode, flags=flags)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def everything(ctx, seed=9):
    """What a caller can get out of a context for its scene: the frame and its counters, the closest hits and the visibility of the
    camera rays of sample 0, every feature buffer."""
    ctx.render_begin(settings(seed))
    ctx.render(0, SPP)
    k = ctx.counters()
    out = dict(frame=ctx.read_framebuffer(), counters=np.array([k.samples, k.extension_rays, k.shadow_rays], np.uint64))
    rows, xy = ctx.camera_rays(0)
    out["rays"], out["xy"] = rows, xy
    if rows.shape[0]:
        out["hits"], out["hit_instances"] = ctx.intersect_rays(rows, want_instances=True)
        shadow = rows.copy()
        shadow[:, 7] = np.where(np.isfinite(out["hits"][:, 1]) & (out["hits"].view(np.uint32)[:, 0] != abi.MISS), out["hits"][:, 1] * F(2.0), F(10.0))
        out["visible"] = ctx.test_visibility(shadow)
    ctx.render_begin(settings(seed))
    ctx.render_features(abi.FEATURE_ALL, 2)
    for ch in sorted(abi.FEATURE_CHANNELS):
        out["feature_" + abi.FEATURE_CHANNELS[ch][0]] = ctx.features(ch)
    return out


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        differ = a.view(np.uint8) != b.view(np.uint8)
        assert not differ.any(), "%s: %s: %d of %d bytes differ" % (what, k, differ.sum(), differ.size)


def assert_same_top(got, want, what):
    for k in ("levels", "nodes", "instances", "boxes", "mesh_boxes"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), "%s: read-out %s differs in %d words" % (
            what, k, (got[k].view(np.uint32) != want[k].view(np.uint32)).sum())


def numpy_world_box(lo, hi, m):
    """The instance-box loop of the host build, restated in float32: the eight corners through the column-major matrix (products
    added left to right, the translation last), min / max, then the pad 1e-5f * max(1, |lo|, |hi|) per axis."""
    lo, hi, m = (np.asarray(a, F) for a in (lo, hi, m))
    wlo, whi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    one = F(1.0)
    for c in range(8):
        p = [hi[0] if c & 4 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 1 else lo[2]]
        with np.errstate(all="ignore"):
            q = [((m[r] * p[0] + m[4 + r] * p[1]) + m[8 + r] * p[2]) + m[12 + r] * one for r in range(4)]
            if q[3] != one:
                inv = one / q[3]
                q = [q[0] * inv, q[1] * inv, q[2] * inv]
        for a in range(3):
            assert q[a].dtype == F
            wlo[a], whi[a] = min(wlo[a], q[a]), max(whi[a], q[a])
    for a in range(3):
        pad = F(1e-5) * max(one, abs(wlo[a]), abs(whi[a]))
        wlo[a], whi[a] = wlo[a] - pad, whi[a] + pad
    return wlo, whi


def mesh_boxes_of(sc):
    """(lo, hi) of the local box of each instance's mesh, by instance."""
    out = []
    pos = sc.vertices["position"].astype(F)
    for rec in sc.instances:
        v = pos[sc.triangles["v"][int(rec["first_triangle"]):int(rec["first_triangle"]) + int(rec["num_triangles"])].reshape(-1)]
        out.append((v.min(axis=0), v.max(axis=0)))
    return out


# ---------------------------------------------------------------- CPU --------------------------------------------------------------------
def test_exports_and_struct_layout():
    lib = binding.load_library()
    for name in ("slrhip_set_instance_transforms", "slrhip_instances_status", "slrhip_instance_world_box", "slrhip_set_camera",
                 "slrhip_debug_instance_update_check", "slrhip_debug_top_level"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    d = abi.instance_transform_dtype
    assert d.itemsize == 128 and d.fields["local_to_world"][1] == 0 and d.fields["world_to_local"][1] == 64
    assert abi.INSTANCE_BAD_TRANSFORM == 1
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert "#define SLRHIP_VERSION 7 " in header and "#define SLRHIP_INSTANCE_BAD_TRANSFORM 1u" in header
    assert lib.slrhip_version() == 7


def test_refusals_through_the_check_twin():
    lib = binding.load_library()
    check = lib.slrhip_debug_instance_update_check
    ok = dict(have_scene=1, num_instances=10, src=4096, first=2, count=8)

    def call(**over):
        a = dict(ok, **over)
        return check(a["have_scene"], a["num_instances"], a["src"], a["first"], a["count"]), lib.slrhip_last_error_string().decode()
    assert call()[0] == 0 and call(first=0, count=10)[0] == 0 and call(first=9, count=1)[0] == 0
    beyond = "first_instance + count is beyond the scene's instances"
    for over, code, text in ((dict(src=None), INVALID, "null device_src"), (dict(src=4096 + 8), INVALID, "misaligned device_src (16 bytes)"),
                             (dict(count=0), INVALID, "count must be >= 1"), (dict(have_scene=0), NO_SCENE, "no scene uploaded"),
                             (dict(num_instances=0), UNSUPPORTED, "the scene has no instances"),
                             (dict(first=3), INVALID, beyond), (dict(first=10, count=1), INVALID, beyond),
                             (dict(first=1, count=0xFFFFFFFF), INVALID, beyond)):                              # first + count wraps in 32 bits
        rc, msg = call(**over)
        assert rc == code and msg == "slrhip_set_instance_transforms: " + text, (over, rc, msg)
    assert lib.slrhip_set_instance_transforms(None, 4096, 0, 1, None) == INVALID
    assert lib.slrhip_set_camera(None, None) == INVALID
    bits_ = C.c_uint32(5)
    assert lib.slrhip_instances_status(None, C.byref(bits_), None) == INVALID
    assert lib.slrhip_instance_world_box(None, None, None, None, None) == INVALID


@pytest.mark.parametrize("name", SCENES)
def test_world_box_equals_the_numpy_restatement_on_the_scenes(name):
    sc = base_scene(name)
    boxes = mesh_boxes_of(sc)
    step = max(1, len(sc.instances) // 60)                  # the grid: every 20th placement and the last
    for move in ["none"] + MOVES[:3]:
        rec = records(sc) if move == "none" else moved(name, move)[0]
        for k in sorted(set(range(0, len(rec), step)) | {len(rec) - 1}):
            got, want = binding.instance_world_box(boxes[k][0], boxes[k][1], rec[k, :16]), numpy_world_box(boxes[k][0], boxes[k][1], rec[k, :16])
            assert np.array_equal(np.concatenate(got).view(np.uint32), np.concatenate(want).view(np.uint32)), (name, move, k, got, want)


def test_world_box_of_a_flat_box_and_of_large_coordinates():
    rng = np.random.default_rng(3)
    turn = np.array(scenes._rotate(0.7, (0.3, 1.0, 0.2)) @ scenes._translate(0.25, -3.0, 1.5), np.float64)
    m = turn.T.reshape(-1).astype(F)
    # a flat mesh box (one triangle in a plane): the world box of an axis-aligned placement stays flat but for the pad
    lo, hi = binding.instance_world_box((0, 2, 0), (4, 2, 4), np.eye(4).T.reshape(-1))
    assert np.array_equal(np.concatenate([lo, hi]).view(np.uint32), np.concatenate(numpy_world_box((0, 2, 0), (4, 2, 4), np.eye(4).reshape(-1))).view(np.uint32))
    assert lo[1] == F(2.0) - F(1e-5) * F(2.0) and hi[1] == F(2.0) + F(1e-5) * F(2.0) and lo[0] == -(F(1e-5) * F(4.0)) and hi[0] == F(4.0) + F(1e-5) * F(4.0)
    cases = [((0, 2, 0), (4, 2, 4), m), ((-1, -1, -1), (-1, -1, -1), m)]                     # flat under a rotation; a single point
    # large coordinates: the pad is the |coordinate| term, and one ulp there is larger than 1e-5
    far = scenes._translate(3.0e6, -2.5e5, 7.0e3) @ turn
    cases += [((-1, 0, -1), (1, 0.5, 1), far.T.reshape(-1).astype(F)), ((1e5, 2e5, -3e5), (1.5e5, 2.5e5, -2e5), m)]
    cases += [(sorted_lo, sorted_hi, (scenes._translate(*rng.uniform(-50, 50, 3)) @ scenes._rotate(float(rng.uniform(0, 6)), (0, 1, 0))
                                      @ np.diag(list(rng.uniform(0.1, 3, 3)) + [1.0])).T.reshape(-1).astype(F))
              for sorted_lo, sorted_hi in [(-rng.uniform(0, 2, 3), rng.uniform(0, 2, 3)) for _ in range(40)]]
    for blo, bhi, mat in cases:
        got, want = binding.instance_world_box(blo, bhi, mat), numpy_world_box(blo, bhi, mat)
        assert np.array_equal(np.concatenate(got).view(np.uint32), np.concatenate(want).view(np.uint32)), (blo, bhi, got, want)
    lo, hi = binding.instance_world_box((-1, 0, -1), (1, 0.5, 1), far.T.reshape(-1).astype(F))
    assert hi[0] - lo[0] > 50.0 and (hi > lo).all()                                        # pad ~ 1e-5 x 3e6 on either side


# ---------------------------------------------------------------- GPU --------------------------------------------------------------------
def check_invariant(sc, top, original, rec, what):
    """The refit's rule, child by child, on a read-out `top` of a context whose instances hold the records `rec`; `original` is the
    read-out after the upload."""
    nodes, before = top["nodes"], original["nodes"]
    tn = top["top_nodes"]
    assert tn == original["top_nodes"] and np.array_equal(top["levels"], original["levels"])
    assert np.array_equal(nodes[:, 24:], before[:, 24:]), what + ": a child reference or a pad word changed"
    assert np.array_equal(nodes[tn:], before[tn:]), what + ": a mesh tree's node changed"
    assert np.array_equal(top["instances"][:, :32], rec.view(np.uint32)), what + ": the instance records are not the ones given"
    assert np.array_equal(top["instances"][:, 32:], original["instances"][:, 32:]) and np.array_equal(top["mesh_boxes"].view(np.uint32), original["mesh_boxes"].view(np.uint32))
    planes = nodes[:, :24].view(F).reshape(-1, 6, 4)                 # [node, plane (minx miny minz maxx maxy maxz), child]
    old = before[:, :24].reshape(-1, 6, 4)
    child = nodes[:, 24:28]
    meshes = top["instances"][:, 35]
    seen = np.zeros(len(rec), bool)
    for i in range(tn):
        for c in range(4):
            ref = int(child[i, c])
            got = planes[i, :, c].view(np.uint32)
            if ref == INVALID_CHILD:
                assert np.array_equal(got, old[i, :, c]), (what, "empty slot", i, c)
            elif ref & LEAF and (ref >> COUNT_SHIFT) & 15:
                assert np.array_equal(got, old[i, :, c]), (what, "triangle packet", i, c)
            elif ref & LEAF:
                k = ref & INDEX_MASK
                seen[k] = True
                mb = top["mesh_boxes"][meshes[k]]
                want = np.concatenate(binding.instance_world_box(mb[0, :3], mb[1, :3], rec[k, :16]))
                assert np.array_equal(got, want.view(np.uint32)), (what, "instance", k, planes[i, :, c], want)
                assert np.array_equal(top["boxes"][k, :, :3].reshape(-1).view(np.uint32), want.view(np.uint32)), (what, "instance box", k)
            else:
                assert i < ref < tn, (what, "inner child", i, c, ref)
                valid = child[ref] != INVALID_CHILD
                want = np.concatenate([planes[ref, :3][:, valid].min(axis=1), planes[ref, 3:][:, valid].max(axis=1)])
                assert np.array_equal(got, want.view(np.uint32)), (what, "inner child: not the union of node %d's children" % ref, i, c, planes[i, :, c], want)
    assert seen.all(), what + ": an instance is not a child of the top level"


def upload_and_read(ctx, sc):
    ctx.upload_scene(sc)
    return ctx.debug_top_level()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_identity_update_changes_no_bit(contexts, name):
    sc = base_scene(name)
    ctx = contexts()
    before = upload_and_read(ctx, sc)
    widths = np.diff(before["levels"])
    if name == "cornell":
        assert len(widths) >= 3
    if name == "grid":
        assert len(sc.instances) == 1250 and widths.max() > before["group_nodes"] >= widths.min(), "both paths of the refit must run: " + str(widths)
    check_invariant(sc, before, before, records(sc), name + " as uploaded")
    first = everything(ctx)
    ctx.set_instance_transforms(records(sc))
    assert ctx.instances_status() == 0
    assert_same_top(ctx.debug_top_level(), before, name + " identity")
    assert_same(everything(ctx), first, name + " identity")


@pytest.mark.gpu
@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", SCENES)
def test_moved_scene_equals_a_fresh_upload(contexts, name, move):
    sc = base_scene(name)
    ctx, fresh = contexts(), contexts(which=1)
    original = upload_and_read(ctx, sc)
    first = everything(ctx)
    rec, lo, count = moved(name, move)
    ctx.set_instance_transforms(rec[lo:lo + count], first=lo)
    assert ctx.instances_status() == 0
    top = ctx.debug_top_level()
    check_invariant(sc, top, original, rec, "%s %s" % (name, move))
    assert not np.array_equal(top["nodes"], original["nodes"])
    if move == "partial":
        outside = np.r_[0:lo, lo + count:len(rec)]
        assert np.array_equal(top["instances"][outside], original["instances"][outside]) and np.array_equal(top["boxes"][outside], original["boxes"][outside])
    got = everything(ctx)
    fresh_top = upload_and_read(fresh, with_records(sc, rec))
    want = everything(fresh)
    assert_same(got, want, "%s %s" % (name, move))
    assert np.array_equal(top["boxes"].view(np.uint32), fresh_top["boxes"].view(np.uint32)) and np.array_equal(np.delete(top["instances"], 32, axis=1), np.delete(fresh_top["instances"], 32, axis=1))      # (word 32: the mesh's root node, behind a top level of another size)
    assert np.isfinite(got["frame"]).all() and got["frame"].max() > 0
    # (a permutation among the placements of one mesh is the same set of surfaces: the same picture from other instances)
    assert not np.array_equal(got["hit_instances" if move == "permute" else "frame"], first["hit_instances" if move == "permute" else "frame"])
    if name == "lattice":
        frame, ctr = ob.load("oracle", abi.MODE_RGB).scene(with_records(sc, rec)).render(settings(), SPP)
        assert_bit_equal(got["frame"], frame, "lattice %s vs the oracle" % move)
        assert int(got["counters"][1]) == int(ctr.extension_rays) and int(got["counters"][2]) == int(ctr.shadow_rays)
    if move == "shrink_and_back":
        ctx.set_instance_transforms(records(sc))
        assert_same_top(ctx.debug_top_level(), original, name + " back")
        assert_same(everything(ctx), first, name + " back")


@pytest.mark.gpu
def test_spectral_context(contexts):
    sc = base_scene("cornell")
    ctx, fresh = contexts(abi.MODE_SPECTRAL), contexts(abi.MODE_SPECTRAL, 1)
    ctx.upload_scene(sc)
    rec = moved("cornell", "permute")[0]
    ctx.set_instance_transforms(rec)
    fresh.upload_scene(with_records(sc, rec))
    assert_same(everything(ctx), everything(fresh), "spectral cornell permute")


@pytest.mark.gpu
def test_coincident_placements_apart_and_back(contexts):
    sc = base_scene("lattice")
    rec = records(sc)
    assert np.array_equal(rec[0], rec[1])                      # the two terrains that coincide: ties across instances
    ctx, fresh = contexts(), contexts(which=1)
    original = upload_and_read(ctx, sc)
    first = everything(ctx)
    apart = rec.copy()
    apart[1:2] = translated(rec[1:2], [[0.0, 2.0, 0.0]])
    ctx.set_instance_transforms(apart[1:2], first=1)
    fresh.upload_scene(with_records(sc, apart))
    got = everything(ctx)
    assert_same(got, everything(fresh), "apart")
    assert not np.array_equal(got["hit_instances"], first["hit_instances"])
    ctx.set_instance_transforms(rec[1:2], first=1)
    assert_same_top(ctx.debug_top_level(), original, "back together")
    assert_same(everything(ctx), first, "back together")


@pytest.mark.gpu
def test_bad_records_leave_their_instances_and_set_the_status_bit(contexts):
    sc = base_scene("cornell")
    ctx, fresh = contexts(), contexts(which=1)
    original = upload_and_read(ctx, sc)
    rec = moved("cornell", "perturb")[0]
    batch = rec.copy()
    batch[5, 13] = np.nan                                      # a NaN in local_to_world
    batch[17, 16 + 7] = 0.25                                   # world_to_local's bottom row is not 0 0 0 1
    ctx.set_instance_transforms(batch)
    assert ctx.instances_status() == abi.INSTANCE_BAD_TRANSFORM
    assert ctx.instances_status() == 0                         # read and cleared
    applied = rec.copy()
    applied[[5, 17]] = records(sc)[[5, 17]]
    top = ctx.debug_top_level()
    assert np.array_equal(top["instances"][[5, 17]], original["instances"][[5, 17]]) and np.array_equal(top["boxes"][[5, 17]].view(np.uint32), original["boxes"][[5, 17]].view(np.uint32))
    good = np.setdiff1d(np.arange(len(rec)), [5, 17])
    assert not (top["instances"][good, :32] == original["instances"][good, :32]).all(axis=1).any()
    check_invariant(sc, top, original, applied, "bad records")
    fresh.upload_scene(with_records(sc, applied))
    assert_same(everything(ctx), everything(fresh), "bad records")
    inf = rec.copy()
    inf[0, 16 + 12] = np.inf
    ctx.set_instance_transforms(inf[:1])
    assert ctx.instances_status() == abi.INSTANCE_BAD_TRANSFORM
    assert np.array_equal(ctx.debug_top_level()["nodes"], top["nodes"])


@pytest.mark.gpu
def test_refusals_change_nothing(contexts):
    lib = binding.load_library()
    sc = base_scene("cornell")
    rec = moved("cornell", "perturb")[0]
    empty = Context(device=0)
    try:
        with pytest.raises(SlrHipError, match=r"slrhip_set_instance_transforms failed \(%d\)" % NO_SCENE):
            empty.set_instance_transforms(rec)
        with pytest.raises(SlrHipError, match=r"slrhip_set_camera failed \(%d\)" % NO_SCENE):
            empty.set_camera(sc.camera)
        assert empty.instances_status() == 0
        empty.upload_scene(base_scene("flat"))
        with pytest.raises(SlrHipError, match=r"slrhip_set_instance_transforms failed \(%d\).*no instances" % UNSUPPORTED):
            empty.set_instance_transforms(rec)
        with pytest.raises(SlrHipError, match=r"slrhip_debug_top_level failed \(%d\)" % UNSUPPORTED):
            empty.debug_top_level()
    finally:
        empty.close()
    ctx = contexts()
    before = upload_and_read(ctx, sc)
    first = everything(ctx)
    n = len(rec)
    with DeviceBlocks() as dev:
        p = dev.put(np.concatenate([rec.reshape(-1), np.zeros(64, F)]))
        for args, code in (((None, 0, n), INVALID), ((p + 4, 0, n), INVALID), ((p, 0, 0), INVALID), ((p, 0, n + 1), INVALID), ((p, n, 1), INVALID),
                           ((p, 1, 0xFFFFFFFF), INVALID)):
            assert lib.slrhip_set_instance_transforms(ctx.handle, *args, None) == code, args
            assert b"slrhip_set_instance_transforms" in lib.slrhip_last_error_string()
        assert lib.slrhip_set_camera(ctx.handle, None) == INVALID
        ctx.synchronize()
    assert ctx.instances_status() == 0
    assert_same_top(ctx.debug_top_level(), before, "after the refusals")
    assert_same(everything(ctx), first, "after the refusals")


def moved_camera(sc):
    """A moved, re-aimed thin-lens camera for the scene (lens radius > 0)."""
    old = np.array(sc.camera.local_to_world[:], np.float64).reshape(4, 4).T
    new = scenes._translate(0.15, 0.1, -0.2) @ old @ scenes._rotate(0.08, (0, 1, 0)) @ scenes._rotate(-0.05, (1, 0, 0))
    return scenes.make_camera(new, 1.0, 0.55, 0.03, 1.0, float(sc.camera.obj_plane_distance) * 0.9)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat", "cornell"])
def test_set_camera_equals_a_fresh_upload(contexts, name):
    sc = base_scene(name)
    cam = moved_camera(sc)
    assert cam.lens_radius > 0
    ctx, fresh = contexts(), contexts(which=1)
    ctx.upload_scene(sc)

    def look(c):
        c.render_begin(settings())
        c.render(0, SPP)
        k = c.counters()
        return dict(frame=c.read_framebuffer(), counters=np.array([k.samples, k.extension_rays, k.shadow_rays], np.uint64), rays=c.camera_rays(1)[0])
    first = look(ctx)
    ctx.set_camera(cam)
    got = look(ctx)
    fresh.upload_scene(with_records(sc, camera=cam))
    assert_same(got, look(fresh), name + " camera")
    assert not np.array_equal(got["rays"], first["rays"]) and not np.array_equal(got["frame"], first["frame"])
    ctx.set_camera(sc.camera)
    assert_same(look(ctx), first, name + " camera back")
    if name == "cornell":
        # the camera and the placements in one frame
        rec = moved("cornell", "perturb")[0]
        ctx.set_camera(cam)
        ctx.set_instance_transforms(rec)
        fresh.upload_scene(with_records(sc, rec, camera=cam))
        assert_same(everything(ctx), everything(fresh), "camera and placements")


@pytest.mark.gpu
def test_traversal_counts_after_an_identity_update(contexts):
    sc = base_scene("grid")
    ctx, fresh = contexts(flags=abi.FLAG_COUNT_TRAVERSAL), contexts(which=1, flags=abi.FLAG_COUNT_TRAVERSAL)
    ctx.upload_scene(sc)
    ctx.set_instance_transforms(records(sc))
    fresh.upload_scene(sc)
    out = []
    for c in (ctx, fresh):
        c.render_begin(settings())
        c.render(0, SPP)
        p = c.profile()
        out.append((list(p.nodes), list(p.triangles), list(p.rays)))
    assert out[0] == out[1] and sum(out[0][0]) > 0, out


# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process: the check on a torch tensor runs in
# a fresh child process that imports torch BEFORE libslrhip.so is loaded.
@pytest.mark.gpu
def test_device_tensor_and_numpy_array_give_the_same_read_out():
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_instance_update as T\nT._torch_check()\n" % (ROOT, os.path.join(ROOT, "tests")))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert "OK _torch_check" in p.stdout, p.stdout[-4000:] + "\n" + p.stderr[-3000:]


def _torch_check():
    import torch
    sc = base_scene("grid")
    rec = moved("grid", "permute")[0]
    ctx = Context(device=0)
    try:
        ctx.upload_scene(sc)
        ctx.set_instance_transforms(rec)
        want = ctx.debug_top_level()
        ctx.set_instance_transforms(records(sc))                  # back, in between
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            t = torch.from_numpy(rec.copy()).cuda()
            ctx.set_instance_transforms(t, stream=side)
            t.zero_()                                             # ordered after the call on the same stream: the kernels have read it
        assert ctx.instances_status(side) == 0
        assert_same_top(ctx.debug_top_level(), want, "torch tensor")
        with pytest.raises(ValueError):
            ctx.set_instance_transforms(t[:, ::2])                # not [n, 32]
        print("OK _torch_check", flush=True)
    finally:
        ctx.close()
