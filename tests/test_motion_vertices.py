"""Motion vectors of moved vertices (slrhip_render_motion_vertices, slrhip_motion_sample_vertices, slrhip_debug_motion_vertices_check).

CPU: the descriptor's layout and the exports; every refusal through the context-free check; slrhip_motion_sample_vertices — the function
the fold kernel calls — bit for bit against a numpy float32 restatement of include/slrhip.h's definition; exactly zero motion where
nothing moved; invalid samples.

GPU: previous_vertices NULL is slrhip_render_motion; the current vertices named as the previous ones give motion exactly zero; after
set_vertices the buffer equals, bit for bit, the restatement summed in pass order over the library's own camera rays and closest hits;
the buffer is independent of shards, cuts, colour mode and interleaved calls; an updated context equals a fresh one; and — independent of
the restatement — a ray of the previous camera through now_pixel + m hits, in a context that holds the PREVIOUS vertices, the same
triangle.  Buffers are compared by bits; the only tolerance is the relative 1e-3 of the last check, the existing test's own."""
import ctypes as C
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import test_motion as M
import test_vertex_update as V
import test_vertex_update_instanced as VI
from helpers import _local_ray, assert_bit_equal
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, DeviceBlocks

ROOT = M.ROOT
F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
SIZE, SPP = M.SIZE, M.SPP
DYNAMIC, INSTANCED, SPLITS = abi.FLAG_DYNAMIC_GEOMETRY, abi.FLAG_DYNAMIC_INSTANCED, abi.FLAG_BVH_SPATIAL_SPLITS
BOTH = DYNAMIC | INSTANCED
TREE_HOST_SAH, TREE_SPATIAL_SPLITS, TREE_INSTANCED = 0, 1, 3
f32, np_mul_point, np_project, records, settings = M.f32, M.np_mul_point, M.np_project, M.records, M.settings
SCENES = ["flat", "lattice", "cornell", "nine"]


@functools.lru_cache(maxsize=None)
def base_scene(name):
    return VI.base_scene("nine") if name == "nine" else M.base_scene(name)


def flags_of(name):
    return DYNAMIC if name == "flat" else BOTH


def perturbed(name):
    """The `perturb` move of test_vertex_update.py (flat) and test_vertex_update_instanced.py: a seeded random displacement per vertex."""
    return V.perturbed("cornell") if name == "flat" else VI.perturbed(name)


def with_vertices(name, vertices):
    sc = base_scene(name)
    return V.with_vertices(sc, vertices) if name == "flat" else VI.with_scene(sc, vertices)


# ---- the restatement of the definition, float32, every intermediate checked ------------------------------------------------------------
def np_motion_vertices(mc_now, mc_prev, rec_now, rec_prev, inst, width, height, pos_now, pos_prev, b1, b2):
    """Per sample {m.x, m.y, z', valid} [n, 4].  pos_now / pos_prev [n, 3 vertices, 3]: the positions of the hit triangle's vertices now
    and in the previous frame; b1, b2 [n]: Moller-Trumbore's barycentrics; inst [n] the instance hit (-1: a loose triangle); rec_now /
    rec_prev [instances, 32] the placements (None: the scene has none)."""
    f32(pos_now, pos_prev, b1, b2)
    with np.errstate(all="ignore"):
        b0 = f32(f32(F(1.0) - b1) - b2)

        def local(p):
            return f32(f32(f32(b0[:, None] * p[:, 0]) + f32(b1[:, None] * p[:, 1])) + f32(b2[:, None] * p[:, 2]))
        l_now, l_prev = local(pos_now), local(pos_prev)
    loose = inst < 0 if rec_now is not None else np.ones(len(b1), bool)
    p_now, p_prev = l_now, l_prev
    if rec_now is not None and (~loose).any():
        k = np.maximum(inst, 0)
        p_now = np.where(loose[:, None], l_now, np_mul_point(rec_now[k, :16], l_now))
        p_prev = np.where(loose[:, None], l_prev, np_mul_point(rec_prev[k, :16], l_prev))
    ok_now, x_now, y_now = np_project(mc_now, f32(p_now), width, height)
    ok_prev, x_prev, y_prev = np_project(mc_prev, f32(p_prev), width, height)
    valid = ok_now & ok_prev
    with np.errstate(all="ignore"):
        d = f32(p_prev - mc_prev[16:19])
        z = f32(np.sqrt(f32(f32(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])))
        out = np.stack([f32(x_prev - x_now), f32(y_prev - y_now), z, np.ones(len(b1), F)], axis=1)
    return f32(np.where(valid[:, None], out, F(0.0)))


def np_barycentrics(rows, inst, rec_now, pos):
    """Moller-Trumbore's (b1, b2) [n] of ray k of `rows` (slrhip_ray rows) against ITS triangle pos[k] ([n, 3, 3], local space), as
    helpers._moller_trumbore states the kernels' triangle test (pt_traverse.h): the ray goes into the instance's local space first
    (helpers._local_ray), e1 = p1 - p0, e2 = p2 - p0, cross is a.y b.z - a.z b.y .., dot is (x + y) + z, invDet = 1 / det."""
    org, dirn = np.ascontiguousarray(rows[:, 0:3]), np.ascontiguousarray(rows[:, 4:7])
    if rec_now is not None:
        k = np.maximum(inst, 0)
        o, d = _local_ray(np.ascontiguousarray(rec_now[k, 16:].T), org, dirn)
        org, dirn = np.where((inst < 0)[:, None], org, o), np.where((inst < 0)[:, None], dirn, d)
    with np.errstate(all="ignore"):
        v0, e1, e2 = pos[:, 0], f32(pos[:, 1] - pos[:, 0]), f32(pos[:, 2] - pos[:, 0])
        dx, dy, dz = dirn[:, 0], dirn[:, 1], dirn[:, 2]
        px, py, pz = dy * e2[:, 2] - dz * e2[:, 1], dz * e2[:, 0] - dx * e2[:, 2], dx * e2[:, 1] - dy * e2[:, 0]
        det = (e1[:, 0] * px + e1[:, 1] * py) + e1[:, 2] * pz
        inv = F(1.0) / det
        sx, sy, sz = org[:, 0] - v0[:, 0], org[:, 1] - v0[:, 1], org[:, 2] - v0[:, 2]
        b1 = ((sx * px + sy * py) + sz * pz) * inv
        qx, qy, qz = sy * e1[:, 2] - sz * e1[:, 1], sz * e1[:, 0] - sx * e1[:, 2], sx * e1[:, 1] - sy * e1[:, 0]
        b2 = ((dx * qx + dy * qy) + dz * qz) * inv
    return f32(b1, b2)


# ---------------------------------------------------------------- CPU --------------------------------------------------------------------
def test_layout_exports_and_version():
    lib = binding.load_library()
    for name in ("slrhip_render_motion_vertices", "slrhip_motion_sample_vertices", "slrhip_debug_motion_vertices_check"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    d = abi.MotionVerticesDesc
    assert C.sizeof(d) == 40 and (d.frame.offset, d.previous_vertices.offset, d.reserved.offset) == (0, 24, 32)
    assert C.sizeof(abi.MotionDesc) == 24 and lib.slrhip_version() == 7
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    for text in ("#define SLRHIP_VERSION 7 ", "typedef struct slrhip_motion_vertices_desc {", "b0 = (1.0f - b1) - b2",
                 "l_now = (b0 * p0 + b1 * p1) + b2 * p2", "l_prev = (b0 * q0 + b1 * q1) + b2 * q2", "CANNOT check how long the caller's array is",
                 "covered by slrhip_render_motion_vertices below", "slrhip_render_motion_vertices takes the previous frame's vertex array"):
        assert text in header, text
    source = open(os.path.join(ROOT, "slr_amd", "csrc", "pt_motion.hip")).read()
    assert "motionSampleVertices(" in source and "motionSampleVertices(" in open(os.path.join(ROOT, "slr_amd", "csrc", "host_util.cpp")).read()


def check(lib, have_render=1, num_instances=0, flags=DYNAMIC, builder=TREE_HOST_SAH, desc=True, camera=None, transforms=None, frame_reserved=(0, 0),
          vertices=4096, reserved=0, begin=3, count=5):
    frame = abi.MotionDesc(C.pointer(camera) if camera is not None else None, transforms, (C.c_uint32 * 2)(*frame_reserved))
    d = abi.MotionVerticesDesc(frame, vertices, reserved)
    rc = lib.slrhip_debug_motion_vertices_check(have_render, num_instances, flags, builder, C.byref(d) if desc else None, begin, count)
    return rc, lib.slrhip_last_error_string().decode()


WITHOUT_GEOMETRY = "previous_vertices given, but the context was created without SLRHIP_FLAG_DYNAMIC_GEOMETRY"
WITHOUT_INSTANCED = "previous_vertices given, but the scene has instances and the context was created without SLRHIP_FLAG_DYNAMIC_INSTANCED"
REFUSALS = [("null descriptor", dict(desc=False), INVALID, "null descriptor"),
            ("outer reserved", dict(reserved=1), INVALID, "reserved must be 0"),
            ("outer reserved, high word", dict(reserved=1 << 40), INVALID, "reserved must be 0"),
            ("misaligned vertices", dict(vertices=4096 + 2), INVALID, "misaligned previous_vertices (4 bytes)"),
            ("frame reserved[0]", dict(frame_reserved=(1, 0)), INVALID, "reserved must be 0"),
            ("frame reserved[1]", dict(frame_reserved=(0, 7)), INVALID, "reserved must be 0"),
            ("misaligned transforms", dict(transforms=4096 + 8, num_instances=6, flags=BOTH, builder=TREE_INSTANCED), INVALID,
             "misaligned previous_transforms (16 bytes)"),
            ("transforms without instances", dict(transforms=4096), INVALID, "previous_transforms given, but the scene has no instances"),
            ("pass range", dict(begin=0xFFFFFFF0, count=0x10), INVALID, "pass range beyond 2^32"),
            ("no render state", dict(have_render=0), NO_SCENE, "call slrhip_render_begin first"),
            ("no flag, flat", dict(flags=0), UNSUPPORTED, WITHOUT_GEOMETRY),
            ("no flag, instanced", dict(flags=0, num_instances=6, builder=TREE_INSTANCED), UNSUPPORTED, WITHOUT_GEOMETRY),
            ("the instanced flag alone", dict(flags=INSTANCED, num_instances=6, builder=TREE_INSTANCED), UNSUPPORTED, WITHOUT_GEOMETRY),
            ("instances without the instanced flag", dict(flags=DYNAMIC, num_instances=6, builder=TREE_INSTANCED), UNSUPPORTED, WITHOUT_INSTANCED),
            ("spatial splits", dict(flags=DYNAMIC | SPLITS, builder=TREE_SPATIAL_SPLITS), UNSUPPORTED,
             "previous_vertices given, but the tree was built with spatial splits")]


@pytest.mark.parametrize("what, over, code, text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_through_the_check(what, over, code, text):
    lib = binding.load_library()
    rc, message = check(lib, **over)
    assert rc == code and message == "slrhip_render_motion_vertices: " + text, (what, rc, message)
    assert "SLRHIP_FLAG_DYNAMIC_" in message or code != UNSUPPORTED or what == "spatial splits"


def test_calls_that_pass_the_check_and_null_arguments():
    lib = binding.load_library()
    cam = scenes.cornell_camera(1.0)
    assert check(lib, flags=0, vertices=None)[0] == 0, "NULL previous_vertices in an unflagged context"
    assert check(lib, flags=0, vertices=None, num_instances=6, builder=TREE_INSTANCED, transforms=4096, camera=cam)[0] == 0
    assert check(lib, flags=DYNAMIC | SPLITS, builder=TREE_SPATIAL_SPLITS, vertices=None)[0] == 0
    assert check(lib, flags=DYNAMIC, camera=cam)[0] == 0, "a flagged flat scene"
    assert check(lib, flags=BOTH, num_instances=6, builder=TREE_INSTANCED, transforms=4096, camera=cam)[0] == 0, "a flagged instanced scene"
    assert check(lib, flags=BOTH, vertices=4096 + 4, begin=0, count=0xFFFFFFFF)[0] == 0, "4-byte alignment; the whole pass range"
    d = abi.MotionVerticesDesc(abi.MotionDesc(None, None, (C.c_uint32 * 2)(0, 0)), None, 0)
    assert lib.slrhip_render_motion_vertices(None, C.byref(d), 0, 1, None) == INVALID
    nine, four = np.zeros(9, F), np.zeros(4, F)
    for args in ((None, cam, nine, nine, four), (cam, None, nine, nine, four), (cam, cam, None, nine, four), (cam, cam, nine, None, four),
                 (cam, cam, nine, nine, None)):
        a, b = (C.byref(c) if c is not None else None for c in args[:2])
        ptrs = [None if p is None else p.ctypes.data for p in args[2:]]
        assert lib.slrhip_motion_sample_vertices(a, b, None, None, 4, 4, ptrs[0], ptrs[1], 0.25, 0.25, ptrs[2]) == INVALID


@functools.lru_cache(maxsize=None)
def sample_inputs(n=2048):
    """Random triangles around points in and beyond the view of test_motion.py's camera pairs, now and moved; random barycentrics with
    the corners and edges among them; a pair of placements per sample."""
    rng = np.random.default_rng(41)
    now = scenes._lattice_camera(8)
    m = M.camera_matrix(now)
    local = np.stack([rng.uniform(-12, 12, n), rng.uniform(-9, 9, n), rng.uniform(0.5, 30, n)], axis=1)
    centre = local @ m[:3, :3].T + m[:3, 3]
    pos_now = (centre[:, None, :] + rng.uniform(-1.0, 1.0, (n, 3, 3))).astype(F)
    pos_prev = (pos_now.astype(np.float64) + rng.uniform(-0.5, 0.5, (n, 3, 3))).astype(F)
    b1 = rng.uniform(0, 1, n).astype(F)
    b2 = (rng.uniform(0, 1, n) * (1.0 - b1.astype(np.float64))).astype(F)
    b1[:6], b2[:6] = [0, 1, 0, 0, 0.5, 0.25], [0, 0, 1, 0.5, 0, 0.75]          # the corners, b1 = 0, b2 = 0, b1 + b2 = 1
    base = records(scenes.lattice_instanced())
    rec_now = np.ascontiguousarray(base[rng.integers(0, len(base), n)])
    rec_prev = np.ascontiguousarray(M.placed(rec_now, rng.uniform(-0.5, 0.5, (n, 3)), 0.5, 0.05))
    return pos_now, pos_prev, b1, b2, rec_now, rec_prev


def library_samples(now, prev, rec_now, rec_prev, w, h, pos_now, pos_prev, b1, b2):
    out = np.zeros((len(b1), 4), F)
    for k in range(len(b1)):
        out[k] = binding.motion_sample_vertices(now, prev, None if rec_now is None else rec_now[k], None if rec_prev is None else rec_prev[k], w, h,
                                                pos_now[k], pos_prev[k], b1[k], b2[k])
    return out


@pytest.mark.parametrize("pair", M.CAMERA_PAIRS)
def test_sample_equals_the_restatement(pair):
    now, prev = M.camera_pair(pair)
    mc_now, mc_prev = binding.motion_camera(now), binding.motion_camera(prev)
    pos_now, pos_prev, b1, b2, rec_now, rec_prev = sample_inputs()
    n, w, h = len(b1), 37, 21
    inst, none = np.arange(n), np.full(n, -1)
    for what, pp in (("moved vertices", pos_prev), ("unmoved vertices", pos_now)):
        loose = np_motion_vertices(mc_now, mc_prev, None, None, none, w, h, pos_now, pp, b1, b2)
        if pair == "behind":
            assert 0.05 <= (loose[:, 3] == 0).mean() <= 0.95, "the input condition: a share of the samples is not valid, a share is"
        else:
            assert (loose[:, 3] == 1).mean() >= 0.25
        assert_bit_equal(library_samples(now, prev, None, None, w, h, pos_now, pp, b1, b2), loose, "loose, " + what)
        assert_bit_equal(library_samples(now, prev, None, rec_prev, w, h, pos_now, pp, b1, b2), loose, "a loose triangle reads no record, " + what)
        moved = np_motion_vertices(mc_now, mc_prev, rec_now, rec_prev, inst, w, h, pos_now, pp, b1, b2)
        assert (moved[:, 3] == 1).mean() >= 0.05 and not (moved[:, :3] == loose[:, :3]).all()
        assert_bit_equal(library_samples(now, prev, rec_now, rec_prev, w, h, pos_now, pp, b1, b2), moved, "moved records, " + what)
        same = np_motion_vertices(mc_now, mc_prev, rec_now, rec_now.copy(), inst, w, h, pos_now, pp, b1, b2)
        assert_bit_equal(library_samples(now, prev, rec_now, rec_now.copy(), w, h, pos_now, pp, b1, b2), same, "bit-equal records, " + what)
        assert_bit_equal(library_samples(now, prev, rec_now, None, w, h, pos_now, pp, b1, b2), same, "no previous record, " + what)
    changed = np_motion_vertices(mc_now, mc_prev, None, None, none, w, h, pos_now, pos_prev, b1, b2)
    both = (changed[:, 3] == 1) & (loose[:, 3] == 1)
    assert (np.abs(changed[both, :2] - loose[both, :2]).max(axis=1) > 0.05).mean() >= 0.5, "the input condition: moved vertices move the vectors"


def test_equal_positions_records_and_cameras_give_exactly_zero():
    now, _ = M.camera_pair("identical")
    pos_now, _, b1, b2, rec_now, _ = sample_inputs()
    for rn, rp in ((None, None), (rec_now, rec_now.copy()), (rec_now, None)):
        got = library_samples(now, now, rn, rp, 37, 21, pos_now, pos_now.copy(), b1, b2)
        assert (got[:, 3] == 1).mean() >= 0.05 and (got[:, 0] == 0).all() and (got[:, 1] == 0).all()
        assert (got[got[:, 3] == 1, 2] > 0).all()


def test_invalid_inputs_give_zeros():
    now, prev = M.camera_pair("moved")
    pos_now, pos_prev, b1, b2, rec_now, rec_prev = (a[:64] for a in sample_inputs())
    ok = library_samples(now, prev, rec_now, rec_prev, 37, 21, pos_now, pos_prev, b1, b2)[:, 3] == 1
    assert ok[6:].mean() >= 0.25
    for bad in (np.nan, np.inf, -np.inf):
        for vertex in range(3):
            pp = pos_prev.copy()
            pp[:, vertex, vertex] = bad                     # one coordinate of one vertex; at a corner its weight may be 0: 0 * inf is a NaN
            for rn, rp in ((None, None), (rec_now, rec_prev)):
                got = library_samples(now, prev, rn, rp, 37, 21, pos_now, pp, b1, b2)
                assert (got == 0).all(), (bad, vertex)
    # a point behind the previous camera: the previous triangle mirrored through the previous lens centre
    centre = binding.motion_camera(prev)[16:19]
    behind = (2.0 * centre.astype(np.float64) - pos_prev.astype(np.float64)).astype(F)
    got = library_samples(now, prev, None, None, 37, 21, pos_now, behind, b1, b2)
    assert ok.any() and (got[ok] == 0).all()


# ---------------------------------------------------------------- GPU --------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(flags=0, which=0, mode=abi.MODE_RGB):
        key = (flags, which, mode)
        if key not in made:
            made[key] = Context(device=0, mode=mode, flags=flags)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def motion_of(ctx, st, calls, prev_cam=None, prev_rec=None, prev_vertices=None, shard=(0, 1)):
    ctx.render_begin(st, shard)
    for begin, count in calls:
        ctx.render_motion(count, prev_cam, prev_rec, spp_begin=begin, previous_vertices=prev_vertices)
    out = ctx.motion()
    assert ctx.features_status() == 0
    return out


def through_the_new_entry_point_with_null(ctx, st, passes, prev_cam, prev_rec):
    """slrhip_render_motion_vertices with previous_vertices NULL (Context.render_motion would take the old entry point)."""
    ctx.render_begin(st)
    with DeviceBlocks() as dev:
        frame = abi.MotionDesc(C.pointer(prev_cam) if prev_cam is not None else None, dev.put(prev_rec) if prev_rec is not None else None,
                               (C.c_uint32 * 2)(0, 0))
        d = abi.MotionVerticesDesc(frame, None, 0)
        assert ctx.lib.slrhip_render_motion_vertices(ctx.handle, C.byref(d), 0, passes, None) == 0, ctx.lib.slrhip_last_error_string()
        ctx.synchronize()
    out = ctx.motion()
    assert ctx.features_status() == 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat", "lattice", "cornell"])
def test_null_previous_vertices_is_the_old_call(contexts, name):
    sc = base_scene(name)
    prev_rec, prev_cam = M.previous_frame(name) if name != "flat" else (None, M.moved_camera(sc.camera, (0.05, -0.03, 0.06), 0.03))
    st = settings()
    for flags in (0, flags_of(name)):
        ctx = contexts(flags)
        ctx.upload_scene(sc)
        want = M.motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec)
        assert (want[..., 3] > 0).mean() >= 0.25 and (np.abs(want[..., :2]) > 0).mean() >= 0.25
        assert_bit_equal(through_the_new_entry_point_with_null(ctx, st, SPP, prev_cam, prev_rec), want, "%s, flags %d" % (name, flags))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_nothing_moved_is_exactly_zero(contexts, name):
    sc = base_scene(name)
    ctx = contexts(flags_of(name))
    ctx.upload_scene(sc)
    st = settings()
    ctx.render_begin(st)
    ctx.render_features(abi.FEATURE_COVERAGE, SPP)
    coverage = ctx.features(abi.FEATURE_COVERAGE)
    assert (coverage > 0).mean() >= 0.25
    implicit = motion_of(ctx, st, [(0, SPP)], prev_vertices=sc.vertices)
    explicit = motion_of(ctx, st, [(0, SPP)], sc.camera, records(sc) if len(sc.instances) else None, sc.vertices)
    for what, got in (("the current vertices alone", implicit), ("the whole current frame passed as the previous one", explicit)):
        assert (got[..., 0] == 0).all() and (got[..., 1] == 0).all(), what
        assert (got[..., 3].view(np.uint32) == coverage.view(np.uint32)).all(), what
        assert np.isfinite(got[..., 2]).all() and (got[..., 2][coverage > 0] > 0).all(), what
    assert_bit_equal(implicit, explicit, "both ways of saying that nothing moved")


def restated_motion(ctx, sc, st, passes, prev_cam, prev_rec, prev_vertices, want_samples=False):
    """The buffer from the library's own camera rays and closest hits (existing calls), pass by pass, summed in pass order.  The context
    holds `sc` (its vertices are the kept array as it now stands) and has begun a render with `st`.  The closest-hit call reports
    (b0, b1) and not b2: b2 is restated from the ray and the triangle (np_barycentrics), and that restatement is held against what the
    call does report — b1 and b0 = (1 - b1) - b2, bit for bit — before it is used."""
    w, h = st.image_width, st.image_height
    mc_now = binding.motion_camera(sc.camera)
    mc_prev = binding.motion_camera(prev_cam) if prev_cam is not None else mc_now
    rec_now = records(sc) if len(sc.instances) else None
    rec_prev = rec_now if prev_rec is None else prev_rec
    tri, pos_now, pos_prev = sc.triangles["v"], sc.vertices["position"].astype(F), prev_vertices["position"].astype(F)
    acc = np.zeros((h, w, 4), F)
    samples, hit_ids = np.zeros((passes, h, w, 4), F), np.full((passes, h, w, 2), -1, np.int64)
    for p in range(passes):
        rows, xy = ctx.camera_rays(p)
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        t = hits.view(np.uint32)[:, 0]
        hit = t != abi.MISS
        idx = tri[np.where(hit, t, 0)]
        b1, b2 = np_barycentrics(rows, inst.astype(np.int64), rec_now, pos_now[idx])
        with np.errstate(all="ignore"):
            b0 = f32(f32(F(1.0) - b1) - b2)
        assert (b1[hit].view(np.uint32) == hits[hit, 3].view(np.uint32)).all() and (b0[hit].view(np.uint32) == hits[hit, 2].view(np.uint32)).all(), \
            "the restated barycentrics are not the traversal's"
        b1, b2 = np.where(hit, b1, F(0.0)), np.where(hit, b2, F(0.0))
        out = np_motion_vertices(mc_now, mc_prev, rec_now, rec_prev, inst.astype(np.int64), w, h, pos_now[idx], pos_prev[idx], f32(b1), f32(b2))
        out = np.where(hit[:, None], out, F(0.0))
        x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
        acc[y, x] = f32(acc[y, x] + out)
        samples[p, y, x] = out
        hit_ids[p, y, x, 0], hit_ids[p, y, x, 1] = np.where(hit, inst, -2), np.where(hit, t.astype(np.int64), -1)
    return (acc, samples, hit_ids) if want_samples else acc


MOVED = [("flat", False), ("lattice", False), ("nine", False), ("lattice", True)]


@functools.lru_cache(maxsize=None)
def moved_case(name, everything):
    """(the scene now: the base scene with perturbed vertices, the previous camera, records and vertices).  everything: the instances and
    the camera moved as well (test_motion.py's previous_frame); else only the vertices."""
    sc = base_scene(name)
    prev_rec, prev_cam = M.previous_frame(name) if everything else (None, None)
    return with_vertices(name, perturbed(name)), prev_cam, prev_rec, sc.vertices


def moved_context(contexts, name, which=0, mode=abi.MODE_RGB):
    """A flagged context that uploaded the base scene and then moved its vertices."""
    ctx = contexts(flags_of(name), which, mode)
    ctx.upload_scene(base_scene(name))
    ctx.set_vertices(perturbed(name))
    assert ctx.geometry_status() == 0
    return ctx


@pytest.fixture(scope="module")
def moved_buffers():
    return {}


@pytest.mark.gpu
@pytest.mark.parametrize("name, everything", MOVED, ids=["%s%s" % (n, "+frame" if e else "") for n, e in MOVED])
def test_moved_scene_equals_the_restatement(contexts, moved_buffers, name, everything):
    now, prev_cam, prev_rec, prev_vertices = moved_case(name, everything)
    ctx = moved_context(contexts, name)
    st = settings()
    ctx.render_begin(st)
    want, samples, ids = restated_motion(ctx, now, st, SPP, prev_cam, prev_rec, prev_vertices, want_samples=True)
    hit, valid = ids[..., 1] >= 0, samples[..., 3] == 1
    length = np.hypot(samples[..., 0], samples[..., 1])
    print("%s/%s: hit samples %.3f, of them valid %.3f, of them |m| > 0.05 px %.3f, mean |m| %.2f px"
          % (name, everything, hit.mean(), valid[hit].mean(), (length[valid] > 0.05).mean(), length[valid].mean()))
    assert hit.mean() >= 0.25 and valid[hit].mean() >= 0.9 and (length[valid] > 0.05).mean() >= 0.5, "the input conditions"
    got = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, prev_vertices)
    assert_bit_equal(got, want, "%s/%s" % (name, everything))
    moved_buffers[(name, everything)] = got
    with DeviceBlocks() as dev:
        ctx.render_begin(st)
        ctx.render_motion(SPP, prev_cam, dev.put(prev_rec) if prev_rec is not None else None,
                          previous_vertices=dev.put(np.ascontiguousarray(prev_vertices).view(F).reshape(-1, 11)))
        assert_bit_equal(ctx.motion(), want, "previous_vertices as a device address")


@pytest.mark.gpu
def test_independence_of_shards_cuts_window_mode_and_interleaving(contexts):
    name = "lattice"
    now, prev_cam, prev_rec, prev_vertices = moved_case(name, True)
    st = settings()
    ctx = moved_context(contexts, name)
    whole = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, prev_vertices)
    assert (whole[..., 3] > 0).mean() >= 0.25 and (np.abs(whole[..., :2]) > 0).mean() >= 0.25
    halves = [motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, prev_vertices, shard=(k, 2)) for k in range(2)]
    assert ((halves[0][..., 3] > 0) & (halves[1][..., 3] > 0)).sum() == 0 and (halves[0][..., 3] > 0).any() and (halves[1][..., 3] > 0).any()
    assert_bit_equal(halves[0] + halves[1], whole, "two shards add up to the whole image")
    assert_bit_equal(motion_of(ctx, st, [(0, 3), (3, 5)], prev_cam, prev_rec, prev_vertices), whole, "8 passes = 3 + 5")
    assert_bit_equal(motion_of(ctx, st, [(0, 70)], prev_cam, prev_rec, prev_vertices),
                     motion_of(ctx, st, [(0, 64), (64, 6)], prev_cam, prev_rec, prev_vertices), "70 passes in one call (two windows) = 64 + 6")
    spectral = moved_context(contexts, name, mode=abi.MODE_SPECTRAL)
    assert_bit_equal(motion_of(spectral, st, [(0, SPP)], prev_cam, prev_rec, prev_vertices), whole, "a spectral context")

    # a render interleaved with the new motion calls, feature and albedo calls: the frame and the counters of a render without them
    def frame(interleave):
        ctx.render_begin(st)
        if interleave:
            ctx.render_motion(3, prev_cam, prev_rec, previous_vertices=prev_vertices)
        ctx.render(0, 4)
        if interleave:
            ctx.render_features(abi.FEATURE_COVERAGE, 2)
            ctx.render_albedo(2)
            ctx.render_motion(5, prev_cam, prev_rec, spp_begin=3, previous_vertices=prev_vertices)
        ctx.render(4, 4)
        k = ctx.counters()
        got = (ctx.read_framebuffer(), (k.samples, k.extension_rays, k.shadow_rays))
        if interleave:
            assert_bit_equal(ctx.motion(), whole, "motion calls between renders")
        return got
    alone, mixed = frame(False), frame(True)
    assert (alone[0].view(np.uint32) == mixed[0].view(np.uint32)).all() and alone[1] == mixed[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["flat", "nine"])
def test_updated_context_equals_a_fresh_one(contexts, name):
    now, _, _, prev_vertices = moved_case(name, False)
    st = settings()
    got = motion_of(moved_context(contexts, name), st, [(0, SPP)], prev_vertices=prev_vertices)
    fresh = contexts(flags_of(name), 1)
    fresh.upload_scene(now)
    want = motion_of(fresh, st, [(0, SPP)], prev_vertices=prev_vertices)
    assert (want[..., 3] > 0).mean() >= 0.25 and (np.abs(want[..., :2]) > 0).mean() >= 0.25
    assert_bit_equal(got, want, name)


def smooth_case(name):
    """(the vertices now, the vertices of the previous frame) for the check against the previous frame's triangles: the uploaded scene is
    the current frame; in the previous frame every vertex stood LOWER in its own local space, by a smooth wave of its local x and z —
    0 .. amplitude, never above.  Smooth, so that neighbouring triangles stay joined (the random `perturb` move tears them apart and the
    rips hide points by a hair); never above, because of what test_motion.py's `lifted` placement is for: the lattice's 2-box stands IN
    the terrain with its top in the plane of the terrain's quads, and a terrain that stood higher against the box than it does now
    would have hidden points of the box's face from a hair in front of them."""
    sc = base_scene(name)
    amplitude, period = (0.6, 5.0) if name == "lattice" else (0.04, 0.7)
    prev = sc.vertices.copy()
    # the lattice: the terrain mesh alone (the first mesh placed); the box and the loose walls stand still
    chosen = VI.vertex_sets(name)[1][0] if name == "lattice" else np.arange(len(prev))
    p = prev["position"][chosen].astype(np.float64)
    wave = 0.25 * (1.0 - np.cos(2.0 * math.pi * p[:, 0] / period)) * (1.0 - np.cos(2.0 * math.pi * p[:, 2] / period))
    p[:, 1] -= amplitude * wave
    prev["position"][chosen] = p.astype(F)
    return sc.vertices, prev


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lattice", "flat"])
def test_vectors_point_at_the_same_triangle_of_the_previous_frame(contexts, name):
    """Independent of the restatement: for every valid sample the previous camera's pinhole ray through now_pixel + m, built in float64,
    is traced in a second context that holds the PREVIOUS vertices.  It must hit the same triangle of the same instance, unless the
    previous scene's hit is nearer than z' (1 - 1e-3): the point was hidden then; where it hits the same triangle, its distance agrees
    with z' to the same relative 1e-3.  The camera moved as well.  (The flat scene is taken behind a pinhole: see below.)
    Measured on MI355X (4 passes of 32 x 32 = 4 096 samples).  lattice: valid 2 150 (52 %); of them the same triangle 1 974 (92 %), hidden
    176 (8 %), unexplained 0; moved by the vertices by more than 0.05 px 1 223 (57 %).  flat: valid 4 096 (100 %); the same triangle 4 085
    (99.7 %), hidden 11 (0.3 %), unexplained 0; moved 2 284 (56 %)."""
    passes = 4
    sc = base_scene(name)
    if sc.camera.lens_radius != 0.0:
        # the flat scene's camera has a lens; the check needs a pinhole (the projection through the lens centre then inverts the camera
        # sample, and a ray's direction says where on the image it is): the same scene behind the same camera with lens radius 0
        c = sc.camera
        sc = abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data,
                       scenes.make_camera(M.camera_matrix(c), c.aspect, c.fov_y, 0.0, c.img_plane_distance, c.obj_plane_distance, c.sensitivity), None,
                       sc.name + "_pinhole")
    assert sc.camera.lens_radius == 0.0 and len(sc.textures) == 0
    _, prev_vertices = smooth_case(name)
    prev_cam = M.moved_camera(sc.camera, (0.3, -0.2, 0.4) if name == "lattice" else (0.05, -0.03, 0.06), 0.03)
    st = settings(seed=3)
    w, h = st.image_width, st.image_height
    ctx = contexts(flags_of(name))
    ctx.upload_scene(sc)
    yard = contexts(flags_of(name), 1)
    yard.upload_scene(with_vertices(name, prev_vertices))      # (its camera is not used: the rays are built here)
    yard.render_begin(st)

    def f64(cam):
        l2w = M.camera_matrix(cam)
        w2l = np.array(cam.world_to_local[:], np.float64).reshape(4, 4).T
        op_h = 2.0 * cam.obj_plane_distance * math.tan(0.5 * cam.fov_y)
        return l2w, w2l, op_h * cam.aspect, op_h, float(cam.obj_plane_distance)
    l2w_n, w2l_n, opw_n, oph_n, obj_n = f64(sc.camera)
    l2w_p, w2l_p, opw_p, oph_p, obj_p = f64(prev_cam)
    valid_total = agree_total = occluded_total = moved_total = 0
    wrong = []
    for p in range(passes):
        got = motion_of(ctx, st, [(p, 1)], prev_cam, None, prev_vertices)          # one pass: the sums are the sample
        still = M.motion_of(ctx, st, [(p, 1)], prev_cam, None)                     # the old call: vertices taken to stand still
        rows, xy = ctx.camera_rays(p)
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
        mv = got[y, x]
        valid = mv[:, 3] == 1
        assert (valid <= (hits.view(np.uint32)[:, 0] != abi.MISS)).all()
        moved_total += int((np.abs(mv[valid, :2] - still[y, x][valid, :2]).max(axis=1) > 0.05).sum())
        d = rows[:, 4:7].astype(np.float64) @ w2l_n[:3, :3].T
        px = (0.5 - (d[:, 0] / d[:, 2]) * obj_n / opw_n) * w
        py = (0.5 - (d[:, 1] / d[:, 2]) * obj_n / oph_n) * h
        assert (np.abs(px - (x + 0.5)) <= 0.5 + 1e-3).all() and (np.abs(py - (y + 0.5)) <= 0.5 + 1e-3).all()
        tx, ty = px + mv[:, 0], py + mv[:, 1]
        local = np.stack([opw_p * (0.5 - tx / w), oph_p * (0.5 - ty / h), np.full(len(tx), obj_p)], axis=1)
        local /= np.linalg.norm(local, axis=1, keepdims=True)
        ray = np.zeros((len(tx), 8), F)
        ray[:, 0:3], ray[:, 4:7], ray[:, 7] = l2w_p[:3, 3], local @ l2w_p[:3, :3].T, np.inf
        ray = ray[valid]
        then, then_inst = yard.intersect_rays(ray, want_instances=True)
        same = (then.view(np.uint32)[:, 0] == hits.view(np.uint32)[valid, 0]) & (then_inst == inst[valid])
        z = mv[valid, 2]
        hidden = ~same & (then[:, 1] < z * F(1.0 - 1e-3))
        far = same & (np.abs(then[:, 1].astype(np.float64) - z) > 1e-3 * z)
        valid_total, agree_total, occluded_total = valid_total + int(valid.sum()), agree_total + int(same.sum()), occluded_total + int(hidden.sum())
        for k in np.nonzero((~same & ~hidden) | far)[0]:
            wrong.append((p, int(x[valid][k]), int(y[valid][k]), int(inst[valid][k]), int(hits.view(np.uint32)[valid, 0][k]), int(then_inst[k]),
                          int(then.view(np.uint32)[k, 0]), float(then[k, 1]), float(z[k])))
    print("%s: valid samples %d of %d, the same triangle %d, hidden in the previous frame %d, unexplained %d; moved by the vertices %d"
          % (name, valid_total, passes * w * h, agree_total, occluded_total, len(wrong), moved_total))
    for row in wrong:
        print("  pass %d pixel (%d, %d): now instance %d triangle %d; then instance %d triangle %d at %.6f, z' %.6f" % row)
    assert valid_total >= 0.25 * passes * w * h
    assert moved_total >= 0.25 * valid_total, "the input condition: the vertices' motion is a visible part of the vectors"
    assert occluded_total <= 0.25 * valid_total, "the input condition: few of the points were hidden in the previous frame"
    assert not wrong, wrong[:10]
    assert agree_total >= 0.7 * valid_total


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_previous_positions_make_their_samples_invalid(contexts, moved_buffers, bad):
    name = "lattice"
    now, prev_cam, prev_rec, prev_vertices = moved_case(name, False)
    ctx = moved_context(contexts, name)
    st = settings()
    if (name, False) not in moved_buffers:
        moved_buffers[(name, False)] = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, prev_vertices)
    clean = moved_buffers[(name, False)]
    n = len(prev_vertices)
    band = np.zeros(n, bool)
    band[n // 4:n // 2] = True
    broken = prev_vertices.copy()
    broken["position"][band, 1] = bad
    got = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, broken)
    assert np.isfinite(got).all()
    # per pixel: the samples whose triangle touches the band, from the library's own closest hits
    touched = band[now.triangles["v"]].any(axis=1)
    ctx.render_begin(st)
    on_band, off_band = np.zeros((SIZE, SIZE), np.int64), np.zeros((SIZE, SIZE), np.int64)
    for p in range(SPP):
        rows, xy = ctx.camera_rays(p)
        hits = ctx.intersect_rays(rows)
        t = hits.view(np.uint32)[:, 0]
        hit = t != abi.MISS
        x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
        np.add.at(on_band, (y, x), hit & touched[np.where(hit, t, 0)])
        np.add.at(off_band, (y, x), hit & ~touched[np.where(hit, t, 0)])
    assert (on_band > 0).mean() >= 0.05 and (on_band == 0).mean() >= 0.05, "the input condition: the band is a part of the image, and not all of it"
    assert (got[..., 3] <= off_band).all(), "a sample on a triangle that touches the band is invalid"
    all_on = (on_band > 0) & (off_band == 0)
    assert all_on.any() and (got[all_on] == 0).all()
    untouched = on_band == 0
    assert_bit_equal(got[untouched], clean[untouched], "the other pixels")


@pytest.mark.gpu
def test_refusals_on_a_live_context_change_nothing(contexts):
    st = settings()
    lib = binding.load_library()
    with DeviceBlocks() as dev:
        block = dev.alloc(1 << 20)

        def call(ctx, vertices=block, transforms=None, reserved=0, frame_reserved=(0, 0), desc=True, begin=0, count=1):
            d = abi.MotionVerticesDesc(abi.MotionDesc(None, transforms, (C.c_uint32 * 2)(*frame_reserved)), vertices, reserved)
            rc = lib.slrhip_render_motion_vertices(ctx.handle, C.byref(d) if desc else None, begin, count, None)
            return rc, lib.slrhip_last_error_string().decode()

        for name, flags, cases in (
                ("flat", DYNAMIC, [(dict(desc=False), INVALID, ""), (dict(reserved=1), INVALID, ""), (dict(vertices=block + 2), INVALID, "previous_vertices"),
                                   (dict(frame_reserved=(0, 1)), INVALID, ""), (dict(transforms=block), INVALID, "no instances"),
                                   (dict(begin=0xFFFFFFFF, count=2), INVALID, "2^32")]),
                ("flat", 0, [(dict(), UNSUPPORTED, "SLRHIP_FLAG_DYNAMIC_GEOMETRY")]),
                ("lattice", 0, [(dict(), UNSUPPORTED, "SLRHIP_FLAG_DYNAMIC_GEOMETRY")]),
                ("lattice", DYNAMIC, [(dict(), UNSUPPORTED, "SLRHIP_FLAG_DYNAMIC_INSTANCED"), (dict(transforms=block + 8), INVALID, "previous_transforms")]),
                ("terrain8", DYNAMIC | SPLITS, [(dict(), UNSUPPORTED, "spatial splits")])):
            sc = V.base_scene(name) if name == "terrain8" else base_scene(name)
            ctx = contexts(flags, 2)
            ctx.upload_scene(sc)
            ctx.render_begin(st)
            ctx.render_motion(2, M.moved_camera(sc.camera, (0.05, -0.03, 0.06), 0.03))
            before = ctx.motion()
            assert (before[..., 3] > 0).mean() >= 0.25
            for over, code, text in cases:
                rc, message = call(ctx, **over)
                assert rc == code and message.startswith("slrhip_render_motion_vertices: ") and text in message, (name, flags, over, rc, message)
                assert_bit_equal(ctx.motion(), before, "a refused call changes nothing")
                assert ctx.features_status() == 0
            assert call(ctx, vertices=None, count=0)[0] == 0                    # nothing to do
            assert_bit_equal(ctx.motion(), before, "no pass: nothing changes")
        fresh = contexts(DYNAMIC, 3)
        fresh.upload_scene(base_scene("flat"))
        assert call(fresh)[0] == NO_SCENE                                        # a scene, but no render state since the upload


def in_child(check):
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_motion_vertices as T\nT.%s()\nprint('CHILD_OK')\n"
           % (ROOT, os.path.join(ROOT, "tests"), check))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (check, p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.gpu
def test_graph_captured_call_replays_the_eager_result():
    """A later call and its resolve captured in a graph (a single branch), with the previous vertices and transforms in device tensors."""
    in_child("_graph_check")


def _graph_check():
    import torch
    name = "lattice"
    _, prev_cam, prev_rec, prev_vertices = moved_case(name, True)
    st = settings()
    ctx = Context(flags=flags_of(name))
    try:
        ctx.upload_scene(base_scene(name))
        ctx.set_vertices(perturbed(name))
        want = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, prev_vertices)
        ctx.render_begin(st)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            rec = torch.from_numpy(prev_rec).cuda()
            verts = torch.from_numpy(np.ascontiguousarray(prev_vertices).view(F).reshape(-1, 11).copy()).cuda()
            out = torch.zeros((SIZE, SIZE, 4), dtype=torch.float32, device="cuda")
            ctx.render_motion(3, prev_cam, rec, stream=side, previous_vertices=verts)      # the first call allocates and clears: passes [0, 3)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                s = torch.cuda.current_stream()
                ctx.render_motion(5, prev_cam, rec, spp_begin=3, stream=s, previous_vertices=verts)
                ctx.motion_into(out.data_ptr(), out.numel(), stream=s)
            g.replay()
            torch.cuda.synchronize()
        assert ctx.features_status(side) == 0
        assert (out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    finally:
        ctx.close()
