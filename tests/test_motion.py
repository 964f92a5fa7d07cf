"""Motion vectors (slrhip_render_motion / slrhip_resolve_motion / slrhip_read_motion, slrhip_motion_camera, slrhip_motion_sample).

CPU: the exports, the header's definitions and the descriptor's layout; every refusal through the context-free check; and
slrhip_motion_sample — the function the fold kernel calls — bit for bit against a numpy float32 restatement of include/slrhip.h's
definition, on 4 096 random points and three camera pairs, with and without instance records.

GPU: a scene in which nothing moved has motion exactly zero; a moved scene's buffer equals, bit for bit, the restatement summed in pass
order over the library's own camera rays and closest hits; the buffer is independent of shards, of how the passes are cut, of the
colour mode and of interleaved renders, and an updated context equals a fresh one; and — independent of the restatement — a ray of the
PREVIOUS camera through now_pixel + m hits, in a fresh context that holds the previous scene, the same triangle of the same instance.
No tolerance is involved except where test 4 says so."""
import ctypes as C
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, DeviceBlocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, NO_SCENE = 1, 4
SIZE, SPP = 32, 8
FLT_MAX = F(3.402823466e+38)


# ---- the restatement of include/slrhip.h's definition, float32, every intermediate checked ---------------------------------------------
def f32(*arrays):
    for a in arrays:
        assert np.asarray(a).dtype == F, "promoted silently"
    return arrays[0] if len(arrays) == 1 else arrays


def np_mul_point(m, p):
    """mulPoint: m [16] or [n, 16] column-major, p [n, 3] -> [n, 3]; per row ((m[r] x + m[4 + r] y) + m[8 + r] z) + m[12 + r] * 1, and
    x, y, z times (1 / w) where w != 1."""
    m = np.asarray(m)
    f32(m, p)
    if m.ndim == 1:
        m = np.broadcast_to(m, (len(p), 16))
    one = F(1.0)
    with np.errstate(all="ignore"):
        q = [f32(((m[:, r] * p[:, 0] + m[:, 4 + r] * p[:, 1]) + m[:, 8 + r] * p[:, 2]) + m[:, 12 + r] * one) for r in range(4)]
        inv = f32(one / q[3])
        out = np.stack([np.where(q[3] != one, f32(q[a] * inv), q[a]) for a in range(3)], axis=1)
    return f32(out)


def np_project(mc, q3, width, height):
    """proj(cam, Q) with the 24 constants of slrhip_motion_camera: (valid [n], X [n], Y [n])."""
    f32(mc)
    q = np_mul_point(mc[:16], q3)
    with np.errstate(all="ignore"):
        valid = (q[:, 2] > 0) & (np.abs(q) <= FLT_MAX).all(axis=1)
        x = f32((F(0.5) - f32(f32(f32(q[:, 0] / q[:, 2]) * mc[21]) / mc[19])) * F(width))
        y = f32((F(0.5) - f32(f32(f32(q[:, 1] / q[:, 2]) * mc[21]) / mc[20])) * F(height))
    return valid, x, y


def np_motion(mc_now, mc_prev, rec_now, rec_prev, inst, width, height, p):
    """Per sample {m.x, m.y, z', valid} [n, 4]: p [n, 3] the hit points now, inst [n] the instance hit (-1: a loose triangle),
    rec_now / rec_prev [instances, 32] the placements now and in the previous frame (None: the scene has none)."""
    f32(p)
    loose = inst < 0 if rec_now is not None else np.ones(len(p), bool)
    p_now, p_prev = p, p
    if rec_now is not None and (~loose).any():
        k = np.maximum(inst, 0)
        local = np_mul_point(rec_now[k, 16:], p)
        p_now = np.where(loose[:, None], p, np_mul_point(rec_now[k, :16], local))
        p_prev = np.where(loose[:, None], p, np_mul_point(rec_prev[k, :16], local))
    ok_now, x_now, y_now = np_project(mc_now, f32(p_now), width, height)
    ok_prev, x_prev, y_prev = np_project(mc_prev, f32(p_prev), width, height)
    valid = ok_now & ok_prev
    with np.errstate(all="ignore"):
        d = f32(p_prev - mc_prev[16:19])
        z = f32(np.sqrt(f32(f32(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])))
        out = np.stack([f32(x_prev - x_now), f32(y_prev - y_now), z, np.ones(len(p), F)], axis=1)
    return f32(np.where(valid[:, None], out, F(0.0)))


# ---- cameras and placements ------------------------------------------------------------------------------------------------------------
def camera_matrix(cam):
    return np.array(cam.local_to_world[:], np.float64).reshape(4, 4).T


def moved_camera(cam, translation=(0.0, 0.0, 0.0), angle=0.0, axis=(0, 1, 0)):
    """The camera turned about its own position by `angle` and then translated (world space)."""
    m = camera_matrix(cam)
    pos = m[:3, 3].copy()
    turn = scenes._translate(*pos) @ scenes._rotate(angle, axis) @ scenes._translate(*(-pos))
    return scenes.make_camera(scenes._translate(*translation) @ turn @ m, cam.aspect, cam.fov_y, cam.lens_radius, cam.img_plane_distance,
                              cam.obj_plane_distance, cam.sensitivity)


def records(sc):
    """[n, 32] float32: local_to_world, world_to_local of the scene's instances."""
    return np.concatenate([sc.instances["local_to_world"], sc.instances["world_to_local"]], axis=1).astype(F)


def _mats(rec):
    r = rec.astype(np.float64)
    return r[:, :16].reshape(-1, 4, 4).transpose(0, 2, 1), r[:, 16:].reshape(-1, 4, 4).transpose(0, 2, 1)


def _records(l2w, w2l):
    return np.concatenate([l2w.transpose(0, 2, 1).reshape(-1, 16), w2l.transpose(0, 2, 1).reshape(-1, 16)], axis=1).astype(F)


def placed(rec, d, s=1.0, angle=0.0):
    """Each placement after a local scale s (a power of two), then a rotation about the world's Y axis through the placement's own
    origin, then a world translation d [n, 3]: T(d) R L S(s) and its inverse, rounded to float32 once."""
    l2w, w2l = _mats(rec)
    out_l, out_w = [], []
    for k in range(len(rec)):
        o = l2w[k][:3, 3]
        turn = scenes._translate(*o) @ scenes._rotate(angle, (0, 1, 0)) @ scenes._translate(*(-o))
        back = scenes._translate(*o) @ scenes._rotate(-angle, (0, 1, 0)) @ scenes._translate(*(-o))
        out_l.append(scenes._translate(*d[k]) @ turn @ l2w[k] @ np.diag([s, s, s, 1.0]))
        out_w.append(np.diag([1 / s, 1 / s, 1 / s, 1.0]) @ w2l[k] @ back @ scenes._translate(*(-np.asarray(d[k], np.float64))))
    return _records(np.array(out_l), np.array(out_w))


def with_records(sc, rec=None, camera=None):
    """The scene with the instance matrices of `rec` and / or another camera: what a fresh context uploads."""
    inst = sc.instances.copy()
    if rec is not None:
        inst["local_to_world"], inst["world_to_local"] = rec[:, :16], rec[:, 16:]
    assert sc.env is None and len(sc.textures) == 0
    return abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, camera if camera is not None else sc.camera, None,
                     sc.name + "_moved", instances=inst if len(inst) else None)


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name == "lattice":
        return scenes.lattice_instanced()
    if name == "cornell":
        return scenes.cornell_instanced(1.0, 10, 5, copies=24)
    assert name == "flat"
    return scenes.cornell_box_spheres(1.0, 8, 4, "glass")


def previous_frame(name, which="moved"):
    """(previous records, previous camera) of a scene: translated / scaled placements with a small turn about Y, a camera translated and
    turned; which = "behind": the previous camera looks so far aside that many of the points now in view were not in front of it."""
    sc = base_scene(name)
    rec, n = records(sc), len(sc.instances)
    rng = np.random.default_rng(17)
    span = 0.25 if name == "lattice" else 0.03
    d = rng.uniform(-span, span, (n, 3))
    if name == "lattice":
        d[1] = d[0]                                        # the two coincident terrains stay coincident
        if which == "lifted":
            # The 2-box (instance 4) stands IN the first terrain: its top lies in the plane of the terrain's quads at y = 4, which
            # reach a unit in front of its front face.  Where it moves against the terrain, a quad hides points of that face from
            # a hair in front of them — hidden, but by less than any relative margin.  So it moves with the terrain, lifted by 0.1:
            # the camera looks down by more than 0.1 per unit, so what a quad hid then, a quad hides now.
            d[4] = d[0] + (0.0, 0.1, 0.0)
    prev = placed(rec, d, 1.0, 0.02)
    if which == "scaled":                                  # the second half of the instances had half their size
        prev[n // 2:] = placed(rec, d, 0.5, 0.02)[n // 2:]
    if which == "behind":
        return prev, moved_camera(sc.camera, (0.2, 0.1, -0.3), 1.5)
    return prev, moved_camera(sc.camera, (0.3, -0.2, 0.4) if name == "lattice" else (0.05, -0.03, 0.06), 0.03)


def settings(seed=9, size=SIZE):
    return ob.settings(size, size, seed=seed)


# ---------------------------------------------------------------- CPU --------------------------------------------------------------------
def test_exports_header_version_and_layout():
    lib = binding.load_library()
    for name in ("slrhip_render_motion", "slrhip_resolve_motion", "slrhip_read_motion", "slrhip_motion_camera", "slrhip_motion_sample",
                 "slrhip_debug_motion_check"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert "#define SLRHIP_VERSION 7 " in header and re.search(r"#define SLRHIP_FEATURE_ALL\s+63u", header)
    assert lib.slrhip_version() == 7 and abi.FEATURE_ALL == 63
    for text in ("typedef struct slrhip_motion_desc {", "P = org + dist * dir", "l = mulPoint(world_to_local_now, P)",
                 "X = (0.5f - ((q.x / q.z) * objPlaneDistance) / opWidth) * (float)width", "m = proj(cam_prev, P_prev) - proj(cam_now, P_now)",
                 "z' = length(P_prev - C_prev)", "must name the SAME previous frame", "motion of loose triangles"):
        assert text in header, text
    # struct slrhip_motion_desc { const slrhip_camera*; const slrhip_instance_transform*; uint32_t reserved[2]; }
    d = abi.MotionDesc
    assert C.sizeof(d) == 24 and d.previous_camera.offset == 0 and d.previous_transforms.offset == 8 and d.reserved.offset == 16
    source = open(os.path.join(ROOT, "slr_amd", "csrc", "slrhip_buffers.hip")).read() + open(os.path.join(ROOT, "slr_amd", "csrc", "pt_motion.hip")).read()
    assert "motionSample(" in source and '#include "pt_motion.h"' in open(os.path.join(ROOT, "slr_amd", "csrc", "host_util.cpp")).read()


MOTION_REFUSALS = [("null descriptor", dict(desc=None), INVALID, "null descriptor"),
                   ("reserved[0]", dict(reserved=(1, 0)), INVALID, "reserved must be 0"),
                   ("reserved[1]", dict(reserved=(0, 7)), INVALID, "reserved must be 0"),
                   ("misaligned transforms", dict(transforms=4096 + 8), INVALID, "misaligned previous_transforms (16 bytes)"),
                   ("transforms without instances", dict(num_instances=0), INVALID, "previous_transforms given, but the scene has no instances"),
                   ("pass range", dict(begin=0xFFFFFFF0, count=0x10), INVALID, "pass range beyond 2^32"),
                   ("no render state", dict(have_render=0), NO_SCENE, "call slrhip_render_begin first")]


@pytest.mark.parametrize("what, over, code, text", MOTION_REFUSALS, ids=[r[0] for r in MOTION_REFUSALS])
def test_motion_refusals_through_the_check(what, over, code, text):
    lib = binding.load_library()
    cam = scenes.cornell_camera(1.0)
    a = dict(have_render=1, num_instances=6, transforms=4096, reserved=(0, 0), begin=3, count=5, desc=True)
    ok = abi.MotionDesc(C.pointer(cam), a["transforms"], (C.c_uint32 * 2)(0, 0))
    assert lib.slrhip_debug_motion_check(1, 6, C.byref(ok), 3, 5) == 0
    assert lib.slrhip_debug_motion_check(1, 0, C.byref(abi.MotionDesc(None, None, (C.c_uint32 * 2)(0, 0))), 0, 0xFFFFFFFF) == 0
    a.update(over)
    d = abi.MotionDesc(C.pointer(cam), a["transforms"], (C.c_uint32 * 2)(*a["reserved"]))
    rc = lib.slrhip_debug_motion_check(a["have_render"], a["num_instances"], C.byref(d) if a["desc"] else None, a["begin"], a["count"])
    assert rc == code and lib.slrhip_last_error_string().decode() == "slrhip_render_motion: " + text, (what, rc)


def test_motion_null_arguments():
    lib = binding.load_library()
    d = abi.MotionDesc(None, None, (C.c_uint32 * 2)(0, 0))
    assert lib.slrhip_render_motion(None, C.byref(d), 0, 1, None) == INVALID
    assert lib.slrhip_resolve_motion(None, 4096, 1 << 20, None) == INVALID and lib.slrhip_read_motion(None, 4096, 1 << 20) == INVALID
    out = np.zeros(24, F)
    assert lib.slrhip_motion_camera(None, out.ctypes.data) == INVALID and lib.slrhip_motion_camera(C.byref(scenes.cornell_camera(1.0)), None) == INVALID
    assert lib.slrhip_motion_sample(None, None, None, None, 4, 4, None, None) == INVALID


def test_motion_camera_constants():
    cam = scenes.cornell_camera(1.25)
    mc = binding.motion_camera(cam)
    assert mc.dtype == F and (mc[:16].view(np.uint32) == np.array(cam.world_to_local[:], F).view(np.uint32)).all()
    centre = np_mul_point(np.array(cam.local_to_world[:], F), np.zeros((1, 3), F))[0]
    assert (mc[16:19].view(np.uint32) == centre.view(np.uint32)).all()
    assert mc[21] == F(cam.obj_plane_distance) and mc[19] == F(mc[20] * F(cam.aspect)) and mc[22] == 0 and mc[23] == 0
    assert abs(float(mc[20]) - 2.0 * cam.obj_plane_distance * math.tan(0.5 * cam.fov_y)) <= 1e-6 * float(mc[20])


CAMERA_PAIRS = ["identical", "moved", "behind"]


def camera_pair(which):
    now = scenes._lattice_camera(8)
    if which == "identical":
        return now, now
    if which == "moved":
        return now, moved_camera(now, (0.3, -0.2, 0.4), 0.03)
    return now, moved_camera(now, (0.2, 0.1, -0.3), 1.3)


@pytest.mark.parametrize("pair", CAMERA_PAIRS)
def test_motion_sample_equals_the_restatement(pair):
    """slrhip_motion_sample on 4 096 random points in and around the view: without records (a loose triangle), with a pair of records
    that differ, with a pair that is bit-equal, and with the previous record left out (the instance did not move)."""
    lib = binding.load_library()
    now, prev = camera_pair(pair)
    mc_now, mc_prev = binding.motion_camera(now), binding.motion_camera(prev)
    rng = np.random.default_rng(31)
    n, w, h = 4096, 37, 21
    # points in front of the current camera, spread over and beyond its view; a few degenerate ones
    m = camera_matrix(now)
    local = np.stack([rng.uniform(-12, 12, n), rng.uniform(-9, 9, n), rng.uniform(0.5, 30, n)], axis=1)
    points = (local @ m[:3, :3].T + m[:3, 3]).astype(F)
    points[:4] = [m[:3, 3], m[:3, 3] - m[:3, 2], (np.inf, 0, 0), (np.nan, 1, 2)]       # the lens centre, behind it, not finite
    base = records(scenes.lattice_instanced())
    rec_now = base[rng.integers(0, len(base), n)]
    rec_prev = placed(rec_now, rng.uniform(-0.5, 0.5, (n, 3)), 0.5, 0.05)
    inst = np.arange(n)

    def library(rn, rp):
        out = np.zeros((n, 4), F)
        for k in range(n):
            a = None if rn is None else rn[k].ctypes.data
            b = None if rp is None else rp[k].ctypes.data
            assert lib.slrhip_motion_sample(C.byref(now), C.byref(prev), a, b, w, h, points[k].ctypes.data, out[k].ctypes.data) == 0
        return out
    rec_now, rec_prev = np.ascontiguousarray(rec_now), np.ascontiguousarray(rec_prev)
    loose = np_motion(mc_now, mc_prev, None, None, np.full(n, -1), w, h, points)
    if pair == "behind":
        # the input condition, on the restatement: a share of the points is not valid, a share is
        assert 0.05 <= (loose[:, 3] == 0).mean() <= 0.95, (loose[:, 3] == 0).mean()
    assert_bit_equal(library(None, None), loose, "loose")
    assert_bit_equal(library(None, rec_prev), loose, "a loose triangle does not read the previous record")
    moved = np_motion(mc_now, mc_prev, rec_now, rec_prev, inst, w, h, points)
    assert (moved[:, 3] == 1).mean() >= 0.05 and not (moved[:, :3] == loose[:, :3]).all()
    assert_bit_equal(library(rec_now, rec_prev), moved, "records that differ")
    same = np_motion(mc_now, mc_prev, rec_now, rec_now.copy(), inst, w, h, points)
    assert_bit_equal(library(rec_now, rec_now.copy()), same, "records that are bit-equal")
    assert_bit_equal(library(rec_now, None), same, "no previous record")
    if pair == "identical":
        assert (same[:, 3] == 1).mean() >= 0.05 and (same[:, 0] == 0).all() and (same[:, 1] == 0).all(), "nothing moved: exactly zero"
        assert (loose[:, 0] == 0).all() and (loose[:, 1] == 0).all()


# ---------------------------------------------------------------- GPU --------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(mode=abi.MODE_RGB, which=0):
        key = (mode, which)
        if key not in made:
            made[key] = Context(device=0, mode=mode)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def motion_of(ctx, st, calls, prev_cam=None, prev_rec=None, shard=(0, 1)):
    ctx.render_begin(st, shard)
    for begin, count in calls:
        ctx.render_motion(count, prev_cam, prev_rec, spp_begin=begin)
    out = ctx.motion()
    assert ctx.features_status() == 0
    return out


def restated_motion(ctx, sc, st, passes, prev_cam, prev_rec, want_samples=False):
    """The buffer from the library's own camera rays and closest hits (existing calls), pass by pass, summed in pass order.  The
    context holds `sc` and has begun a render with `st`.  want_samples: also (per-sample vectors [passes, H, W, 4], hit records)."""
    w, h = st.image_width, st.image_height
    mc_now = binding.motion_camera(sc.camera)
    mc_prev = binding.motion_camera(prev_cam) if prev_cam is not None else mc_now
    rec_now = records(sc) if len(sc.instances) else None
    rec_prev = rec_now if prev_rec is None else prev_rec
    acc = np.zeros((h, w, 4), F)
    samples, hit_ids = np.zeros((passes, h, w, 4), F), np.full((passes, h, w, 2), -1, np.int64)
    for p in range(passes):
        rows, xy = ctx.camera_rays(p)
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        hit = hits.view(np.uint32)[:, 0] != abi.MISS
        with np.errstate(all="ignore"):
            point = f32(rows[:, 0:3] + f32(hits[:, 1:2] * rows[:, 4:7]))
        point = np.where(hit[:, None], point, F(0.0))
        out = np_motion(mc_now, mc_prev, rec_now, rec_prev, inst.astype(np.int64), w, h, f32(point))
        out = np.where(hit[:, None], out, F(0.0))
        x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
        acc[y, x] = f32(acc[y, x] + out)
        samples[p, y, x] = out
        hit_ids[p, y, x, 0], hit_ids[p, y, x, 1] = np.where(hit, inst, -2), np.where(hit, hits.view(np.uint32)[:, 0].astype(np.int64), -1)
    return (acc, samples, hit_ids) if want_samples else acc


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lattice", "cornell", "flat"])
def test_nothing_moved_is_exactly_zero(contexts, name):
    sc = base_scene(name)
    ctx = contexts()
    ctx.upload_scene(sc)
    st = settings()
    ctx.render_begin(st)
    ctx.render_features(abi.FEATURE_COVERAGE, SPP)
    coverage = ctx.features(abi.FEATURE_COVERAGE)
    assert (coverage > 0).mean() >= 0.25
    implicit = motion_of(ctx, st, [(0, SPP)])
    explicit = motion_of(ctx, st, [(0, SPP)], sc.camera, records(sc) if len(sc.instances) else None)
    for what, got in (("previous_* NULL", implicit), ("the current frame passed as the previous one", explicit)):
        assert (got[..., 0] == 0).all() and (got[..., 1] == 0).all(), what
        assert (got[..., 3].view(np.uint32) == coverage.view(np.uint32)).all(), what
        assert np.isfinite(got[..., 2]).all() and (got[..., 2][coverage > 0] > 0).all(), what
    assert_bit_equal(implicit, explicit, "both ways of saying that nothing moved")


@pytest.mark.gpu
@pytest.mark.parametrize("name, which", [("lattice", "moved"), ("lattice", "scaled"), ("cornell", "moved"), ("lattice", "behind")])
def test_moved_scene_equals_the_restatement(contexts, name, which):
    sc = base_scene(name)
    prev_rec, prev_cam = previous_frame(name, which)
    ctx = contexts()
    ctx.upload_scene(sc)
    st = settings()
    ctx.render_begin(st)
    want, samples, ids = restated_motion(ctx, sc, st, SPP, prev_cam, prev_rec, want_samples=True)
    hit = ids[..., 1] >= 0
    valid = samples[..., 3] == 1
    print("%s/%s: hit samples %.3f, of them valid %.3f, mean |m| %.2f px" % (name, which, hit.mean(), valid[hit].mean(),
                                                                               np.abs(samples[..., :2][valid]).mean() if valid.any() else 0.0))
    assert hit.mean() >= 0.25
    if which == "behind":
        assert (~valid[hit]).mean() >= 0.05 and valid[hit].mean() >= 0.05, "the input condition: a share of the hit samples is not valid"
    else:
        assert valid[hit].mean() >= 0.9 and (np.abs(samples[..., :2][valid]) > 0.05).mean() >= 0.5, "the vectors are not trivial"
    got = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec)
    assert_bit_equal(got, want, "%s/%s" % (name, which))
    # a device pointer for the previous transforms gives the same buffer as the staged numpy array
    with DeviceBlocks() as dev:
        ctx.render_begin(st)
        ctx.render_motion(SPP, prev_cam, dev.put(prev_rec))
        assert_bit_equal(ctx.motion(), want, "previous_transforms as a device address")


@pytest.mark.gpu
def test_independence_of_shards_cuts_mode_and_interleaving(contexts):
    sc = base_scene("cornell")
    prev_rec, prev_cam = previous_frame("cornell")
    st = settings()
    ctx = contexts()
    ctx.upload_scene(sc)
    whole = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec)
    assert (whole[..., 3] > 0).mean() >= 0.25
    halves = [motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec, shard=(k, 2)) for k in range(2)]
    assert ((halves[0][..., 3] > 0) & (halves[1][..., 3] > 0)).sum() == 0 and (halves[0][..., 3] > 0).any() and (halves[1][..., 3] > 0).any()
    assert_bit_equal(halves[0] + halves[1], whole, "two shards add up to the whole image")
    assert_bit_equal(motion_of(ctx, st, [(0, 3), (3, 5)], prev_cam, prev_rec), whole, "8 passes = 3 + 5")
    spectral = contexts(abi.MODE_SPECTRAL)
    spectral.upload_scene(sc)
    assert_bit_equal(motion_of(spectral, st, [(0, SPP)], prev_cam, prev_rec), whole, "a spectral context")

    # a render interleaved with motion (and feature) calls: the frame and the counters of a render without them
    def frame(interleave):
        ctx.render_begin(st)
        if interleave:
            ctx.render_motion(3, prev_cam, prev_rec)
        ctx.render(0, 4)
        if interleave:
            ctx.render_features(abi.FEATURE_COVERAGE, 2)
            ctx.render_motion(5, prev_cam, prev_rec, spp_begin=3)
        ctx.render(4, 4)
        k = ctx.counters()
        got = (ctx.read_framebuffer(), (k.samples, k.extension_rays, k.shadow_rays))
        if interleave:
            assert_bit_equal(ctx.motion(), whole, "motion calls between renders")
        return got
    alone, mixed = frame(False), frame(True)
    assert (alone[0].view(np.uint32) == mixed[0].view(np.uint32)).all() and alone[1] == mixed[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lattice", "cornell"])
def test_updated_context_equals_a_fresh_one(contexts, name):
    """Frame 1 is the base scene; the instances and the camera then move (set_instance_transforms, set_camera) and frame 2's motion pass
    names frame 1 as its previous frame.  A fresh context uploaded with the moved scene gives the same buffer."""
    sc = base_scene(name)
    now_rec, now_cam = previous_frame(name)               # (any moved placement serves as the new frame here)
    st = settings()
    ctx = contexts()
    ctx.upload_scene(sc)
    ctx.set_instance_transforms(now_rec)
    ctx.set_camera(now_cam)
    assert ctx.instances_status() == 0
    got = motion_of(ctx, st, [(0, SPP)], sc.camera, records(sc))
    fresh = contexts(which=1)
    fresh.upload_scene(with_records(sc, now_rec, now_cam))
    want = motion_of(fresh, st, [(0, SPP)], sc.camera, records(sc))
    assert (want[..., 3] > 0).mean() >= 0.25 and (np.abs(want[..., :2]) > 0).mean() >= 0.25
    assert_bit_equal(got, want, name)


@pytest.mark.gpu
def test_vectors_point_at_the_same_triangle_of_the_previous_frame(contexts):
    """Independent of the restatement: for every valid sample the previous camera's pinhole ray through now_pixel + m, built in float64,
    is traced in a fresh context that holds the PREVIOUS scene.  It must hit the same triangle of the same instance, unless the previous
    scene's hit is nearer than z' (1 - 1e-3): the point was hidden then."""
    name, passes = "lattice", 4
    sc = base_scene(name)
    assert sc.camera.lens_radius == 0.0                    # a pinhole: the projection through the lens centre inverts the camera sample
    prev_rec, prev_cam = previous_frame(name, "lifted")
    st = settings(seed=3)
    w, h = st.image_width, st.image_height
    ctx = contexts()
    ctx.upload_scene(sc)
    yard = contexts(which=1)
    yard.upload_scene(with_records(sc, prev_rec, prev_cam))
    yard.render_begin(st)

    def f64(cam):
        l2w = camera_matrix(cam)
        w2l = np.array(cam.world_to_local[:], np.float64).reshape(4, 4).T
        op_h = 2.0 * cam.obj_plane_distance * math.tan(0.5 * cam.fov_y)
        return l2w, w2l, op_h * cam.aspect, op_h, float(cam.obj_plane_distance)
    l2w_n, w2l_n, opw_n, oph_n, obj_n = f64(sc.camera)
    l2w_p, w2l_p, opw_p, oph_p, obj_p = f64(prev_cam)
    valid_total = agree_total = occluded_total = 0
    wrong = []
    for p in range(passes):
        got = motion_of(ctx, st, [(p, 1)], prev_cam, prev_rec)          # one pass: the sums are the sample
        rows, xy = ctx.camera_rays(p)
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        x, y = (xy & 0xFFFF).astype(np.int64), (xy >> 16).astype(np.int64)
        mv = got[y, x]
        valid = mv[:, 3] == 1
        assert (valid <= (hits.view(np.uint32)[:, 0] != abi.MISS)).all()
        # where on the image the sample is: its ray's direction through the current camera, in float64
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
        hidden = ~same & (then[:, 1] < mv[valid, 2] * F(1.0 - 1e-3))
        valid_total, agree_total, occluded_total = valid_total + int(valid.sum()), agree_total + int(same.sum()), occluded_total + int(hidden.sum())
        for k in np.nonzero(~same & ~hidden)[0]:
            wrong.append((p, int(x[valid][k]), int(y[valid][k]), int(inst[valid][k]), int(hits.view(np.uint32)[valid, 0][k]), int(then_inst[k]),
                          int(then.view(np.uint32)[k, 0]), float(then[k, 1]), float(mv[valid, 2][k])))
    print("valid samples %d, the same triangle %d, hidden in the previous frame %d, unexplained %d" % (valid_total, agree_total, occluded_total, len(wrong)))
    for row in wrong:
        print("  pass %d pixel (%d, %d): now instance %d triangle %d; then instance %d triangle %d at %.6f, z' %.6f" % row)
    assert valid_total >= 0.25 * passes * w * h
    assert occluded_total <= 0.25 * valid_total, "the input condition: few of the points were hidden in the previous frame"
    assert not wrong, wrong[:10]
    assert agree_total >= 0.7 * valid_total


def in_child(check):
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_motion as T\nT.%s()\nprint('CHILD_OK')\n"
           % (ROOT, os.path.join(ROOT, "tests"), check))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (check, p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.gpu
def test_graph_captured_motion_call_replays_the_eager_result():
    """A later motion call and its resolve captured in a graph (a single branch), with the previous transforms in a device tensor."""
    in_child("_graph_check")


def _graph_check():
    import torch
    sc = base_scene("cornell")
    prev_rec, prev_cam = previous_frame("cornell")
    st = settings()
    ctx = Context()
    try:
        ctx.upload_scene(sc)
        want = motion_of(ctx, st, [(0, SPP)], prev_cam, prev_rec)
        ctx.render_begin(st)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            rec = torch.from_numpy(prev_rec).cuda()
            out = torch.zeros((SIZE, SIZE, 4), dtype=torch.float32, device="cuda")
            ctx.render_motion(3, prev_cam, rec, stream=side)             # the first call allocates and clears: passes [0, 3)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                s = torch.cuda.current_stream()
                ctx.render_motion(5, prev_cam, rec, spp_begin=3, stream=s)
                ctx.motion_into(out.data_ptr(), out.numel(), stream=s)
            g.replay()
            torch.cuda.synchronize()
        assert ctx.features_status(side) == 0
        assert (out.cpu().numpy().view(np.uint32) == want.view(np.uint32)).all()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_calls_that_are_refused_on_a_context(contexts):
    ctx = contexts(which=2)
    lib = ctx.lib
    d = abi.MotionDesc(None, None, (C.c_uint32 * 2)(0, 0))
    ctx.upload_scene(base_scene("flat"))
    st = settings()
    ctx.render_begin(st)
    with DeviceBlocks() as dev:
        block = dev.alloc(128 * 4)
        bad = abi.MotionDesc(None, block, (C.c_uint32 * 2)(0, 0))
        assert lib.slrhip_render_motion(ctx.handle, C.byref(bad), 0, 1, None) == INVALID          # the flat scene has no instances
        assert lib.slrhip_render_motion(ctx.handle, None, 0, 1, None) == INVALID
        assert lib.slrhip_render_motion(ctx.handle, C.byref(d), 0, 0, None) == 0                  # nothing to do
        assert lib.slrhip_resolve_motion(ctx.handle, block + 2, 1 << 20, None) == INVALID and lib.slrhip_resolve_motion(ctx.handle, block, 8, None) == INVALID
    got = ctx.motion()
    assert (got == 0).all(), "before the first motion call the sums are zeros"
