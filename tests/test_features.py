"""First-hit feature buffers and camera rays (slrhip_render_features / slrhip_resolve_features / slrhip_camera_rays).
CPU: argument checks without a device, the BMP encoding of a normal buffer.  GPU (MI355X): the camera rays against the compiled
reference's jittered pixel positions, the feature pass against slrhip_intersect_rays on the same rays on every tree kind, the
hits against the compiled reference, the surface points against a float32 numpy restatement of the reference's arithmetic, and
the accumulation / independence identities, bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from slr_amd import abi, binding, scenes
from test_ray_queries import assert_same_hits, triangles_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS = abi.MISS
F32 = np.float32
NORMALS = abi.FEATURE_GEOMETRIC_NORMAL | abi.FEATURE_SHADING_NORMAL | abi.FEATURE_SHADING_TANGENT
EPS = 2.0 ** -23


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_feature_entry_points_reject_null_arguments_without_a_gpu():
    lib = binding.load_library()
    bits, count = C.c_uint32(7), C.c_uint32(7)
    assert lib.slrhip_render_features(None, abi.FEATURE_ALL, 0, 1, None) == 1
    assert b"null" in lib.slrhip_last_error_string()
    assert lib.slrhip_render_features(None, abi.FEATURE_ALL, 0, 0, None) == 1
    assert lib.slrhip_resolve_features(None, abi.FEATURE_IDS, None, 0, None) == 1
    assert b"null" in lib.slrhip_last_error_string()
    assert lib.slrhip_camera_rays(None, 0, None, None, 0, C.byref(count), None) == 1
    assert lib.slrhip_camera_rays(None, 0, None, None, 0, None, None) == 1
    assert lib.slrhip_features_status(None, C.byref(bits), None) == 1
    assert b"null" in lib.slrhip_last_error_string()


def test_debug_renderer_outputs_are_parsed_from_the_scene_language():
    """setRenderer("debug", (outputs = (...))) (libSLRSceneGraph/API.cpp:1037-1059) -> renderer["outputs"]; other methods as before."""
    from slr_amd import scene_language as SL

    def renderer(config_items, method="debug"):
        holder = type("H", (), {})()
        SL.Interpreter._set_renderer(holder, {"method": method, "config": SL.Tuple(config_items)})
        return holder.renderer
    r = renderer([("samples", 4), ("outputs", SL.Tuple([(None, "geometric normal"), (None, "distance")]))])
    assert r == {"method": "debug", "samples": 4, "outputs": ["geometric normal", "distance"]}
    assert renderer([("outputs", "shading tangent")])["outputs"] == ["shading tangent"]
    assert renderer([])["outputs"] is None and renderer([])["samples"] == 8
    with pytest.raises(SL.SceneLanguageError, match="unknown output"):
        renderer([("outputs", SL.Tuple([(None, "albedo")]))])
    assert renderer([("samples", 2), ("outputs", "whatever")], method="PT") == {"method": "PT", "samples": 2}


def test_normal_bmp_encoding_matches_debug_renderer_formula(tmp_path):
    """(uint8)clamp((0.5 n + 0.5) * 255, 0, 255) of the per-pixel mean (DebugRenderer.cpp:162-185), BGR bottom-up in the file."""
    from slr_amd import host
    rng = np.random.default_rng(5)
    h, w = 7, 9
    n = rng.normal(size=(h, w, 3)).astype(F32)
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    cov = rng.integers(0, 5, (h, w)).astype(F32)
    sums = n * cov[:, :, None]
    bgr = host.encode_normals(sums, cov)
    mean = np.where(cov[:, :, None] > 0, sums / np.maximum(cov, 1)[:, :, None], 0).astype(F32)
    want = np.clip((F32(0.5) * mean + F32(0.5)) * F32(255), 0, 255).astype(np.uint8)
    assert bgr.shape == (h, w, 3) and bgr.dtype == np.uint8
    assert (bgr[::-1, :, ::-1] == want).all()
    assert (bgr[::-1][cov == 0] == 127).all()              # a pixel without a hit: n = 0 -> 127
    path = str(tmp_path / "n.bmp")
    host.save_bmp(path, bgr)
    raw = open(path, "rb").read()
    assert raw[:2] == b"BM" and len(raw) >= 54 + h * ((w * 3 + 3) // 4 * 4)


# ---- GPU helpers -------------------------------------------------------------------------------------------------------------
def settings(w, h, seed=42):
    from oracle import binding as ob
    return ob.settings(w, h, seed=seed)


def one_pass(ctx, st, channels, pass_, shard=(0, 1)):
    ctx.render_begin(st, shard)
    ctx.render_features(channels | abi.FEATURE_COVERAGE, 1, pass_)
    return {c: ctx.features(c) for c in abi.FEATURE_CHANNELS if c & (channels | abi.FEATURE_COVERAGE)}


def per_pixel(rows_or_vals, xy, h, w, fill=0):
    out = np.full((h, w) + rows_or_vals.shape[1:], fill, rows_or_vals.dtype)
    out[xy >> 16, xy & 0xFFFF] = rows_or_vals
    return out


SCENES = {
    "cornell_box_spheres": (lambda: scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "glass"), 0),
    "cornell_instanced": (lambda: scenes.cornell_instanced(1.0, 10, 5, copies=6), 0),
    "cornell_textured": (lambda: scenes.cornell_textured(1.0, 16, 8), 0),
    "displaced_grid_400": (lambda: scenes.displaced_grid(400), 0),
    "cornell_device_build": (lambda: scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "glass"), abi.FLAG_BVH_DEVICE_BUILD),
    "cornell_spatial_splits": (lambda: scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "glass"), abi.FLAG_BVH_SPATIAL_SPLITS),
}


# ---- 1. camera rays are the reference's ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_pinhole", "cornell_box_spheres", "displaced_grid_60"])
def test_camera_rays_meet_the_reference_object_plane_point(ref_rgb, name):
    """The ray of (pixel, pass) in camera space starts on the lens (z = 0, |xy| <= lens_radius) and meets the plane z =
    obj_plane_distance at (opWidth (0.5 - p.x / W), opHeight (0.5 - p.y / H)), p = the REFERENCE's jittered position.
    Bound, derived: the device computes the point pFocus in float32 (one division, one subtraction, one product: 3 roundings ->
    1.5 eps relative to opWidth / 2), normalises pFocus - org (a sum of three squares, a square root, a reciprocal, a product: <= 4
    eps relative per component), and applies a 3 x 3 transform (3 products + 2 sums: <= 3 eps of the vector's length); this test
    undoes it with world_to_local in float64 (exact to 1e-16).  Scaling the direction back to the plane multiplies by
    |pFocus - org| / dir.z <= sqrt(objDist^2 + (opWidth^2 + opHeight^2) / 4) / objDist x objDist, which is < 2 opWidth for every
    camera here; so |error| <= (1.5 + 4 + 3) eps x 2 opWidth = 17 eps opWidth, with eps = 2^-23.  The origin: one 3 x 4 transform of
    a vector of length <= lens_radius plus the translation: 4 eps of the translation's length."""
    sc = scenes.displaced_grid(60) if name == "displaced_grid_60" else SCENES["cornell_box_spheres"][0]()
    cam = sc.camera
    if name == "cornell_pinhole":
        cam.lens_radius = 0.0                   # the same camera without a lens: every ray starts at the translation column
    assert (cam.lens_radius > 0) == (name != "cornell_pinhole")
    w, h = 64, 48
    st = settings(w, h, seed=11)
    ref = ref_rgb.scene(sc)
    passes = [0, 1, 7, 500, 1000]
    w2l = np.asarray(cam.world_to_local, np.float64).reshape(4, 4).T
    op_h = 2.0 * cam.obj_plane_distance * np.tan(cam.fov_y * 0.5)
    op_w = op_h * cam.aspect
    translation = np.asarray(cam.local_to_world, np.float64)[12:15]
    # the premise of the bound: the longest camera-space ray to the object plane, lens included, is shorter than 2 opWidth
    assert np.sqrt(cam.obj_plane_distance ** 2 + (op_w / 2 + cam.lens_radius) ** 2 + (op_h / 2 + cam.lens_radius) ** 2) < 2 * op_w
    ctx = binding.Context()
    checked = 0
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        for p in passes:
            rows, xy = ctx.camera_rays(p)
            assert len(rows) == w * h and (rows[:, 3] == 0).all() and np.isinf(rows[:, 7]).all()
            assert sorted(xy.tolist()) == sorted((np.arange(w)[None, :] | (np.arange(h)[:, None] << 16)).reshape(-1).tolist())
            pick = np.arange(p % 3, len(rows), 3)                # 1 024 of the 3 072 pixels of each pass, spread over the frame
            C_ = ref.components
            pxy = np.array([ref.sample(st, int(xy[i] & 0xFFFF), int(xy[i] >> 16), p)[C_:C_ + 2] for i in pick], np.float64)
            assert (pxy[:, 0].astype(int) == (xy[pick] & 0xFFFF)).all() and (pxy[:, 1].astype(int) == (xy[pick] >> 16)).all()
            org = rows[pick, 0:3].astype(np.float64) @ w2l[:3, :3].T + w2l[:3, 3]
            d = rows[pick, 4:7].astype(np.float64) @ w2l[:3, :3].T
            tol_org = 4 * EPS * max(np.linalg.norm(translation), 1.0)
            assert np.abs(org[:, 2]).max() <= tol_org
            assert (np.linalg.norm(org[:, :2], axis=1) <= cam.lens_radius * (1 + 4 * EPS) + tol_org).all()
            if cam.lens_radius == 0:
                assert (rows[pick, 0:3] == translation.astype(F32)).all()
            t = (cam.obj_plane_distance - org[:, 2]) / d[:, 2]
            at = org + d * t[:, None]
            want = np.stack([op_w * (0.5 - pxy[:, 0] / w), op_h * (0.5 - pxy[:, 1] / h)], 1)
            err = np.abs(at[:, :2] - want).max()
            print("camera rays %s pass %d: max error %.3e, bound %.3e" % (name, p, err, 17 * EPS * op_w))
            assert err <= 17 * EPS * op_w
            checked += len(pick)
    finally:
        ctx.close()
    assert checked >= 4096


# ---- 2. the feature pass traces these rays --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SCENES))
def test_one_pass_ids_and_distance_equal_intersect_rays_on_the_camera_rays(name):
    make, flags = SCENES[name]
    sc = make()
    w, h = 96, 72
    st = settings(w, h, seed=5)
    ctx = binding.Context(flags=flags)
    try:
        ctx.upload_scene(sc)
        for p in (0, 3):
            ctx.render_begin(st)
            rows, xy = ctx.camera_rays(p)
            hits, inst = ctx.intersect_rays(rows, want_instances=True)
            got = one_pass(ctx, st, abi.FEATURE_IDS | abi.FEATURE_DISTANCE, p)
            ids, dist, cov = got[abi.FEATURE_IDS], got[abi.FEATURE_DISTANCE], got[abi.FEATURE_COVERAGE]
            tri = triangles_of(hits)
            hit = tri != MISS
            assert hit.sum() > 1000
            assert (ids[:, :, 0] == per_pixel(tri, xy, h, w)).all()
            assert (ids[:, :, 1] == per_pixel(inst.view(np.uint32), xy, h, w)).all()
            mat = per_pixel(np.where(hit, sc.triangles["material"][np.where(hit, tri, 0)], MISS).astype(np.uint32), xy, h, w)
            assert (ids[:, :, 2] == mat).all()
            want_dist = per_pixel(np.where(hit, hits[:, 1], F32(0)).astype(F32), xy, h, w)
            assert (dist.view(np.uint32) == want_dist.view(np.uint32)).all()
            assert (cov == per_pixel(hit.astype(F32), xy, h, w)).all()
        assert ctx.features_status() == 0
    finally:
        ctx.close()


# ---- 3. hits are the reference's --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [abi.MODE_RGB, abi.MODE_SPECTRAL])
@pytest.mark.parametrize("name", ["cornell_instanced", "cornell_textured"])
def test_camera_ray_hits_equal_the_live_reference(request, name, mode):
    from oracle import binding as ob
    ref = request.getfixturevalue("ref_rgb" if mode == abi.MODE_RGB else "ref_spectral")
    sc = SCENES[name][0]()
    st = settings(128, 128, seed=9)
    ctx = binding.Context(mode=mode)
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        rows = np.concatenate([ctx.camera_rays(p)[0] for p in (0, 1, 2, 3)])
        hits = ctx.intersect_rays(rows)
    finally:
        ctx.close()
    rays = np.zeros(len(rows), ob.ray_dtype)
    rays["org"], rays["dir"], rays["dist_min"], rays["dist_max"] = rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7]
    want = ref.scene(sc).trace(rays)
    w4 = np.zeros((len(rows), 4), F32)
    w4[:, 0], w4[:, 1], w4[:, 2], w4[:, 3] = want["triangle"].view(F32), want["dist"], want["b0"], want["b1"]
    miss = want["triangle"] == MISS
    w4[miss, 1] = hits[miss, 1]                        # the distance of a miss is not part of the comparison (INFINITY here)
    w4[miss, 2:] = 0
    assert (~miss).sum() > 10000
    assert_same_hits(hits, w4, name)


# ---- 4. surface points are the reference's arithmetic -----------------------------------------------------------------------------
def f32_normalize(v):
    l = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    r = F32(1) / l
    return v * r[:, None]


def f32_dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def f32_from_local(fx, fy, fz, v):
    """ReferenceFrame::fromLocal (geometry.h:225-235): component k = dot((x_k, y_k, z_k), v), left to right."""
    return np.stack([fx[:, k] * v[:, 0] + fy[:, k] * v[:, 1] + fz[:, k] * v[:, 2] for k in range(3)], 1)


def f32_cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def checker_normal_components(tex, u, v, guard):
    """CheckerBoardNormal3DTexture::evaluate (checker_board_textures.cpp:16-43) after OffsetAndScale2DMapping::map, float32.  Also
    returns `near`: the texture coordinate lies within `guard` of one of the steps (or of the wrap) of this piecewise-constant
    function, where an ulp of the coordinate decides the value."""
    ox, oy = F32(tex["offset"][0]), F32(tex["offset"][1])
    sx, sy = F32(tex["scale"][0]), F32(tex["scale"][1])
    step, reverse = F32(tex["value"][0]), F32(tex["value"][1]) != 0
    x, y = (u + ox) * sx, (v + oy) * sy
    q = (step * F32(0.5)) * F32(0.5)
    wu, wv = np.fmod(np.abs(x), F32(1)), np.fmod(np.abs(y), F32(1))

    def comp(wr):
        c = np.zeros(len(wr), F32)
        c[(wr > F32(0.5) - q) & (wr < F32(0.5) + q)] = -1
        c[(wr < q) | (wr > F32(1) - q)] = 1
        return c
    uc, vc = comp(wu), comp(wv)
    uc = np.where(wv > F32(0.5), -uc, uc)
    vc = np.where(wu > F32(0.5), -vc, vc)
    if reverse:
        uc, vc = -uc, -vc
    edges = np.array([0.0, float(q), 0.5 - float(q), 0.5, 0.5 + float(q), 1.0 - float(q), 1.0])
    near = (np.abs(wu.astype(np.float64)[:, None] - edges).min(1) < guard) | (np.abs(wv.astype(np.float64)[:, None] - edges).min(1) < guard)
    return uc.astype(F32), vc.astype(F32), near


def restate_surface_points(sc, tri, inst, b0, b1):
    """Triangle::getSurfacePoint (TriangleMesh.cpp:180-215), the bump step (SurfaceObject.cpp:123-134) and the instance step
    (:329-336) in numpy float32, one rounding per operation, left to right as the C++ evaluates.  From the public hit record
    (b0, b1) = (Intersection::u, ::v).  Returns the three vectors and `near`, the bump-mapped hits whose texture coordinate is
    within 1e-4 of a step of the normal map: the reference interpolates the texture coordinate with Moller-Trumbore's own b2
    (TriangleMesh.cpp:160-161), which the hit record does not carry; 1 - u - v differs from it by a few 2^-24, the coordinate
    (|texcoord| <= 1, scale <= 6: see the scenes) by < 1e-5 after the mapping, and the texture is piecewise constant, so the
    restatement is exact except where a step lies inside that interval."""
    v = sc.triangles["v"][tri]
    V = sc.vertices
    p = [V["position"][v[:, k]].astype(F32) for k in range(3)]
    gn = f32_normalize(f32_cross(p[1] - p[0], p[2] - p[0]))
    b2 = F32(1) - b0 - b1
    nrm = [V["normal"][v[:, k]].astype(F32) for k in range(3)]
    tng = [V["tangent"][v[:, k]].astype(F32) for k in range(3)]
    sn = f32_normalize(b0[:, None] * nrm[0] + b1[:, None] * nrm[1] + b2[:, None] * nrm[2])
    tn = f32_normalize(b0[:, None] * tng[0] + b1[:, None] * tng[1] + b2[:, None] * tng[2])
    d = f32_dot(sn, tn)
    fix = np.abs(d) >= F32(0.01)
    tn = np.where(fix[:, None], f32_normalize(tn - d[:, None] * sn), tn)
    near = np.zeros(len(tri), bool)
    nmap = (sc.materials["reserved"][sc.triangles["material"][tri]] & 0xFFFF).astype(np.int64) - 1
    for t in np.unique(nmap[nmap >= 0]):
        m = nmap == t
        uv = [V["texcoord"][v[m, k]].astype(F32) for k in range(3)]
        tu = (b0[m] * uv[0][:, 0] + b1[m] * uv[1][:, 0]) + b2[m] * uv[2][:, 0]
        tv = (b0[m] * uv[0][:, 1] + b1[m] * uv[1][:, 1]) + b2[m] * uv[2][:, 1]
        uc, vc, near[m] = checker_normal_components(sc.textures[t], tu, tv, 1e-4)
        n_l = f32_normalize(np.stack([uc, vc, np.ones_like(uc)], 1))
        zero = np.zeros_like(uc)
        dx = n_l[:, 0] * F32(1) + n_l[:, 1] * F32(0) + n_l[:, 2] * F32(0)
        t_l = np.stack([F32(1) + zero, zero, zero], 1) - dx[:, None] * n_l
        fx, fz = tn[m], sn[m]
        fy = f32_cross(fz, fx)
        tn[m] = f32_normalize(f32_from_local(fx, fy, fz, t_l))
        sn[m] = f32_normalize(f32_from_local(fx, fy, fz, n_l))
    for k in np.unique(inst[inst >= 0]):
        m = inst == k
        l2w = np.asarray(sc.instances[k]["local_to_world"], F32)
        w2l = np.asarray(sc.instances[k]["world_to_local"], F32)

        def vec(x):       # Matrix4x4 x Vector3D, column-major m[c * 4 + r]
            return np.stack([l2w[0 + r] * x[:, 0] + l2w[4 + r] * x[:, 1] + l2w[8 + r] * x[:, 2] for r in range(3)], 1)
        g = gn[m]
        gn[m] = f32_normalize(np.stack([w2l[4 * r] * g[:, 0] + w2l[4 * r + 1] * g[:, 1] + w2l[4 * r + 2] * g[:, 2] for r in range(3)], 1))
        sn[m] = f32_normalize(vec(sn[m]))
        tn[m] = f32_normalize(vec(tn[m]))
    return gn, sn, tn, near


def similarity_instances(sc):
    """Instances whose transform keeps angles (M^T M = s^2 I to 1e-5): only those keep normal and tangent orthogonal when both are
    taken to world space as VECTORS (SurfaceObject.cpp:329-336)."""
    out = []
    for rec in sc.instances:
        m = np.asarray(rec["local_to_world"], np.float64).reshape(4, 4).T[:3, :3]
        g = m.T @ m
        out.append(bool(np.abs(g / g[0, 0] - np.eye(3)).max() < 1e-5))
    return np.array(out, bool)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_box_spheres", "cornell_instanced", "cornell_textured"])
def test_one_pass_normals_equal_the_float32_restatement(ref_rgb, name):
    from oracle import binding as ob
    sc = SCENES[name][0]()
    w, h = 96, 96
    st = settings(w, h, seed=21)
    ctx = binding.Context()
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        rows, xy = ctx.camera_rays(2)
        hits, inst = ctx.intersect_rays(rows, want_instances=True)
        got = one_pass(ctx, st, NORMALS, 2)
    finally:
        ctx.close()
    # the reference's hits on these rays: the records the restatement starts from
    rays = np.zeros(len(rows), ob.ray_dtype)
    rays["org"], rays["dir"], rays["dist_min"], rays["dist_max"] = rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7]
    ref = ref_rgb.scene(sc).trace(rays)
    hit = ref["triangle"] != MISS
    r4 = np.zeros((len(rows), 4), F32)
    r4[:, 0], r4[:, 1], r4[:, 2], r4[:, 3] = ref["triangle"].view(F32), np.where(hit, ref["dist"], hits[:, 1]), np.where(hit, ref["b0"], 0), np.where(hit, ref["b1"], 0)
    assert_same_hits(hits, r4, name)
    hit &= triangles_of(hits) == ref["triangle"]              # (an equal-distance tie, at most one, is left out)
    tri = ref["triangle"]
    y, x = xy[hit] >> 16, xy[hit] & 0xFFFF
    gn, sn, tn = (got[c][y, x] for c in (abi.FEATURE_GEOMETRIC_NORMAL, abi.FEATURE_SHADING_NORMAL, abi.FEATURE_SHADING_TANGENT))
    for vname, vv in (("gn", gn), ("sn", sn), ("tn", tn)):
        l = np.linalg.norm(vv.astype(np.float64), axis=1)
        assert np.abs(l - 1).max() <= 4 * EPS, (vname, float(np.abs(l - 1).max()))
    reserved = sc.materials["reserved"][sc.triangles["material"][tri[hit]]]
    bumped = (reserved & 0xFFFF) != 0
    assert bumped.any() == (name == "cornell_textured")
    # TriangleMesh.cpp re-orthogonalises the mesh-local frame above 0.01; an instance's transform then takes normal and tangent to
    # world space as two VECTORS (SurfaceObject.cpp:329-336), which keeps their angle only if it is a similarity
    keeps_angles = np.ones(hit.sum(), bool)
    if len(sc.instances):
        similar = similarity_instances(sc)
        keeps_angles = (inst[hit] < 0) | similar[np.maximum(inst[hit], 0)]
        if name == "cornell_instanced":
            assert not similar.all(), "every placement is a similarity: no hit needs to be left out"
    ortho = ~bumped & keeps_angles
    assert ortho.any() and (np.abs(f32_dot(sn, tn))[ortho] < 0.01 + 4 * EPS).all()
    # a miss adds nothing
    missed = ~per_pixel(triangles_of(hits) != MISS, xy, h, w)
    assert all((got[c][missed] == 0).all() for c in got)
    want_gn, want_sn, want_tn, near = restate_surface_points(sc, tri[hit], inst[hit], ref["b0"][hit], ref["b1"][hit])
    assert near.sum() <= 0.02 * max(1, bumped.sum()), (int(near.sum()), int(bumped.sum()))
    if name == "cornell_textured":
        assert (bumped & ~near).sum() > 300
    for vname, a, b in (("geometric normal", gn, want_gn), ("shading normal", sn, want_sn), ("shading tangent", tn, want_tn)):
        k = ~near if vname != "geometric normal" else np.ones(len(a), bool)      # the bump step does not touch gNormal
        b = F32(0) + b              # the buffer is a float32 SUM that starts at +0: a component -0 comes out as +0
        equal = (a[k].view(np.uint32) == b[k].view(np.uint32)).all(axis=1)
        print("%s %s: %d of %d bit-equal (%d bump-mapped, %d of them near a step of the map)" % (name, vname, equal.sum(), len(equal), bumped.sum(), near.sum()))
        assert equal.all(), (name, vname, int((~equal).sum()), len(equal))


# ---- 5. accumulation and independence ---------------------------------------------------------------------------------------------
FLOAT_CHANNELS = [c for c in abi.FEATURE_CHANNELS if c != abi.FEATURE_IDS]


def read_all(ctx):
    return {c: ctx.features(c) for c in abi.FEATURE_CHANNELS}


def assert_same_buffers(a, b, what):
    for c in a:
        assert (a[c].view(np.uint32) == b[c].view(np.uint32)).all(), (what, abi.FEATURE_CHANNELS[c][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell_textured", "cornell_instanced"])
def test_sixteen_passes_are_the_pass_ordered_sum_however_they_are_cut(name):
    sc = SCENES[name][0]()
    w, h = 80, 60
    st = settings(w, h, seed=33)
    ctx = binding.Context()
    spectral = binding.Context(mode=abi.MODE_SPECTRAL)
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        ctx.render_features(abi.FEATURE_ALL, 16)
        whole = read_all(ctx)
        sums = {c: np.zeros_like(whole[c]) for c in FLOAT_CHANNELS}
        hits = np.zeros((h, w), F32)
        for p in range(16):
            one = one_pass(ctx, st, abi.FEATURE_ALL, p)
            for c in FLOAT_CHANNELS:
                sums[c] = sums[c] + one[c]
            hits += (one[abi.FEATURE_IDS][:, :, 0] != MISS)
        for c in FLOAT_CHANNELS:
            assert (sums[c].view(np.uint32) == whole[c].view(np.uint32)).all(), abi.FEATURE_CHANNELS[c][0]
        assert (one[abi.FEATURE_IDS] == whole[abi.FEATURE_IDS]).all()           # the ids of the highest pass
        assert (whole[abi.FEATURE_COVERAGE] == hits).all() and hits.sum() > 0        # (the box is closed: every ray may hit)
        ctx.render_begin(st)
        ctx.render_features(abi.FEATURE_ALL, 5, 0)
        ctx.render_features(abi.FEATURE_ALL, 11, 5)
        assert_same_buffers(read_all(ctx), whole, "[0, 5) + [5, 16)")
        shards = []
        for k in range(2):
            ctx.render_begin(st, (k, 2))
            ctx.render_features(abi.FEATURE_ALL, 16)
            shards.append(read_all(ctx))
        merged = {c: shards[0][c] + shards[1][c] for c in FLOAT_CHANNELS}
        merged[abi.FEATURE_IDS] = shards[0][abi.FEATURE_IDS] & shards[1][abi.FEATURE_IDS]      # 0xFFFFFFFF outside a shard
        assert_same_buffers(merged, whole, "two shards")
        spectral.upload_scene(sc)
        spectral.render_begin(st)
        spectral.render_features(abi.FEATURE_ALL, 16)
        assert_same_buffers(read_all(spectral), whole, "spectral context")
        assert ctx.features_status() == 0 and spectral.features_status() == 0
    finally:
        ctx.close()
        spectral.close()


@pytest.mark.gpu
def test_a_call_longer_than_the_record_window_is_the_pass_ordered_sum():
    """The record window holds at most 64 passes: 150 passes in one call run in three windows over the same record buffer."""
    sc = SCENES["cornell_textured"][0]()
    w, h = 24, 18
    st = settings(w, h, seed=4)
    ctx = binding.Context()
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        ctx.render_features(abi.FEATURE_ALL, 150)
        whole = read_all(ctx)
        ctx.render_begin(st)
        ctx.render_features(abi.FEATURE_ALL, 70, 0)
        ctx.render_features(abi.FEATURE_ALL, 80, 70)
        assert_same_buffers(read_all(ctx), whole, "[0, 70) + [70, 150)")
        sums = {c: np.zeros_like(whole[c]) for c in FLOAT_CHANNELS}
        for p in range(150):
            one = one_pass(ctx, st, abi.FEATURE_ALL, p)
            for c in FLOAT_CHANNELS:
                sums[c] = sums[c] + one[c]
        for c in FLOAT_CHANNELS:
            assert (sums[c].view(np.uint32) == whole[c].view(np.uint32)).all(), abi.FEATURE_CHANNELS[c][0]
        assert (one[abi.FEATURE_IDS] == whole[abi.FEATURE_IDS]).all()           # the ids of pass 149
        assert ctx.features_status() == 0
    finally:
        ctx.close()


def counter_fields(c):
    return {name: getattr(c, name) for name, _ in c._fields_ if name != "build_seconds"}


@pytest.mark.gpu
def test_feature_passes_between_render_calls_leave_the_frame_and_counters_identical():
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "glass")
    st = settings(96, 72, seed=3)
    ctx = binding.Context(stripes=1)
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        ctx.render(0, 16)
        whole = ctx.read_framebuffer()
        c0 = ctx.counters()
        ctx.render_begin(st)
        ctx.render(0, 8)
        ctx.render(8, 8)
        c_split = ctx.counters()
        ctx.render_begin(st)
        ctx.render_features(abi.FEATURE_ALL, 16)
        alone = read_all(ctx)
        ctx.render_begin(st)
        ctx.render(0, 8)
        ctx.render_features(abi.FEATURE_ALL, 16)
        ctx.render(8, 8)
        split = ctx.read_framebuffer()
        c1 = ctx.counters()
        assert_same_buffers(read_all(ctx), alone, "features around render calls")
    finally:
        ctx.close()
    assert (split.view(np.uint32) == whole.view(np.uint32)).all()
    assert (c0.samples, c0.extension_rays, c0.shadow_rays) == (c1.samples, c1.extension_rays, c1.shadow_rays)
    # every counter, the iteration count included, is that of the same two render calls without a feature pass between them; the
    # render's error word was clear at the end of each call (slrhip_render fails on a set word: Context.render raises)
    assert counter_fields(c1) == counter_fields(c_split)


def in_child(check):
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_features as T\nT.%s()\nprint('CHILD_OK')\n"
           % (ROOT, os.path.join(ROOT, "tests"), check))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (check, p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.gpu
def test_graph_captured_feature_pass_on_a_side_stream_replays_the_same_buffers():
    in_child("_graph_check")


def _graph_check():
    import torch
    sc = scenes.cornell_textured(1.0, 16, 8)
    st = settings(96, 72, seed=8)
    w, h = 96, 72
    ctx = binding.Context()
    try:
        ctx.upload_scene(sc)
        ctx.render_begin(st)
        ctx.render_features(abi.FEATURE_ALL, 8)
        want = read_all(ctx)
        ctx.render_begin(st)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.render_features(abi.FEATURE_ALL, 4, 0, stream=side)        # warm-up: allocates and clears, passes [0, 4)
            out = {c: torch.zeros((h, w, abi.FEATURE_CHANNELS[c][1]), dtype=torch.int32, device="cuda") for c in abi.FEATURE_CHANNELS}
            rows = torch.zeros((w * h, 8), dtype=torch.float32, device="cuda")
            count = C.c_uint32(0)
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                s = torch.cuda.current_stream()
                ctx.render_features(abi.FEATURE_ALL, 4, 4, stream=s)         # passes [4, 8)
                for c in out:
                    ctx.features_into(c, out[c].data_ptr(), out[c].numel(), stream=s)
                binding._check(ctx.lib, ctx.lib.slrhip_camera_rays(ctx.handle, 3, rows.data_ptr(), None, w * h, C.byref(count), s.cuda_stream), "camera_rays")
            g.replay()
            torch.cuda.synchronize()
        assert ctx.features_status(side) == 0 and count.value == w * h
        for c in out:
            got = out[c].cpu().numpy().view(np.uint32).reshape(want[c].shape)
            assert (got == want[c].view(np.uint32)).all(), abi.FEATURE_CHANNELS[c][0]
        assert (rows.cpu().numpy() == ctx.camera_rays(3)[0]).all()
        dev_rows, dev_xy = ctx.camera_rays(3, device=True)
        torch.cuda.synchronize()
        assert (dev_rows.cpu().numpy() == rows.cpu().numpy()).all() and (dev_xy.cpu().numpy().view(np.uint32) == ctx.camera_rays(3)[1]).all()
    finally:
        ctx.close()


# ---- host programs ----------------------------------------------------------------------------------------------------------------
FILES = {abi.FEATURE_GEOMETRIC_NORMAL: "geometric_normal.bmp", abi.FEATURE_SHADING_NORMAL: "shading_normal.bmp", abi.FEATURE_SHADING_TANGENT: "shading_tangent.bmp"}


def expected_bmp_bytes(ctx, channel, w, h):
    from slr_amd import host
    bgr = host.encode_normals(ctx.features(channel), ctx.features(abi.FEATURE_COVERAGE))
    rows = np.zeros((h, 3 * w + w % 4), np.uint8)
    rows[:, :3 * w] = bgr.reshape(h, 3 * w)
    return rows.reshape(-1)


@pytest.mark.gpu
def test_cpp_debug_renderer_writes_the_three_normal_images(tmp_path):
    """SLRHip::DebugRenderer (host/SLRHip.cpp) through the C++ host program: byte for byte the images the Python encoding makes of
    the same scene's feature buffers."""
    exe = os.path.join(ROOT, "slr_amd", "csrc", "host", "cornell_main")
    w, h, spp = 50, 36, 4
    tables = os.path.join(ROOT, "slr_amd", "data", "upsampling_tables.bin")
    out = subprocess.check_output([exe, str(spp), str(w), str(h), str(tmp_path), "rgb", tables, "debug"], text=True)
    assert len([l for l in out.splitlines() if l.startswith("debug:")]) == 3
    ctx = binding.Context()
    try:
        ctx.upload_scene(scenes.tiny_box(w / h))
        ctx.render_begin(settings(w, h, seed=abi.DEFAULT_SEED))
        ctx.render_features(NORMALS | abi.FEATURE_COVERAGE, spp)
        for c, name in FILES.items():
            raw = np.frombuffer(open(tmp_path / name, "rb").read(), np.uint8)
            want = expected_bmp_bytes(ctx, c, w, h)
            assert (raw[54:] == want).all() and len(np.unique(want)) > 3, name
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["--features", "debug renderer"])
def test_python_host_program_writes_feature_files(tmp_path, how):
    """python -m slr_amd.host: the beauty frames as before, and — with --features DIR, or for a scene whose renderer is "debug" — the
    normal BMPs and features.npz."""
    from test_scene_language import cornell_script
    text = cornell_script("matte").replace('"width": 320, "height": 240', '"width": 40, "height": 30')
    outputs = ("geometric_normal", "shading_normal", "shading_tangent")
    if how == "debug renderer":
        text = text.replace('setRenderer("method": "PT", ("samples": 64,));', 'setRenderer("method": "debug", ("samples": 64, "outputs": ("shading normal", "distance")));')
        assert '"debug"' in text
        outputs = ("shading_normal",)
    scene_file = tmp_path / "scene.txt"
    scene_file.write_text(text)
    feat = tmp_path / "feat" if how == "--features" else tmp_path
    cmd = ([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-m", "slr_amd.host", str(scene_file), "--samples", "2", "--out", str(tmp_path)]
           + (["--features", str(feat)] if how == "--features" else []))
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert os.path.exists(tmp_path / "001.bmp")
    z = np.load(feat / "features.npz")
    want_keys = [v[0] for v in abi.FEATURE_CHANNELS.values()] if how == "--features" else ["shading_normal", "distance", "coverage"]
    assert sorted(z.files) == sorted(want_keys)
    from slr_amd import host
    for c, name in FILES.items():
        if abi.FEATURE_CHANNELS[c][0] not in outputs:
            assert not os.path.exists(feat / name)
            continue
        raw = np.frombuffer(open(feat / name, "rb").read(), np.uint8)
        bgr = host.encode_normals(z[abi.FEATURE_CHANNELS[c][0]], z["coverage"])
        hh, ww, _ = bgr.shape
        assert (hh, ww) == (30, 40)
        rows = np.zeros((hh, 3 * ww + ww % 4), np.uint8)
        rows[:, :3 * ww] = bgr.reshape(hh, 3 * ww)
        assert (raw[54:] == rows.reshape(-1)).all() and len(np.unique(rows)) > 3, name
    assert z["coverage"].max() == 2


# ---- 6. loud failures --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_loud_failures():
    ctx = binding.Context()
    lib = ctx.lib
    count = C.c_uint32(0)
    try:
        with pytest.raises(binding.SlrHipError, match=r"\(4\).*render_begin"):
            ctx.render_features(abi.FEATURE_ALL, 1)
        ctx.upload_scene(scenes.tiny_box())
        with pytest.raises(binding.SlrHipError, match=r"\(4\).*render_begin"):
            ctx.render_features(abi.FEATURE_ALL, 1)
        with pytest.raises(binding.SlrHipError, match=r"\(4\).*render_begin"):
            ctx.camera_rays(0)
        assert lib.slrhip_resolve_features(ctx.handle, abi.FEATURE_IDS, 16, 0, None) == 4
        st = settings(32, 24)
        ctx.render_begin(st)
        with pytest.raises(binding.SlrHipError, match="unknown channel"):
            ctx.render_features(64, 1)
        with pytest.raises(binding.SlrHipError, match="unknown channel"):
            ctx.render_features(0, 1)
        ctx.render_features(abi.FEATURE_ALL, 0)                      # spp_count == 0 does nothing: no channel is marked
        with pytest.raises(binding.SlrHipError, match="asked for this channel"):
            ctx.features(abi.FEATURE_DISTANCE)
        ctx.render_features(abi.FEATURE_DISTANCE, 2)
        assert ctx.features(abi.FEATURE_DISTANCE).shape == (24, 32)
        with pytest.raises(binding.SlrHipError, match="channel set differs"):
            ctx.render_features(abi.FEATURE_DISTANCE | abi.FEATURE_IDS, 2, 2)
        with pytest.raises(binding.SlrHipError, match="asked for this channel"):
            ctx.features(abi.FEATURE_SHADING_NORMAL)
        with pytest.raises(binding.SlrHipError, match="one SLRHIP_FEATURE"):
            ctx.features_into(abi.FEATURE_DISTANCE | abi.FEATURE_IDS, 16, 1 << 20)
        with pytest.raises(binding.SlrHipError, match="too small"):
            ctx.features_into(abi.FEATURE_DISTANCE, 16, 32 * 24 - 1)
        with pytest.raises(binding.SlrHipError, match="misaligned"):
            ctx.features_into(abi.FEATURE_DISTANCE, 18, 1 << 20)
        with pytest.raises(binding.SlrHipError, match="null"):
            ctx.features_into(abi.FEATURE_DISTANCE, None, 1 << 20)
        assert lib.slrhip_camera_rays(ctx.handle, 0, 32, None, 32 * 24 - 1, C.byref(count), None) == 1 and count.value == 32 * 24
        assert b"capacity" in lib.slrhip_last_error_string()
        assert lib.slrhip_camera_rays(ctx.handle, 0, 40, None, 32 * 24, C.byref(count), None) == 1
        assert b"misaligned" in lib.slrhip_last_error_string()
        assert lib.slrhip_camera_rays(ctx.handle, 0, None, None, 32 * 24, C.byref(count), None) == 1
        assert b"null" in lib.slrhip_last_error_string()
        count.value = 0
        assert lib.slrhip_camera_rays(ctx.handle, 0, None, None, 0, C.byref(count), None) == 0 and count.value == 32 * 24      # the count alone
        ctx.render_begin(st)                                         # render_begin clears the accumulation and the channel set
        with pytest.raises(binding.SlrHipError, match="asked for this channel"):
            ctx.features(abi.FEATURE_DISTANCE)
    finally:
        ctx.close()
