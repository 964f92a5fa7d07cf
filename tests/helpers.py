import math
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from slr_amd import abi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


class _Prefixed:
    """View of an npz whose keys carry a prefix (several scenes in one fixture)."""
    def __init__(self, g, prefix):
        self.g, self.prefix = g, prefix
        self.files = [k[len(prefix):] for k in g.files if k.startswith(prefix)]

    def __getitem__(self, k):
        return self.g[self.prefix + k]


def scene_from_golden(g, name="golden", prefix=""):
    if prefix:
        g = _Prefixed(g, prefix)
    cam = abi.Camera()
    c = g["camera"]
    cam.local_to_world[:] = c[0:16].tolist()
    cam.world_to_local[:] = c[16:32].tolist()
    (cam.aspect, cam.fov_y, cam.lens_radius, cam.img_plane_distance, cam.obj_plane_distance,
     cam.sensitivity) = [float(v) for v in c[32:38]]
    env = None
    if "env_texels" in g.files:
        env = (g["env_texels"].astype(np.float32), float(g["env_scale"]), g["env_importance"])
        if "env_texels_uvs" in g.files:
            env = env + (g["env_texels_uvs"].astype(np.float32), g["env_importance_uvs"])
    textures = g["textures"] if "textures" in g.files else None
    texels = g["texture_texels"] if "texture_texels" in g.files else None
    texels_uvs = g["texture_texels_uvs"] if "texture_texels_uvs" in g.files else None
    instances = g["instances"] if "instances" in g.files else None
    return abi.Scene(g["vertices"], g["triangles"], g["materials"], g["spectra"], g["spectrum_data"], cam, env, name, textures=textures,
                     texture_texels=texels, texture_texels_uvs=texels_uvs, instances=instances)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_equal(a, b, what=""):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = bits(a) != bits(b)
    # +0 / -0 are the same radiance
    bad &= ~((a == 0) & (b == 0))
    assert not bad.any(), "%s: %d of %d floats differ, max abs diff %g" % (what, bad.sum(), bad.size, np.abs(a - b).max())


def summary_double_sum(values):
    """The fixed order of the double sums of slrhip_statistics_summary and slrhip_clamp_summary (include/slrhip.h) over per-pixel
    values in pixel-list order: per thread 16 pixels with stride 256 of a block of 4096, per wave the __shfl_down tree with offsets
    32 .. 1, thread 0 adds waves 1 .. 3, one thread adds the blocks in index order.  A pixel past the end adds zero."""
    x = np.asarray(values, np.float64)
    blocks = -(-x.size // 4096)
    x = np.concatenate([x, np.zeros(blocks * 4096 - x.size)]).reshape(blocks, 16, 256)
    total = 0.0
    with np.errstate(all="ignore"):
        for b in range(blocks):
            a = np.zeros(256)
            for k in range(16):
                a = a + x[b, k]
            a = a.reshape(4, 64)
            for off in (32, 16, 8, 4, 2, 1):
                a = a[:, :off] + a[:, off:2 * off]
            total = total + (((a[0, 0] + a[1, 0]) + a[2, 0]) + a[3, 0])
    return float(total)


def libm_tolerance(got, want, what, within=0.999, rtol=2e-6, rmse_rel=2e-5, cap=None):
    """Frames whose paths call float libm (GGX / Ward / Ashikhmin lobes, the environment sphere): the device math library is not
    glibc, so a sample moves by an ulp and — rarely — a discrete decision flips.  Stated tolerance: at least `within` of the
    floats inside `rtol` relative (thresholds one notch under the figures measured on MI355X: profiles/r03_a_parity_stats.jsonl,
    written by this function on the GPU box), RMSE <= `rmse_rel` x the mean (measured <= 1.3e-6; north_star's bound is 1e-3; on frames clipped at `cap` x the mean where single
    texels are hundreds of times the mean), everything finite."""
    import json
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), what
    close = float(np.isclose(got, want, rtol=rtol, atol=1e-9).mean())
    exact = float(((bits(got) == bits(want)) | ((got == 0) & (want == 0))).mean())
    a, b = got.astype(np.float64), want.astype(np.float64)
    if cap is not None:
        lim = cap * float(b.mean())
        a, b = np.minimum(a, lim), np.minimum(b, lim)
    rmse, mean = float(np.sqrt(np.mean((a - b) ** 2))), float(b.mean())
    out_dir = os.path.join(os.path.dirname(GOLDEN), os.pardir, "gpurun_out")
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, "parity_stats.jsonl"), "a") as f:
            f.write(json.dumps({"what": what, "within_%g" % rtol: close, "bit_exact": exact, "rmse_over_mean": rmse / max(mean, 1e-30)}) + "\n")
    assert close >= within, (what, "fraction within %g" % rtol, close, "bit-exact", exact)
    assert rmse <= rmse_rel * mean, (what, rmse, mean)


# ---- a tree-free reference for the ray queries (tests/test_traversal_edges.py) ---------------------------------------------
def _moller_trumbore(org, dirn, tmin, tmax, v0, e1, e2):
    """Triangle::intersect as pt_traverse.h:91-103 and slr_oracle.cpp:558-574 write it, every ray against every triangle, in the
    dtype of the inputs: org, dirn [c, 3], tmin, tmax [c], v0, e1, e2 [m, 3] -> ok (bool), t, b1, b2 [c, m].  cross is
    a.y*b.z - a.z*b.y ..., dot is (x + y) + z, invDet = 1 / det, and the rejections are the negated rejects of the C code, so
    that a NaN passes or fails exactly as it does there.  As in the C code, b2 and t are computed only for the pairs that pass
    the det and b1 tests (NaN elsewhere): that is most of the time on the 320 000-triangle grid."""
    T = org.dtype
    assert all(a.dtype == T for a in (dirn, tmin, tmax, v0, e1, e2))
    ox, oy, oz = (org[:, k, None] for k in range(3))
    dx, dy, dz = (dirn[:, k, None] for k in range(3))
    ax, ay, az = (v0[None, :, k] for k in range(3))
    e1x, e1y, e1z = (e1[None, :, k] for k in range(3))
    e2x, e2y, e2z = (e2[None, :, k] for k in range(3))
    with np.errstate(all="ignore"):
        px, py, pz = dy * e2z - dz * e2y, dz * e2x - dx * e2z, dx * e2y - dy * e2x          # p = cross(dir, e2)
        det = (e1x * px + e1y * py) + e1z * pz
        inv = T.type(1.0) / det
        sx, sy, sz = ox - ax, oy - ay, oz - az                                              # d = org - v0
        b1 = ((sx * px + sy * py) + sz * pz) * inv
        ok = (det != 0) & ~((b1 < 0) | (b1 > 1))
        r, k = np.nonzero(ok)                                                                # the pairs that go on
        sx, sy, sz, inv, b1k = sx[r, k], sy[r, k], sz[r, k], inv[r, k], b1[r, k]
        e1x, e1y, e1z, e2x, e2y, e2z = e1[k, 0], e1[k, 1], e1[k, 2], e2[k, 0], e2[k, 1], e2[k, 2]
        dx, dy, dz = dirn[r, 0], dirn[r, 1], dirn[r, 2]
        qx, qy, qz = sy * e1z - sz * e1y, sz * e1x - sx * e1z, sx * e1y - sy * e1x          # q = cross(d, e1)
        b2k = ((dx * qx + dy * qy) + dz * qz) * inv
        ttk = ((e2x * qx + e2y * qy) + e2z * qz) * inv
        okk = ~((b2k < 0) | (b1k + b2k > 1)) & ~((ttk < tmin[r]) | (ttk > tmax[r]))
    assert ttk.dtype == T and b1.dtype == T and b2k.dtype == T and det.dtype == T, "promoted silently"
    tt, b2 = np.full(b1.shape, np.nan, T), np.full(b1.shape, np.nan, T)
    tt[r, k], b2[r, k], ok[r, k] = ttk, b2k, okk
    return ok, tt, b1, b2


class BruteForce:
    """What brute_force_hits returns.  Candidates are (instance, triangle) pairs in ascending order, loose triangles as instance
    -1 first: cand_inst, cand_tri [m].  Per ray: hit [n] (some triangle accepts the ray in its own interval — test_visibility
    is its negation), tmin [n] (the minimum t with the winner's own bits — a tie at t = 0 may hold +0 and -0; inf on a miss), winner [n] (the LARGEST candidate of the tie set = the tie rule's answer, -1 on a
    miss).  The tie set (every candidate that accepts the ray at t == tmin) as parallel arrays over its entries: tie_ray,
    tie_cand, tie_t, tie_b0, tie_b1 — b0 = 1 - b1 - b2 and b1 as hitsToUV and the oracle report them — and tie_size [n].
    With keep_pairs: ok, t, b1, b2 [n, m]."""


def _candidate_groups(sc):
    tri = sc.triangles["v"]
    pos = sc.vertices["position"].astype(np.float32)
    mesh = np.zeros(len(tri), bool)
    for rec in sc.instances:
        mesh[int(rec["first_triangle"]):int(rec["first_triangle"]) + int(rec["num_triangles"])] = True
    groups = [(-1, np.nonzero(~mesh)[0], None)]
    for k, rec in enumerate(sc.instances):
        first, num = int(rec["first_triangle"]), int(rec["num_triangles"])
        groups.append((k, np.arange(first, first + num), rec["world_to_local"].astype(np.float32)))
    out = []
    for inst, idx, w2l in groups:
        v = pos[tri[idx]]                                    # [m, 3 corners, 3]
        out.append((inst, idx, w2l, v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]))
    return out


def _local_ray(w2l, org, dirn):
    """pt_traverse.h:60-64: the world-to-local matrix (column-major) times the origin as a point and the direction as a vector,
    float32, left to right."""
    if w2l is None:
        return org, dirn
    m = w2l
    one = np.float32(1.0)
    o = np.stack([m[r] * org[:, 0] + m[4 + r] * org[:, 1] + m[8 + r] * org[:, 2] + m[12 + r] * one for r in range(3)], axis=1)
    d = np.stack([m[r] * dirn[:, 0] + m[4 + r] * dirn[:, 1] + m[8 + r] * dirn[:, 2] for r in range(3)], axis=1)
    assert o.dtype == np.float32 and d.dtype == np.float32
    return o, d


def brute_force_hits(sc, rows, keep_pairs=False, dtype=np.float32, pairs_per_chunk=1 << 23):
    """The tree-free answer to a batch of ray queries: every ray of `rows` (slrhip_ray rows [n, 8]: org, dist_min, dir, dist_max)
    against every triangle of the scene with the float32 arithmetic the kernels promise (_moller_trumbore), no tree and no box.
    Instanced scenes: the ray goes into each instance's local space first (_local_ray), the test runs on the mesh's local
    triangles, dist_min / dist_max stay.  Alpha textures are not handled (the lattice scenes have none).  Rays are taken in
    chunks of pairs_per_chunk (ray, triangle) pairs: 32 MB per float32 temporary.  dtype=np.float64 evaluates the same formulas
    in double on the same inputs (the witness that the inputs are free of rounding ambiguity); instanced scenes: float32 only.
    No NaN or infinite origins or directions: what they return depends on the order of the tests, in the reference and on the
    device alike."""
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 8)
    assert sc.textures is None or len(sc.textures) == 0, "alpha textures are out of scope"
    T = np.dtype(dtype)
    groups = _candidate_groups(sc)
    assert T == np.float32 or len(groups) == 1
    cand_inst = np.concatenate([np.full(len(g[1]), g[0], np.int64) for g in groups])
    cand_tri = np.concatenate([g[1] for g in groups]).astype(np.int64)
    n, m = len(rows), len(cand_tri)
    out = BruteForce()
    out.cand_inst, out.cand_tri = cand_inst, cand_tri
    step = max(1, min(pairs_per_chunk // max(m, 1), -(-n // 8)))

    def chunk(lo):
        r = rows[lo:lo + step]
        org, dirn, tmin, tmax = r[:, 0:3], r[:, 4:7], r[:, 3], r[:, 7]
        parts = []
        for inst, idx, w2l, v0, e1, e2 in groups:
            o, d = _local_ray(w2l, org, dirn)
            parts.append(_moller_trumbore(o.astype(T), d.astype(T), tmin.astype(T), tmax.astype(T), v0.astype(T), e1.astype(T), e2.astype(T)))
        ok, tt, b1, b2 = (np.concatenate([p[k] for p in parts], axis=1) if len(parts) > 1 else parts[0][k] for k in range(4))
        best = np.where(ok, tt, T.type(np.inf)).min(axis=1)
        member = ok & (tt == best[:, None])
        ray, cand = np.nonzero(member)
        size = np.bincount(ray, minlength=len(r))
        hit = size > 0
        win = np.full(len(r), -1, np.int64)
        np.maximum.at(win, ray, cand)                     # the tie rule: the largest (instance, triangle) pair
        best[hit] = tt[np.nonzero(hit)[0], win[hit]]      # the winner's own bits: a tie at t = 0 may hold +0 and -0
        entries = (ray + lo, cand, tt[ray, cand], T.type(1.0) - b1[ray, cand] - b2[ray, cand], b1[ray, cand])
        return hit, best, win, size, entries, ((ok, tt, b1, b2) if keep_pairs else None)

    # numpy's loops release the interpreter lock: a few threads take the chunks side by side
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        done = list(pool.map(chunk, range(0, n, step)))
    cat = lambda k, empty: np.concatenate([d[k] for d in done]) if done else empty
    out.hit, out.tmin, out.winner, out.tie_size = cat(0, np.zeros(0, bool)), cat(1, np.zeros(0, T)), cat(2, np.zeros(0, np.int64)), cat(3, np.zeros(0, np.int64))
    for j, k in enumerate(("ray", "cand", "t", "b0", "b1")):
        setattr(out, "tie_" + k, np.concatenate([d[4][j] for d in done]) if done else np.zeros(0, T))
    assert out.tie_t.dtype == T and out.tie_b0.dtype == T and out.tie_b1.dtype == T and out.tmin.dtype == T
    assert len(out.hit) == n and (out.hit == (out.winner >= 0)).all() and (np.isinf(out.tmin) == ~out.hit).all()
    if keep_pairs:
        for j, k in enumerate(("ok", "t", "b1", "b2")):
            setattr(out, k, np.concatenate([d[5][j] for d in done]))
    return out


def ray_rows(org, direction, dist_min, dist_max):
    """[n, 8] float32 slrhip_ray rows."""
    org = np.asarray(org, np.float64).reshape(-1, 3)
    r = np.zeros((len(org), 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = org, dist_min, direction, dist_max
    return r


DIAGONALS = ((1, -1, 0), (-1, -1, 0), (0, -1, 1), (1, -1, 1), (1, -2, 0.5), (-0.5, -1, 2), (1, -0.25, 1), (2, -1, -2), (1, 0, 1), (-1, 0, 1))
INTERVALS = ("dmax=t", "dmin=t", "dmin=dmax=t", "dmax<t", "dmin>t", "dmin>dmax", "dmax=FLT_MAX", "dmin<0")


def special_rays(sc, n, coords=None, first_triangle=0, horizontal=True):
    """The rays a general-position family never holds, for a lattice scene of n x n cells (scenes.lattice_terrain; `sc` is needed
    for the intervals, which are cut at the brute-force distance, and for the points on its surface; first_triangle: where the
    terrain's triangles start; horizontal=False leaves axis_x and axis_z out: the quad deck is one plane, and they all miss it).  Returns (rows, tags): slrhip_ray rows and one tag "sub-family/case" per ray.  coords: the x and z
    values of the origins (default: every half-lattice point from -1/2 to n + 1/2; the large grid passes a few of them).

      axis_x, axis_y, axis_z  axis-parallel, both signs, from every half-lattice point of the opposite face — through vertices, edge
                  midpoints and cell centres, and along the scene's own bounding planes x = 0, x = n, z = 0, z = n, y = 4, where the
                  slab product is 0 * inf at the root — each with its zero components as +0.0 and again as -0.0; direction
                  lengths 1, 2, 1/2 in turn (directions need not be normalised)
      diagonal    ten directions with power-of-two components, each aimed at every lattice point (x, 1, z) from four steps back
      interval    the vertical rays that hit, sent again with dist_min / dist_max exactly at, one ulp either side of and around
                  the brute-force distance (exact: det = +-1, +-2 or 16 there), with FLT_MAX and with a negative dist_min
      surface     origins on a triangle's interior (v0 + e1/4 + e2/4, exact) with dist_min = 0: a hit at t = 0
      degenerate  rays lying in a triangle's plane (det == 0: a miss for that triangle) and zero directions (every det is 0)

    No NaN or infinite origins or directions: what they return depends on the order of the tests, in the reference and on the
    device alike."""
    inf = np.inf
    h = np.arange(-0.5, n + 0.75, 0.5) if coords is None else np.asarray(coords, np.float64)
    ints = h[(h == np.round(h)) & (h >= 0) & (h <= n)]
    yh = np.arange(0.0, 4.75, 0.5)
    rows, tags = [], []

    def add(r, tag):
        rows.append(r)
        tags.extend([tag] * len(r) if isinstance(tag, str) else tag)

    def axis_family(axis, a, b, far):
        """Origins (a_i, b_j) in the two other axes on both faces `far` = (low, high) of `axis`."""
        u, v = np.meshgrid(a, b, indexing="ij")
        u, v = u.reshape(-1), v.reshape(-1)
        others = [k for k in range(3) if k != axis]
        for face, sign in ((far[0], 1.0), (far[1], -1.0)):
            for zero, ztag in ((0.0, "+0"), (-0.0, "-0")):
                org = np.zeros((len(u), 3))
                org[:, axis], org[:, others[0]], org[:, others[1]] = face, u, v
                d = np.full((len(u), 3), zero)
                d[:, axis] = sign * np.array([1.0, 2.0, 0.5])[np.arange(len(u)) % 3]
                add(ray_rows(org, d, 0.0, inf), "axis_%s/%s%s" % ("xyz"[axis], "+" if sign > 0 else "-", ztag))

    axis_family(1, h, h, (-1.0, 6.0))            # others = (x, z)
    if horizontal:
        axis_family(0, yh, h, (-1.0, n + 1.0))       # others = (y, z)
        axis_family(2, h, yh, (-1.0, n + 1.0))       # others = (x, y)

    tx, tz = np.meshgrid(ints, ints, indexing="ij")
    target = np.stack([tx.reshape(-1), np.ones(tx.size), tz.reshape(-1)], axis=1)
    for d in DIAGONALS:
        d = np.array(d, np.float64)
        add(ray_rows(target - 4.0 * d, np.tile(d, (len(target), 1)), 0.0, inf), "diagonal/%g,%g,%g" % tuple(d))

    ux, uz = np.meshgrid(h, h, indexing="ij")
    org = np.stack([ux.reshape(-1), np.full(ux.size, 6.0), uz.reshape(-1)], axis=1)
    down = np.tile([0.0, -1.0, 0.0], (len(org), 1))
    t = brute_force_hits(sc, ray_rows(org, down, 0.0, inf)).tmin
    org, down, t = org[np.isfinite(t)], down[np.isfinite(t)], t[np.isfinite(t)]
    before, after = np.nextafter(t, np.float32(0.0)), np.nextafter(t, np.float32(inf))
    flt_max = np.finfo(np.float32).max
    for tag, dmin, dmax in zip(INTERVALS, (0.0, t, t, 0.0, after, t + np.float32(1.0), 0.0, -1.0), (t, inf, t, before, inf, t, flt_max, inf)):
        add(ray_rows(org, down, dmin, dmax), "interval/" + tag)

    tri = sc.triangles["v"][first_triangle:first_triangle + 2 * n * n]
    if coords is not None:
        tri = tri[:: max(1, len(tri) // 256)]
    p = sc.vertices["position"][tri].astype(np.float64)
    on = p[:, 0] + 0.25 * (p[:, 1] - p[:, 0]) + 0.25 * (p[:, 2] - p[:, 0])
    for d in ((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), (1.0, -1.0, 1.0)):
        add(ray_rows(on, np.tile(d, (len(on), 1)), 0.0, inf), "surface/%g,%g,%g" % d)

    k = len(ints)
    add(ray_rows(np.stack([np.full(k, -1.0), np.full(k, 4.0), ints], 1), np.tile([1.0, 0.0, 0.0], (k, 1)), 0.0, inf), "degenerate/quad plane from outside")
    add(ray_rows(np.stack([np.full(k, 1.0), np.full(k, 4.0), ints], 1), np.tile([1.0, 0.0, 0.0], (k, 1)), 0.0, inf), "degenerate/quad plane from inside")
    add(ray_rows(np.stack([ints, np.full(k, 4.0), np.full(k, n + 1.0)], 1), np.tile([-0.0, 0.0, -2.0], (k, 1)), 0.0, inf), "degenerate/quad plane along -z")
    wall_y = np.array([2.5, 3.0, 3.5, 4.5])
    add(ray_rows(np.stack([np.zeros(4), wall_y, np.full(4, -1.0)], 1), np.tile([0.0, 0.0, 1.0], (4, 1)), 0.0, inf), "degenerate/wall plane x=0")
    add(ray_rows(np.stack([np.full(4, 1.0), wall_y, np.full(4, float(n))], 1), np.tile([1.0, 0.0, 0.0], (4, 1)), 0.0, inf), "degenerate/wall plane z=n")
    add(ray_rows(np.stack([ints, np.full(k, 3.0), ints], 1), np.tile([1.0, 0.0, 1.0], (k, 1)), 0.0, inf), "degenerate/collinear triangle's line")
    add(ray_rows(np.stack([ints, np.full(k, 3.0), ints[::-1]], 1), np.zeros((k, 3)), 0.0, inf), "degenerate/zero direction")
    add(ray_rows(on[:k], np.full((len(on[:k]), 3), -0.0), 0.0, inf), "degenerate/zero direction on a surface")

    rows, tags = np.concatenate(rows), np.array(tags)
    assert len(rows) == len(tags) and np.isfinite(rows[:, [0, 1, 2, 4, 5, 6]]).all()
    return rows, tags


def every_kth(rows, tags, limit):
    """About `limit` rays: every k-th ray of each sub-family/case, so that none drops out; k is taken coprime to the case's size,
    so that the stride does not fall in step with the rows of the origins' grid."""
    keep = np.zeros(len(rows), bool)
    cases = sorted(set(tags))
    share = max(1, limit // len(cases))
    for c in cases:
        idx = np.nonzero(tags == c)[0]
        k = max(1, -(-len(idx) // share))
        while math.gcd(k, len(idx)) > 1 and k > 1:
            k -= 1
        keep[idx[::k][:share]] = True
    return rows[keep], tags[keep]


def sub_family(tags):
    return np.array([t.split("/")[0] for t in tags])


def rays_on_planes(rows, lo, hi):
    """Rays whose origin coordinate equals a bounding plane (lo / hi per axis) in an axis where the direction is zero: the slab
    product is 0 * inf = NaN there."""
    org, d = rows[:, 0:3], rows[:, 4:7]
    return ((d == 0) & ((org == np.asarray(lo, np.float32)) | (org == np.asarray(hi, np.float32)))).any(axis=1)
