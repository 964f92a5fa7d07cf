"""Temporal reprojection (slrhip_reproject / Context.reproject): the previous frame's history fetched along the motion vectors, tested
against the guides and blended with the current frame, as include/slrhip.h defines it.

The yardstick is a numpy float32 restatement of that definition, written here operation by operation (every intermediate is asserted
to be float32; no fused multiply-add exists in numpy), so every comparison is bit for bit (helpers.assert_bit_equal).

Synthetic inputs (np.random.default_rng(seed), no render): instance and material ids piecewise constant over interleaved regions (the
previous frame's shifted by a pixel), distance a slanted plane plus steps, normals piecewise constant plus noise, motion a smooth field
that matches the shift plus a region of large vectors that leave the image, coverage 0 on a diagonal band, history lengths 0 .. 40,
NaN and infinite pixels sprinkled into the history.  max_history 16, min_alpha 0.1, sigma_distance 0.05, min_normal_dot 0.9.

Input condition, asserted on the restatement BEFORE the GPU result is looked at, for the 37 x 21 case with every input given (1 x 1,
70 x 3 and 3 x 70 print their shares).  Shares as measured on the CPU (3 and 16 components share the guides; the last tap test reads
the colour):
    taps of the candidate pixels with b != 0, each test evaluated on its own (the guide tests on the taps inside the image):
        out of image 27.4 %   ids 15.6 %   distance 8.6 %   normal 16.9 %   history not finite 7.6 % (16 components: 8.0 %)
    pixels, 3 components:  rejected 41.1 %   accepted 58.9 %   clamped by max_history 41.1 %   min_alpha binds 51.0 %
    pixels, 16 components: rejected 41.2 %   accepted 58.8 %   clamped by max_history 40.5 %   min_alpha binds 50.8 %
Each of the first set and `rejected`, `clamped`, `binds` is required to be at least 5 %, `accepted` at least 25 %.

End to end (test_reprojected_frame_is_closer_to_the_converged_one): see that test's docstring for the measured values."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes, spectra
from slr_amd.binding import DeviceBlocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID = 1
FLT_MAX = F(3.402823466e+38)
PARAMS = dict(max_history=16.0, min_alpha=0.1, sigma_distance=0.05, min_normal_dot=0.9)
SHAPES = [(37, 21), (1, 1), (70, 3), (3, 70)]
OPTIONAL = ["all", "no_variance", "no_ids", "no_normal", "no_distance_test"]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def f32(*arrays):
    for a in arrays:
        assert np.asarray(a).dtype == F, np.asarray(a).dtype
    return arrays[0] if len(arrays) == 1 else arrays


def luminance(v):
    """Y of [..., 3] or [..., 16] float32, as include/slrhip.h states it for slrhip_sample_luminance."""
    v = np.asarray(v)
    f32(v)
    with np.errstate(all="ignore"):
        if v.shape[-1] == 3:
            d = v.astype(np.float64)
            return ((0.222485 * d[..., 0] + 0.716905 * d[..., 1]) + 0.060610 * d[..., 2]).astype(F)
        t = np.asarray(spectra.tables()["cmf16"], F)
        w, integral = t[16:32], F(t[48])
        p = [f32(((w[4 * q] * v[..., 4 * q] + w[4 * q + 1] * v[..., 4 * q + 1]) + w[4 * q + 2] * v[..., 4 * q + 2]) + w[4 * q + 3] * v[..., 4 * q + 3])
             for q in range(4)]
        return f32(((p[0] + p[1]) + (p[2] + p[3])) / integral)


def unit(n):
    with np.errstate(all="ignore"):
        length = f32(np.sqrt(f32(f32(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2])))
        return f32(np.where((length > 0)[..., None], f32(n / length[..., None]), F(0.0)))


def restate(color, motion, coverage, prev_color, prev_length, prev_distance, prev_coverage, variance=None, ids=None, normal=None,
            prev_variance=None, prev_ids=None, prev_normal=None, max_history=16.0, min_alpha=0.1, sigma_distance=0.05, min_normal_dot=0.9,
            stats=None):
    """(output, output_length, output_variance or None) of slrhip_reproject, float32 step by step.  stats (a dict) collects the counts
    of the input condition."""
    f32(color, motion, coverage, prev_color, prev_length, prev_distance, prev_coverage)
    h, w, comps = color.shape
    maxh, mina, sig, mind = F(max_history), F(min_alpha), F(sigma_distance), F(min_normal_dot)
    one, zero = F(1.0), F(0.0)
    var_p = variance if variance is not None else np.zeros((h, w), F)
    var_q = prev_variance if prev_variance is not None else np.zeros((h, w), F)
    counts = dict(taps=0, outside=0, ids=0, distance=0, normal=0, nonfinite=0)
    with np.errstate(all="ignore"):
        n = motion[..., 3]
        candidate = ~(coverage <= 0) & ~(n <= 0)
        mx, my, ze = f32(motion[..., 0] / n), f32(motion[..., 1] / n), f32(motion[..., 2] / n)
        fx = f32(np.arange(w, dtype=F)[None, :] + mx)
        fy = f32(np.arange(h, dtype=F)[:, None] + my)
        x0, y0 = f32(np.floor(fx)), f32(np.floor(fy))
        tx, ty = f32(fx - x0), f32(fy - y0)
        y_prev = luminance(prev_color)
        if normal is not None:
            n_p, n_prev = unit(normal), unit(prev_normal)
        z_prev = f32(prev_distance / prev_coverage)
        acc, acc_len, acc_var, total = np.zeros((h, w, comps), F), np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = f32(x0 + F(i)), f32(y0 + F(j))
                b = f32((tx if i else f32(one - tx)) * (ty if j else f32(one - ty)))
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                live = candidate & (b != 0)
                ix = np.where(inside, qx, zero).astype(np.int64)
                iy = np.where(inside, qy, zero).astype(np.int64)
                ok = live & inside & (prev_coverage[iy, ix] > 0) & (prev_length[iy, ix] > 0)
                counts["taps"] += int(live.sum())
                counts["outside"] += int((live & ~inside).sum())
                if ids is not None:
                    same = (prev_ids[iy, ix, 1] == ids[..., 1]) & (prev_ids[iy, ix, 2] == ids[..., 2])
                    counts["ids"] += int((live & inside & ~same).sum())
                    ok &= same
                if sig > 0:
                    near = np.abs(f32(z_prev[iy, ix] - ze)) <= f32(sig * ze)
                    counts["distance"] += int((live & inside & ~near).sum())
                    ok &= near
                if normal is not None:
                    nq = n_prev[iy, ix]
                    facing = f32(f32(n_p[..., 0] * nq[..., 0] + n_p[..., 1] * nq[..., 1]) + n_p[..., 2] * nq[..., 2]) >= mind
                    counts["normal"] += int((live & inside & ~facing).sum())
                    ok &= facing
                finite = np.abs(y_prev[iy, ix]) <= FLT_MAX
                counts["nonfinite"] += int((live & inside & ~finite).sum())
                ok &= finite
                total = f32(np.where(ok, f32(total + b), total))
                acc = f32(np.where(ok[..., None], f32(acc + f32(b[..., None] * prev_color[iy, ix])), acc))
                acc_len = f32(np.where(ok, f32(acc_len + f32(b * prev_length[iy, ix])), acc_len))
                acc_var = f32(np.where(ok, f32(acc_var + f32(b * var_q[iy, ix])), acc_var))
        accepted = candidate & ~(total <= 0)
        big_n = f32(np.fmin(f32(f32(acc_len / total) + one), maxh))
        alpha = f32(np.fmax(f32(one / big_n), mina))
        keep = f32(one - alpha)
        blended = f32(f32(keep[..., None] * f32(acc / total[..., None])) + f32(alpha[..., None] * color))
        blended_var = f32(f32(f32(alpha * alpha) * var_p) + f32(f32(keep * keep) * f32(acc_var / total)))
        output = f32(np.where(accepted[..., None], blended, color))
        length = f32(np.where(accepted, big_n, one))
        out_var = f32(np.where(accepted, blended_var, var_p)) if variance is not None else None
    if stats is not None:
        taps = max(counts["taps"], 1)
        stats.update({k: counts[k] / taps for k in ("outside", "ids", "distance", "normal", "nonfinite")})
        stats["rejected"], stats["accepted"] = float((~accepted).mean()), float(accepted.mean())
        with np.errstate(all="ignore"):
            stats["clamped"] = float((accepted & (f32(f32(acc_len / total) + one) > maxh)).mean())
            stats["binds"] = float((accepted & (f32(one / big_n) < mina)).mean())
    return output, length, out_var


# ---- synthetic inputs -----------------------------------------------------------------------------------------------------------------
def make_inputs(w, h, comps, seed=11):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]

    def regions(xx, yy):
        return ((xx // 5 + yy // 4) % 3).astype(np.int64)
    shift = (1, 0)                                        # the previous frame's content sat one pixel to the right: m = (+1, 0) finds it
    reg, reg_prev = regions(x, y), regions(x - shift[0], y - shift[1])
    ids = np.stack([rng.integers(0, 1000, (h, w)), reg, reg % 2 + 3], axis=-1).astype(np.uint32)
    prev_ids = np.stack([rng.integers(0, 1000, (h, w)), reg_prev, reg_prev % 2 + 3], axis=-1).astype(np.uint32)
    spp = 4.0

    def plane(xx, yy):
        return 5.0 + 0.05 * xx + 0.08 * yy + 1.5 * ((xx // 9) % 2)
    coverage = np.where((x + y) % 13 < 2, 0.0, spp).astype(F)
    prev_coverage = np.where((x - y) % 17 == 0, 0.0, spp).astype(F)
    dist_now = plane(x, y)
    prev_distance = (plane(x - shift[0], y - shift[1]) * (1.0 + rng.normal(0, 0.01, (h, w))) * prev_coverage).astype(F)
    normals = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.0, 0.8]])

    def noisy(r):
        v = normals[r] + rng.normal(0, 0.12, (h, w, 3))
        return (v * spp).astype(F)
    normal, prev_normal = noisy(reg), noisy(reg_prev)
    # motion: the shift plus a smooth sub-pixel field; a block of large vectors that leave the image; sums over `valid` samples
    valid = np.where(coverage > 0, rng.integers(1, int(spp) + 1, (h, w)), 0).astype(np.float64)
    mx = shift[0] + 0.6 * np.sin(0.3 * y) + 0.2 * np.cos(0.2 * x)
    my = shift[1] + 0.5 * np.cos(0.25 * x)
    far = (x >= w - max(1, w // 5)) | (y < max(0, h // 8))
    mx, my = np.where(far, mx + 3.0 * w, mx), np.where(far & (x % 2 == 0), my - 2.0 * h, my)
    motion = np.stack([mx * valid, my * valid, dist_now * (1.0 + rng.normal(0, 0.01, (h, w))) * valid, valid], axis=-1).astype(F)
    base = np.array([0.2, 0.7, 1.6])[reg]
    color = (base[..., None] * rng.uniform(0.5, 1.5, (h, w, comps))).astype(F)
    prev_color = (np.array([0.2, 0.7, 1.6])[reg_prev][..., None] * rng.uniform(0.8, 1.2, (h, w, comps))).astype(F)
    bad = rng.uniform(0, 1, (h, w)) < 0.12
    prev_color[bad, rng.integers(0, comps, int(bad.sum()))] = np.where(rng.uniform(0, 1, int(bad.sum())) < 0.5, np.nan, np.inf)
    prev_length = np.where(rng.uniform(0, 1, (h, w)) < 0.1, 0, rng.integers(0, 41, (h, w))).astype(F)
    variance = np.exp2(rng.uniform(-10, -2, (h, w))).astype(F)
    prev_variance = np.exp2(rng.uniform(-12, -4, (h, w))).astype(F)
    return dict(color=color, motion=motion, coverage=coverage, prev_color=prev_color, prev_length=prev_length, prev_distance=prev_distance,
                prev_coverage=prev_coverage, variance=variance, ids=ids, normal=normal, prev_variance=prev_variance, prev_ids=prev_ids,
                prev_normal=prev_normal)


def variant(inputs, which):
    a, p = dict(inputs), dict(PARAMS)
    if which == "no_variance":
        a["variance"] = a["prev_variance"] = None
    elif which == "no_ids":
        a["ids"] = a["prev_ids"] = None
    elif which == "no_normal":
        a["normal"] = a["prev_normal"] = None
    elif which == "no_distance_test":
        p["sigma_distance"] = 0.0
    return a, p


def check_condition(stats, what):
    print("%s: taps: " % what + "  ".join("%s %.1f %%" % (k, 100 * stats[k]) for k in ("outside", "ids", "distance", "normal", "nonfinite"))
          + ";  pixels: " + "  ".join("%s %.1f %%" % (k, 100 * stats[k]) for k in ("rejected", "accepted", "clamped", "binds")))
    for k in ("outside", "ids", "distance", "normal", "nonfinite", "rejected", "clamped", "binds"):
        assert stats[k] >= 0.05, (what, k, stats[k])
    assert stats["accepted"] >= 0.25, (what, stats["accepted"])


# ---------------------------------------------------------------- CPU --------------------------------------------------------------------
def test_exports_header_and_layout():
    lib = binding.load_library()
    for name in ("slrhip_reproject", "slrhip_debug_reproject_check"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert "#define SLRHIP_VERSION 7 " in header and lib.slrhip_version() == 7
    for text in ("typedef struct slrhip_reproject_desc {", "fx = (float)x + m.x;  x0 = floorf(fx);  tx = fx - x0", "the + 0.5 and the - 0.5 cancel",
                 "b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty)", "fabsf(prev_distance_q / prev_coverage_q - z_e) <= sigma_distance * z_e",
                 "N = fminf(len + 1.0f, max_history);  a = fmaxf(1.0f / N, min_alpha)", "output[k] = (1.0f - a) * hist[k] + a * color[k]",
                 "output_variance = (a * a) * variance_p + ((1.0f - a) * (1.0f - a)) * vhist", "moment-based temporal variance",
                 "reprojecting the environment under camera rotation"):
        assert text in header, text
    # uint32 width, height, components; (pad); 13 input pointers; 3 output pointers; 4 floats; uint32 reserved[2]
    d = abi.ReprojectDesc
    assert C.sizeof(d) == 168 and d.width.offset == 0 and d.components.offset == 8 and d.color.offset == 16 and d.normal.offset == 56
    assert d.prev_color.offset == 64 and d.prev_normal.offset == 112 and d.output.offset == 120 and d.output_length.offset == 136
    assert d.max_history.offset == 144 and d.min_normal_dot.offset == 156 and d.reserved.offset == 160


def good_desc(w=8, h=4, comps=3, base=1 << 20):
    """A descriptor that passes, over made-up addresses a megabyte apart (the check compares pointers and never follows them)."""
    names = ["color", "variance", "motion", "coverage", "ids", "normal", "prev_color", "prev_variance", "prev_length", "prev_distance",
             "prev_coverage", "prev_ids", "prev_normal", "output", "output_variance", "output_length"]
    a = dict(width=w, height=h, components=comps, reserved=(0, 0), **PARAMS)
    a.update({n: base * (k + 1) for k, n in enumerate(names)})
    return a


def desc_of(a):
    return abi.ReprojectDesc(a["width"], a["height"], a["components"], a["color"], a["variance"], a["motion"], a["coverage"], a["ids"], a["normal"],
                             a["prev_color"], a["prev_variance"], a["prev_length"], a["prev_distance"], a["prev_coverage"], a["prev_ids"],
                             a["prev_normal"], a["output"], a["output_variance"], a["output_length"], a["max_history"], a["min_alpha"],
                             a["sigma_distance"], a["min_normal_dot"], (C.c_uint32 * 2)(*a["reserved"]))


def refusals(a):
    """Every refusal of include/slrhip.h's list, as overrides of the good descriptor `a`."""
    nan = float("nan")
    frame, plane = 4 * a["width"] * a["height"] * a["components"], 4 * a["width"] * a["height"]
    out = [("zero width", dict(width=0)), ("zero height", dict(height=0)), ("2^31 pixels", dict(width=1 << 16, height=1 << 15)),
           ("components 4", dict(components=4)), ("components 0", dict(components=0)),
           ("reserved[0]", dict(reserved=(1, 0))), ("reserved[1]", dict(reserved=(0, 1))),
           ("NaN max_history", dict(max_history=nan)), ("NaN min_alpha", dict(min_alpha=nan)), ("NaN sigma_distance", dict(sigma_distance=nan)),
           ("NaN min_normal_dot", dict(min_normal_dot=nan)), ("max_history < 1", dict(max_history=0.5)),
           ("min_alpha < 0", dict(min_alpha=-0.01)), ("min_alpha > 1", dict(min_alpha=1.01)),
           ("variance without prev_variance", dict(prev_variance=None, output_variance=None)),
           ("prev_variance without variance", dict(variance=None, output_variance=None)),
           ("output_variance without variance", dict(variance=None, prev_variance=None)),
           ("ids without prev_ids", dict(prev_ids=None)), ("prev_ids without ids", dict(ids=None)),
           ("normal without prev_normal", dict(prev_normal=None)), ("prev_normal without normal", dict(normal=None))]
    for name in ("color", "motion", "coverage", "prev_color", "prev_length", "prev_distance", "prev_coverage", "output", "output_length"):
        out.append(("null " + name, {name: None}))
    for name in ("color", "variance", "motion", "coverage", "ids", "normal", "prev_color", "prev_variance", "prev_length", "prev_distance",
                 "prev_coverage", "prev_ids", "prev_normal", "output", "output_variance", "output_length"):
        out.append(("misaligned " + name, {name: a[name] + 2}))
    sizes = dict(color=frame, variance=plane, motion=4 * plane, coverage=plane, ids=3 * plane, normal=3 * plane, prev_color=frame,
                 prev_variance=plane, prev_length=plane, prev_distance=plane, prev_coverage=plane, prev_ids=3 * plane, prev_normal=3 * plane)
    for name, size in sizes.items():
        out.append(("output = " + name, dict(output=a[name])))                                   # in place: refused
        out.append(("output_length ends in " + name, dict(output_length=a[name] - plane + 4)))   # the last float overlaps the first
        out.append(("output_variance begins in the last float of " + name, dict(output_variance=a[name] + size - 4)))
    out += [("output_variance inside output", dict(output_variance=a["output"] + frame - 4)), ("output_length = output", dict(output_length=a["output"])),
            ("output_length = output_variance", dict(output_length=a["output_variance"]))]
    return out


REFUSALS = refusals(good_desc())


def test_good_descriptors_pass_the_check():
    lib = binding.load_library()
    a = good_desc()
    assert lib.slrhip_debug_reproject_check(C.byref(desc_of(a))) == 0
    # optional inputs absent; buffers that touch without overlapping; the limits of the parameters; 16 components
    frame, plane = 4 * a["width"] * a["height"] * a["components"], 4 * a["width"] * a["height"]
    for over in (dict(variance=None, prev_variance=None, output_variance=None), dict(output_variance=None), dict(ids=None, prev_ids=None),
                 dict(normal=None, prev_normal=None), dict(output=a["color"] + frame), dict(output_length=a["output"] + frame),
                 dict(output_variance=a["coverage"] - plane), dict(max_history=1.0, min_alpha=0.0), dict(min_alpha=1.0, sigma_distance=-1.0),
                 dict(max_history=float("inf"), min_normal_dot=-2.0), dict(components=16)):
        assert lib.slrhip_debug_reproject_check(C.byref(desc_of(dict(a, **over)))) == 0, (over, lib.slrhip_last_error_string())
    assert lib.slrhip_debug_reproject_check(None) == INVALID and lib.slrhip_reproject(None, C.byref(desc_of(a)), None) == INVALID


@pytest.mark.parametrize("what, over", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_through_the_check(what, over):
    lib = binding.load_library()
    rc = lib.slrhip_debug_reproject_check(C.byref(desc_of(dict(good_desc(), **over))))
    assert rc == INVALID and lib.slrhip_last_error_string().decode().startswith("slrhip_reproject: "), (what, rc)


def test_restatement_input_condition():
    """The shares of the module docstring, on the CPU: the inputs exercise every branch of the definition."""
    for comps in (3, 16):
        stats = {}
        out, length, var = restate(**make_inputs(37, 21, comps), **PARAMS, stats=stats)
        check_condition(stats, "37 x 21, %d components" % comps)
        assert np.isfinite(out).all() and np.isfinite(var).all() and (length >= 1).all() and (length <= F(PARAMS["max_history"])).all()


# ---------------------------------------------------------------- GPU --------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = Context(device=0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", OPTIONAL)
@pytest.mark.parametrize("comps", [3, 16])
@pytest.mark.parametrize("w, h", SHAPES)
def test_reproject_equals_the_restatement(ctx, w, h, comps, which):
    inputs, params = variant(make_inputs(w, h, comps), which)
    stats = {}
    want = restate(**inputs, **params, stats=stats)
    if (w, h) == (37, 21) and which == "all":
        check_condition(stats, "%d x %d x %d" % (w, h, comps))
    got = ctx.reproject(**inputs, **params)
    assert len(got) == (3 if inputs["variance"] is not None else 2)
    assert_bit_equal(got[0], want[0], "output")
    assert_bit_equal(got[1], want[1], "output_length")
    if inputs["variance"] is not None:
        assert_bit_equal(got[2], want[2], "output_variance")


@pytest.mark.gpu
@pytest.mark.parametrize("comps", [3, 16])
def test_unaligned_buffers_give_the_same_result(ctx, comps):
    """Buffers that are 4-byte but not 16-byte aligned take the scalar loads: the same bits."""
    w, h = 37, 21
    inputs = make_inputs(w, h, comps)
    want = restate(**inputs, **PARAMS)
    with DeviceBlocks() as dev:
        ptrs = {}
        for name, a in inputs.items():
            block = dev.alloc(a.nbytes + 16)
            binding._hip_check(dev.hip.hipMemcpy(block + 4, np.ascontiguousarray(a).ctypes.data, a.nbytes, 1), "hipMemcpy")
            ptrs[name] = block + 4
        output, length, var = dev.alloc(4 * w * h * comps + 16) + 4, dev.alloc(4 * w * h + 16) + 12, dev.alloc(4 * w * h + 16) + 8
        ctx.reproject_into(w, h, comps, output=output, output_length=length, output_variance=var, **ptrs, **PARAMS)
        ctx.synchronize()
        assert_bit_equal(dev.get(output, (h, w, comps)), want[0], "output")
        assert_bit_equal(dev.get(length, (h, w)), want[1], "output_length")
        assert_bit_equal(dev.get(var, (h, w)), want[2], "output_variance")


@pytest.mark.gpu
@pytest.mark.parametrize("comps", [3, 16])
def test_zero_motion_blends_pixel_by_pixel_and_counts_the_frames(ctx, comps):
    w, h = 19, 11
    rng = np.random.default_rng(5)
    spp = F(4.0)
    coverage = np.full((h, w), spp, F)
    distance = (rng.uniform(2, 9, (h, w)) * 4).astype(F)
    normal = (rng.normal(0, 1, (h, w, 3)) * 4).astype(F)
    ids = rng.integers(0, 50, (h, w, 3)).astype(np.uint32)
    motion = np.zeros((h, w, 4), F)
    motion[..., 2], motion[..., 3] = distance, spp         # z_e = distance / spp, the tap's own distance
    params = dict(max_history=1e9, min_alpha=0.0, sigma_distance=0.05, min_normal_dot=0.9)
    guides = dict(motion=motion, coverage=coverage, prev_distance=distance, prev_coverage=coverage, ids=ids, prev_ids=ids, normal=normal,
                  prev_normal=normal)
    # one step on a history of given lengths: exactly (1 - a) prev + a cur with a = 1 / (len + 1)
    prev, cur = rng.uniform(0, 2, (h, w, comps)).astype(F), rng.uniform(0, 2, (h, w, comps)).astype(F)
    lengths = rng.integers(1, 30, (h, w)).astype(F)
    out, length = ctx.reproject(cur, prev_color=prev, prev_length=lengths, **guides, **params)
    a = F(1.0) / (lengths + F(1.0))
    assert a.dtype == F
    assert_bit_equal(out, (F(1.0) - a)[..., None] * prev + a[..., None] * cur, "one blend")
    assert_bit_equal(length, lengths + F(1.0), "the length")
    # six frames of a constant plus noise, the outputs fed back: the length counts 1 .. 6 and the history is the running mean
    history, lengths = np.zeros((h, w, comps), F), np.zeros((h, w), F)
    truth = rng.uniform(0.5, 1.5, (h, w, comps))
    total = np.zeros((h, w, comps))
    for frame in range(1, 7):
        cur = (truth + rng.normal(0, 0.2, (h, w, comps))).astype(F)
        total += cur
        history, lengths = ctx.reproject(cur, prev_color=history, prev_length=lengths, **guides, **params)
        assert (lengths == frame).all(), frame
        assert np.abs(history - total / frame).max() <= 1e-5
    assert np.abs(history - truth).mean() < 0.6 * 0.2 * np.sqrt(2 / np.pi)


@pytest.mark.gpu
def test_refused_call_writes_nothing_and_good_call_allocates_nothing(ctx):
    w, h, comps = 37, 21, 3
    inputs = make_inputs(w, h, comps)
    want = restate(**inputs, **PARAMS)
    hip = binding._hip_runtime()
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]

    def free_bytes():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    with DeviceBlocks() as dev:
        ptrs = {name: dev.put(a) for name, a in inputs.items()}
        sentinel = np.full(w * h * comps, -7.5, F)
        outs = dict(output=dev.put(sentinel), output_length=dev.put(sentinel[:w * h]), output_variance=dev.put(sentinel[:w * h]))
        good = dict(width=w, height=h, components=comps, reserved=(0, 0), **PARAMS, **ptrs, **outs)
        for what, over in (("max_history < 1", dict(max_history=0.0)), ("in place", dict(output=ptrs["prev_color"])),
                           ("NaN min_alpha", dict(min_alpha=float("nan"))), ("reserved", dict(reserved=(0, 3))),
                           ("ids without prev_ids", dict(prev_ids=None)), ("misaligned", dict(output_length=outs["output_length"] + 2))):
            assert ctx.lib.slrhip_reproject(ctx.handle, C.byref(desc_of(dict(good, **over))), None) == INVALID, what
        ctx.synchronize()
        for name, n in (("output", w * h * comps), ("output_length", w * h), ("output_variance", w * h)):
            assert (dev.get(outs[name], (n,)) == F(-7.5)).all(), name
        for name, a in inputs.items():
            assert (dev.get(ptrs[name], a.shape, a.dtype).view(np.uint8) == a.view(np.uint8)).all(), name
        assert ctx.lib.slrhip_reproject(ctx.handle, C.byref(desc_of(good)), None) == 0
        ctx.synchronize()
        before = free_bytes()
        assert ctx.lib.slrhip_reproject(ctx.handle, C.byref(desc_of(good)), None) == 0
        ctx.synchronize()
        assert free_bytes() == before, "the call allocates nothing"
        assert_bit_equal(dev.get(outs["output"], (h, w, comps)), want[0], "after the refusals")


def in_child(check):
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_reproject as T\nT.%s()\nprint('CHILD_OK')\n"
           % (ROOT, os.path.join(ROOT, "tests"), check))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (check, p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.gpu
def test_graph_captured_call_replays_the_eager_result():
    """The FIRST reproject call of a context, captured in a graph on a side stream: the replay's outputs equal the eager call's."""
    in_child("_graph_check")


def _graph_check():
    import torch
    w, h, comps = 37, 21, 16
    inputs = make_inputs(w, h, comps)
    want = restate(**inputs, **PARAMS)
    c = Context()
    try:
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            dev = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in inputs.items()}
            outs = {k: torch.full(shape, -1.0, dtype=torch.float32, device="cuda") for k, shape in
                    (("output", (h, w, comps)), ("output_length", (h, w)), ("output_variance", (h, w)))}
            side.synchronize()
            args = dict({k: v.data_ptr() for k, v in dev.items()}, **{k: v.data_ptr() for k, v in outs.items()})
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                c.reproject_into(w, h, comps, stream=torch.cuda.current_stream(), **args, **PARAMS)
            assert (outs["output"].cpu().numpy() == -1.0).all(), "a captured call does not run"
            g.replay()
            torch.cuda.synchronize()
            graph = {k: v.cpu().numpy() for k, v in outs.items()}
            for v in outs.values():
                v.fill_(-1.0)
            c.reproject_into(w, h, comps, stream=side, **args, **PARAMS)
            torch.cuda.synchronize()
        for k, ref in (("output", want[0]), ("output_length", want[1]), ("output_variance", want[2])):
            eager = outs[k].cpu().numpy()
            assert (graph[k].view(np.uint32) == eager.view(np.uint32)).all(), k
            assert_bit_equal(eager, ref, k)
    finally:
        c.close()


# ---- end to end: two frames of a moving scene ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_reprojected_frame_is_closer_to_the_converged_one():
    """cornell_instanced at 64 x 64.  Frame 1 at 4 spp; then the instances move by small translations and the camera a little; frame 2
    at 4 spp, reprojected onto frame 1 with the guides and the motion vectors of the library.  Its luminance RMSE against a 256-spp
    frame 2 of the same context must be strictly lower than that of frame 2 alone (the only claim: the yardstick is the frame that was
    not accumulated).
    Measured on MI355X: RMSE of frame 2 alone 1.14453e-3, reprojected onto frame 1 1.14186e-3; accepted pixels 96.6 %.  At 4 spp the
    RMSE is the energy of a few fireflies (it equals the mean luminance, 9.5e-4): the blend halves this frame's and brings in the
    other's at half weight.  The bulk does what two frames should: the median absolute error falls from 7.78e-5 to 5.82e-5, the largest
    from 0.0407 to 0.0266 (printed by the test)."""
    from test_motion import moved_camera, placed, records
    size, spp = 64, 4
    sc = scenes.cornell_instanced(1.0, 10, 5, copies=24)
    rec1 = records(sc)
    rng = np.random.default_rng(5)
    rec2 = placed(rec1, rng.uniform(-0.03, 0.03, (len(rec1), 3)))
    cam2 = moved_camera(sc.camera, (0.04, 0.02, -0.05))
    want_features = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE | abi.FEATURE_IDS
    c = Context(device=0)
    try:
        c.upload_scene(sc)

        def frame(seed, passes, motion_from=None):
            c.render_begin(ob.settings(size, size, seed=seed))
            c.render(0, passes)
            out = dict(color=c.read_framebuffer() / F(passes))
            if passes == spp:
                c.render_features(want_features, passes)
                out.update(normal=c.features(abi.FEATURE_SHADING_NORMAL), distance=c.features(abi.FEATURE_DISTANCE),
                           coverage=c.features(abi.FEATURE_COVERAGE), ids=c.features(abi.FEATURE_IDS))
                if motion_from is not None:
                    c.render_motion(passes, *motion_from)
                    out["motion"] = c.motion()
            return out
        one = frame(21, spp)
        c.set_instance_transforms(rec2)
        c.set_camera(cam2)
        assert c.instances_status() == 0
        two = frame(22, spp, (sc.camera, rec1))
        truth = frame(23, 256)["color"]
        out, length = c.reproject(two["color"], two["motion"], two["coverage"], prev_color=one["color"], prev_length=np.ones((size, size), F),
                                  prev_distance=one["distance"], prev_coverage=one["coverage"], ids=two["ids"], prev_ids=one["ids"],
                                  normal=two["normal"], prev_normal=one["normal"])
    finally:
        c.close()
    y_true = luminance(truth).astype(np.float64)
    alone = float(np.sqrt(np.mean((luminance(two["color"]) - y_true) ** 2)))
    reprojected = float(np.sqrt(np.mean((luminance(out) - y_true) ** 2)))
    accepted = float((length > 1).mean())
    e_alone, e_out = np.abs(luminance(two["color"]) - y_true), np.abs(luminance(out) - y_true)
    print("mean luminance %.6g; |error| alone / reprojected: median %.6g / %.6g, 99th percentile %.6g / %.6g, largest %.6g / %.6g"
          % (y_true.mean(), np.median(e_alone), np.median(e_out), np.percentile(e_alone, 99), np.percentile(e_out, 99), e_alone.max(), e_out.max()))
    print("luminance RMSE against 256 spp: frame 2 alone %.6g, reprojected onto frame 1 %.6g; accepted pixels %.1f %%" % (alone, reprojected, 100 * accepted))
    assert accepted >= 0.25, "the reprojection has to have happened"
    assert reprojected < alone
