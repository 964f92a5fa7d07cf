"""The denoiser (slrhip_denoise / Context.denoise / Context.denoised): the variance-guided a-trous filter of include/slrhip.h.

The yardstick is a numpy float32 restatement of that definition, written here operation by operation (every intermediate is
asserted to be float32; no fused multiply-add exists in numpy), so every comparison is bit for bit (helpers.assert_bit_equal).

Synthetic inputs (np.random.default_rng(seed), no render): coverage 0 on diagonal bands (a quarter of the pixels), normals piecewise
constant over three interleaved regions plus noise, distance a slanted plane plus steps, colour piecewise constant plus noise whose
standard deviation differs per region, variance = the variance of that noise's luminance.  sigma_luminance 4, sigma_distance 0.02,
normal_power_log2 7.

Input condition, asserted on the restatement BEFORE the GPU result is looked at, for the 37 x 21 case with 5 iterations (the case
the shares below were chosen on; 1 x 1 has no non-centre tap at all, 70 x 3 and 3 x 70 have every vertical / horizontal tap outside
the image from s = 2 on, and one iteration at 130 x 66 loses under 5 % of its taps to the image border: for those shapes the shares
are printed, not asserted).  Shares of the in-image non-centre taps of all iterations, measured on the CPU:
    37 x 21, 5 iterations, 3 components (seed 11)
        w_n == 0: 12.6 %   0 < w_n < 1: 43.7 %      w_z == 0: 25.8 %   0 < w_z < 1: 30.5 %      w_l == 0: 28.0 %   0 < w_l < 1: 35.0 %
        skipped for a hit-class mismatch: 37.0 %;  out of image at the last iteration (of the 24 non-centre taps of every pixel): 89.4 %
    37 x 21, 5 iterations, 16 components (seed 11)
        w_n, w_z, mismatch, out of image: as above (the guides are the same);  w_l == 0: 30.9 %   0 < w_l < 1: 32.1 %
Each is required to be at least 5 %.

Quality (test_denoised_frame_is_closer_to_the_converged_one): see that test's docstring for the two measured values."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, host, scenes, spectra

F = np.float32
H5 = [F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16)]
G3 = [F(1 / 4), F(1 / 2), F(1 / 4)]
SIGMA_L, SIGMA_D, POWER = 4.0, 0.02, 7


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def cmf16():
    t = np.asarray(spectra.tables()["cmf16"], F)
    return t[16:32].copy(), F(t[48])


def luminance(v):
    """Y of [..., 3] or [..., 16] float32, as include/slrhip.h states it for slrhip_sample_luminance."""
    v = np.asarray(v)
    assert v.dtype == F
    with np.errstate(all="ignore"):
        if v.shape[-1] == 3:
            d = v.astype(np.float64)
            return ((0.222485 * d[..., 0] + 0.716905 * d[..., 1]) + 0.060610 * d[..., 2]).astype(F)
        w, integral = cmf16()
        p = []
        for q in range(4):
            a = ((w[4 * q] * v[..., 4 * q] + w[4 * q + 1] * v[..., 4 * q + 1]) + w[4 * q + 2] * v[..., 4 * q + 2]) + w[4 * q + 3] * v[..., 4 * q + 3]
            assert a.dtype == F
            p.append(a)
        y = ((p[0] + p[1]) + (p[2] + p[3])) / integral
    assert y.dtype == F
    return y


def shifted(a, oy, ox):
    """(b, inside): b[y, x] = a[y + oy, x + ox] where that is inside the image (0 elsewhere), and the mask of those pixels."""
    h, w = a.shape[:2]
    b, inside = np.zeros_like(a), np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return b, inside


def f32(*arrays):
    for a in arrays:
        assert a.dtype == F, a.dtype
    return arrays[0] if len(arrays) == 1 else arrays


def restate(color, variance=None, normal=None, distance=None, coverage=None, iterations=5, sigma_luminance=SIGMA_L, sigma_distance=SIGMA_D,
            normal_power_log2=POWER, stats=None):
    """(output, output_variance) of slrhip_denoise, float32 step by step.  stats (a dict) collects the tap counts of the input
    condition."""
    color = np.asarray(color)
    assert color.dtype == F and all(a is None or np.asarray(a).dtype == F for a in (variance, normal, distance, coverage))
    h, w, comps = color.shape
    sl, sd_ = F(sigma_luminance), F(sigma_distance)
    stop_l = variance is not None and sl > 0
    stop_n = normal is not None
    stop_z = distance is not None and sd_ > 0
    counts = dict(taps=0, mismatch=0, n0=0, n01=0, z0=0, z01=0, l0=0, l01=0, last_taps=0, last_outside=0)
    with np.errstate(all="ignore"):
        # guides
        hit = coverage > 0 if coverage is not None else np.zeros((h, w), bool)
        if stop_n:
            nx, ny, nz = normal[..., 0], normal[..., 1], normal[..., 2]
            length = f32(np.sqrt((nx * nx + ny * ny) + nz * nz))
            n = np.where((hit & (length > 0))[..., None], normal / length[..., None], F(0))
            f32(n)
        if distance is not None:
            z = f32(np.where(hit, distance / coverage, F(0)))
        c, v = color, (variance if variance is not None else np.zeros((h, w), F))
        for i in range(iterations):
            s = 1 << i
            y = luminance(c)
            if stop_l:
                num, den = np.zeros((h, w), F), np.zeros((h, w), F)
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        vq, inside = shifted(v, dy, dx)
                        g = G3[dx + 1] * G3[dy + 1]
                        num, den = np.where(inside, num + g * vq, num), np.where(inside, den + g, den)
                sd = np.sqrt(np.fmax(F(0), num / den))
                denom = sl * sd + F(1e-20)
                f32(num, den, sd, denom)
            acc, acc_v, sum_w = np.zeros((h, w, comps), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, inside = shifted(c, dy * s, dx * s)
                    vq, _ = shifted(v, dy * s, dx * s)
                    wgt = np.full((h, w), H5[dx + 2] * H5[dy + 2], F)
                    take = inside
                    if dx or dy:
                        hit_q, _ = shifted(hit, dy * s, dx * s)
                        take = inside & (hit_q == hit)
                        counts["taps"] += int(inside.sum())
                        counts["mismatch"] += int((inside & (hit_q != hit)).sum())
                        if i == iterations - 1:
                            counts["last_taps"] += h * w
                            counts["last_outside"] += int((~inside).sum())
                        if stop_n:
                            nq, _ = shifted(n, dy * s, dx * s)
                            t = np.fmax(F(0), (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2])
                            for _k in range(normal_power_log2):
                                t = t * t
                            wgt = wgt * np.where(hit, f32(t), F(1))
                            counts["n0"] += int((take & hit & (t == 0)).sum())
                            counts["n01"] += int((take & hit & (t > 0) & (t < 1)).sum())
                        if stop_z:
                            zq, _ = shifted(z, dy * s, dx * s)
                            d = F(s * max(abs(dx), abs(dy)))
                            x = np.abs(z - zq) / ((sd_ * d) * z)
                            t = np.fmax(F(0), F(1) - x)
                            wz = f32(t * t)
                            wgt = wgt * np.where(hit, wz, F(1))
                            counts["z0"] += int((take & hit & (wz == 0)).sum())
                            counts["z01"] += int((take & hit & (wz > 0) & (wz < 1)).sum())
                        if stop_l:
                            yq, _ = shifted(y, dy * s, dx * s)
                            x = np.abs(y - yq) / denom
                            t = np.fmax(F(0), F(1) - x)
                            wl = f32(t * t)
                            wgt = wgt * wl
                            counts["l0"] += int((take & (wl == 0)).sum())
                            counts["l01"] += int((take & (wl > 0) & (wl < 1)).sum())
                    f32(wgt)
                    take = take & (wgt != 0)                     # a tap of weight 0 adds nothing (a NaN weight is added)
                    acc = np.where(take[..., None], acc + wgt[..., None] * cq, acc)
                    acc_v = np.where(take, acc_v + (wgt * wgt) * vq, acc_v)
                    sum_w = np.where(take, sum_w + wgt, sum_w)
                    f32(acc, acc_v, sum_w)
            c, v = f32(acc / sum_w[..., None]), f32(acc_v / (sum_w * sum_w))
    if stats is not None:
        stats.update(counts)
    return c, v


def shares(stats):
    t = max(stats["taps"], 1)
    out = {k: stats[k] / t for k in ("n0", "n01", "z0", "z01", "l0", "l01", "mismatch")}
    out["last_outside"] = stats["last_outside"] / max(stats["last_taps"], 1)
    return out


def assert_input_condition(stats):
    s = shares(stats)
    print("shares of the in-image non-centre taps:", {k: "%.1f %%" % (100 * x) for k, x in s.items()})
    for k, x in s.items():
        assert x >= 0.05, (k, s)


# ---- synthetic inputs -----------------------------------------------------------------------------------------------------------
def make_inputs(width, height, comps, seed=11):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    region = (xx // 4 + yy // 3) % 3                                # three interleaved regions
    coverage = np.where(((xx + 2 * yy) // 3) % 4 == 0, 0, 4).astype(F)      # 0 on diagonal bands; else 4 samples hit
    axes = np.array([[1, 0.1, 0.2], [0.1, 1, 0.3], [0.6, 0.7, 0.4]], F)    # the first two nearly perpendicular, the third between them
    normal = (axes[region] + rng.normal(0, 0.04, (height, width, 3)).astype(F)) * coverage[..., None]      # a SUM over the hits
    dist = (F(5) + F(0.05) * xx.astype(F) + F(0.02) * yy.astype(F) + F(3) * ((xx // 5 + yy // 4) % 2).astype(F))
    distance = (dist * coverage).astype(F)
    base = (F(0.2) + F(0.8) * rng.random((3, comps)).astype(F))[region]
    sigma = np.array([0.02, 0.05, 0.1], F)[region]
    color = (base + sigma[..., None] * rng.normal(0, 1, (height, width, comps)).astype(F)).astype(F)
    weights = luminance(np.eye(comps, dtype=F)).astype(np.float64)  # Y is linear: the luminance of iid noise has variance sigma^2 sum w^2
    variance = (sigma.astype(np.float64) ** 2 * float((weights ** 2).sum())).astype(F)
    return dict(color=color, variance=variance, normal=normal.astype(F), distance=distance, coverage=coverage)


PARAMS = dict(sigma_luminance=SIGMA_L, sigma_distance=SIGMA_D, normal_power_log2=POWER)
SHAPES = [(37, 21), (1, 1), (70, 3), (3, 70), (130, 66)]
_cases = {}


def case(width, height, comps, iterations):
    """The inputs and the restated result of one case, computed once and shared (never modified)."""
    key = (width, height, comps, iterations)
    if key not in _cases:
        inputs, stats = make_inputs(width, height, comps), {}
        want = restate(iterations=iterations, stats=stats, **inputs, **PARAMS)
        for a in list(inputs.values()) + list(want):
            a.setflags(write=False)
        _cases[key] = dict(inputs=inputs, want=want, stats=stats)
    return _cases[key]


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("slrhip_denoise", "slrhip_denoise_scratch_bytes")


def test_library_exports_the_denoise_symbols():
    lib = binding.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in binding.EXPORTS
    assert lib.slrhip_version() == 7
    d = abi.DenoiseDesc()
    assert lib.slrhip_denoise(None, C.byref(d), None) == 1 and lib.slrhip_denoise(None, None, None) == 1      # no GPU needed to refuse


def header_struct(name):
    """[(type, field)] of `typedef struct <name> { ... }` in include/slrhip.h, comments stripped."""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slrhip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        m = re.match(r"(const float\*|float\*|uint32_t|float)\s+(.*)", decl.strip(), re.S)
        if m:
            fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return fields


def test_struct_layout_equals_the_header():
    """The header's fields under the C layout rules of the target (LP64: 8-byte pointers aligned to 8, 4-byte scalars)."""
    size = {"uint32_t": 4, "float": 4, "const float*": 8, "float*": 8}
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float, "const float*": C.c_void_p, "float*": C.c_void_p}
    fields = header_struct("slrhip_denoise_desc")
    assert [n for _, n in fields] == [n for n, _ in abi.DenoiseDesc._fields_]
    offset = 0
    for (t, n), (_, ct) in zip(fields, abi.DenoiseDesc._fields_):
        offset = (offset + size[t] - 1) // size[t] * size[t]
        assert ct is ctype[t], n
        assert getattr(abi.DenoiseDesc, n).offset == offset, n
        offset += size[t]
    assert C.sizeof(abi.DenoiseDesc) == (offset + 7) // 8 * 8 == 88


def test_scratch_size():
    lib = binding.load_library()
    size = lib.slrhip_denoise_scratch_bytes
    for w, h, c in ((0, 4, 3), (4, 0, 3), (4, 4, 0), (4, 4, 4), (4, 4, 15), (4, 4, 17), (65536, 32768, 3), (1 << 31, 1, 3), (0xFFFFFFFF, 0xFFFFFFFF, 16)):
        assert size(w, h, c) == 0, (w, h, c)
    # the documented formula: a 16-byte guide record, two 8-byte {Y, v} records and two colour records (16 or 64 bytes) per pixel
    for w, h in ((1, 1), (37, 21), (130, 66), (1280, 720), (65535, 32768), (1, (1 << 31) - 1)):
        assert size(w, h, 3) == w * h * (32 + 2 * 16) and size(w, h, 16) == w * h * (32 + 2 * 64)
    # monotone in each argument
    for a, b in ((36, 37), (1, 2), (1279, 1280)):
        for c in (3, 16):
            assert size(a, 21, c) < size(b, 21, c) and size(21, a, c) < size(21, b, c)
        assert size(a, b, 3) < size(a, b, 16)


def test_host_program_parses_the_denoise_flag(capsys):
    ap = host.build_parser()
    assert ap.parse_args(["scene.txt"]).denoise is None
    assert ap.parse_args(["scene.txt", "--denoise"]).denoise == 5
    assert ap.parse_args(["scene.txt", "--denoise", "3", "--samples", "8"]).denoise == 3
    a = ap.parse_args(["--denoise", "2", "scene.txt", "--adaptive", "0.25"])
    assert (a.denoise, a.adaptive, a.scene) == (2, 0.25, "scene.txt")
    for bad in (["--denoise", "0"], ["--denoise", "9"], ["--denoise", "-1"], ["--denoise", "x"]):
        with pytest.raises(SystemExit):                            # refused before the scene is read
            host.main(["scene.txt"] + bad)
    capsys.readouterr()


@pytest.mark.parametrize("comps", [3, 16])
def test_restatement_keeps_a_constant_image_constant(comps):
    """c' = (sum w k) / (sum w) with one value k per component.  In float32 that is k for every k only if the sums are exact; with k
    a power of two, w * k is exact and the sum of the w * k rounds exactly as the sum of the w does, so the quotient is k to the
    last bit, for any guides and any weights."""
    inputs = dict(make_inputs(37, 21, comps))
    k = np.array([2.0 ** (e % 5 - 2) for e in range(comps)], F)
    inputs["color"] = np.broadcast_to(k, (21, 37, comps)).copy()
    for kw in (PARAMS, dict(PARAMS, sigma_luminance=0.0), dict(PARAMS, sigma_distance=0.0, normal_power_log2=0)):
        out, _ = restate(iterations=5, **inputs, **kw)
        assert_bit_equal(out, inputs["color"], "constant image")
    out, _ = restate(inputs["color"], iterations=3)
    assert_bit_equal(out, inputs["color"], "constant image, no guides")


def test_restatement_with_every_stop_off_is_the_b3_convolution():
    inputs = make_inputs(37, 21, 3)
    color = inputs["color"]
    out, var = restate(color, iterations=1)                          # no guide at all
    flat = dict(inputs, coverage=np.full((21, 37), 4, F), normal=np.broadcast_to(np.array([0, 0, 4], F), (21, 37, 3)).copy())
    out2, _ = restate(iterations=1, **flat, sigma_luminance=0.0, sigma_distance=0.0, normal_power_log2=7)
    k = np.outer(H5, H5).astype(np.float64)
    for (y, x) in ((2, 2), (10, 17), (18, 34)):                      # interior: all 25 taps inside, sum of the weights exactly 1
        want = sum(k[dy + 2, dx + 2] * color[y + dy, x + dx].astype(np.float64) for dy in range(-2, 3) for dx in range(-2, 3))
        np.testing.assert_allclose(out[y, x], want, rtol=2e-6)
        assert var[y, x] == 0
    # every pixel a hit with the normal (0, 0, 1) (n.n' = 1 exactly), both sigmas 0: the same weights, so the same bits
    assert_bit_equal(out2, out, "every stop off vs no guide")


def test_input_condition_of_the_synthetic_case():
    for comps in (3, 16):
        assert_input_condition(case(37, 21, comps, 5)["stats"])


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def assert_result(got, want, what):
    assert_bit_equal(got[0], want[0], what + ": output")
    assert_bit_equal(got[1], want[1], what + ": output_variance")


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 5])
@pytest.mark.parametrize("comps", [3, 16])
@pytest.mark.parametrize("width, height", SHAPES)
def test_bit_exact(ctx, width, height, comps, iterations):
    k = case(width, height, comps, iterations)
    if (width, height, iterations) == (37, 21, 5):
        assert_input_condition(k["stats"])
    else:
        print("shares (not asserted for this shape):", shares(k["stats"]))
    assert np.isfinite(k["want"][0]).all()
    got = ctx.denoise(iterations=iterations, want_variance=True, **k["inputs"], **PARAMS)
    assert_result(got, k["want"], "%d x %d x %d, %d iterations" % (width, height, comps, iterations))
    assert_bit_equal(ctx.denoise(iterations=iterations, **k["inputs"], **PARAMS), k["want"][0], "without output_variance")


@pytest.mark.gpu
def test_switches(ctx):
    """Every combination of absent guides that the call accepts, and non-positive sigmas, takes the path the definition says."""
    inputs = case(37, 21, 3, 2)["inputs"]
    seen = set()
    for mask in range(16):
        use = {name: bool(mask >> b & 1) for b, name in enumerate(("variance", "normal", "distance", "coverage"))}
        if (use["normal"] or use["distance"]) and not use["coverage"]:
            continue                                               # refused: test_argument_errors
        given = dict(color=inputs["color"], **{k: inputs[k] for k in use if use[k]})
        for sl, sd in ((SIGMA_L, SIGMA_D),) if mask != 15 else ((SIGMA_L, SIGMA_D), (0.0, SIGMA_D), (-1.0, SIGMA_D), (SIGMA_L, 0.0), (SIGMA_L, -2.0), (0.0, 0.0),
                                                              (float("inf"), float("inf"))):
            kw = dict(iterations=2, sigma_luminance=sl, sigma_distance=sd, normal_power_log2=3)
            want = restate(**given, **kw)
            seen.add(want[0].tobytes())
            assert_result(ctx.denoise(want_variance=True, **given, **kw), want, "guides %r, sigmas %r" % (use, (sl, sd)))
    assert len(seen) >= 10, "the switches do not change the result: the input does not tell them apart"
    for power in (0, 1, 7):
        kw = dict(PARAMS, iterations=2, normal_power_log2=power)
        assert_result(ctx.denoise(want_variance=True, **inputs, **kw), restate(**inputs, **kw), "normal_power_log2 %d" % power)


def assert_same_with_nan(got, want, what):
    for g, w in zip(got, want):
        assert np.array_equal(np.isnan(g), np.isnan(w)), what + ": NaN masks differ"
        assert_bit_equal(np.where(np.isnan(g), F(0), g), np.where(np.isnan(w), F(0), w), what)


@pytest.mark.gpu
@pytest.mark.parametrize("comps", [3, 16])
def test_non_finite_pixels(ctx, comps):
    k = case(37, 21, comps, 5)
    inputs = dict(k["inputs"])
    color = inputs["color"].copy()
    assert inputs["coverage"][9, 17] > 0 and inputs["coverage"][14, 30] > 0 and inputs["coverage"][4, 5] == 0
    color[9, 17, 1], color[14, 30, 0], color[4, 5, 2] = np.nan, np.inf, np.nan          # two hit pixels and a miss pixel
    inputs["color"] = color
    planted = np.zeros((21, 37), bool)
    planted[9, 17] = planted[14, 30] = planted[4, 5] = True
    # the luminance stop on: each stays in its own pixel
    want = restate(iterations=5, **inputs, **PARAMS)
    assert np.array_equal(~np.isfinite(want[0]).all(axis=2), planted) and np.isfinite(want[1]).all()
    assert np.isnan(want[0][9, 17, 1]) and np.isinf(want[0][14, 30, 0])
    got = ctx.denoise(iterations=5, want_variance=True, **inputs, **PARAMS)
    assert_same_with_nan(got, want, "luminance stop on")
    # off: they spread to every pixel of their hit class that the taps connect them to
    kw = dict(PARAMS, sigma_luminance=0.0, iterations=3)
    want = restate(**inputs, **kw)
    spread = ~np.isfinite(want[0]).all(axis=2)
    assert spread.sum() >= 20 and not spread.all()
    assert_same_with_nan(ctx.denoise(want_variance=True, **inputs, **kw), want, "luminance stop off")


@pytest.mark.gpu
def test_argument_errors(ctx):
    w, h, comps = 37, 21, 3
    k = case(w, h, comps, 2)
    inputs = k["inputs"]
    with binding.DeviceBlocks() as dev:
        p = {name: dev.put(a) for name, a in inputs.items()}
        sentinel = F(-7.5)
        out, out_v = dev.put(np.full((h, w, comps), sentinel)), dev.put(np.full((h, w), sentinel))
        big = dev.put(np.full((2 * h * w * comps,), sentinel))               # room for overlapping ranges

        def desc(**over):
            f = dict(width=w, height=h, components=comps, iterations=2, color=p["color"], variance=p["variance"], normal=p["normal"],
                     distance=p["distance"], coverage=p["coverage"], output=out, output_variance=out_v, sigma_luminance=SIGMA_L,
                     sigma_distance=SIGMA_D, normal_power_log2=POWER, reserved=0)
            f.update(over)
            return abi.DenoiseDesc(**f)
        lib = ctx.lib
        nan = float("nan")
        frame = 4 * h * w * comps
        bad = [dict(color=None), dict(output=None), dict(color=p["color"] + 2), dict(output=out + 1), dict(variance=p["variance"] + 2),
               dict(output_variance=out_v + 2), dict(components=4), dict(components=0), dict(iterations=0), dict(iterations=9),
               dict(normal_power_log2=8), dict(reserved=1), dict(sigma_luminance=nan), dict(sigma_distance=nan), dict(width=0), dict(height=0),
               dict(width=65536, height=32768), dict(coverage=None), dict(coverage=None, normal=None), dict(coverage=None, distance=None),
               dict(output=p["color"]), dict(output=p["color"] + frame - 4), dict(output_variance=p["color"] + 4),
               dict(output=big, output_variance=big + frame - 4), dict(output=big + 4, output_variance=big),
               dict(output=p["normal"] - 4), dict(output=p["normal"]),
               dict(output_variance=p["coverage"]), dict(output_variance=p["variance"] + 4 * (h * w - 1)), dict(output_variance=p["distance"])]
        for over in bad:
            d = desc(**over)
            assert lib.slrhip_denoise(ctx.handle, C.byref(d), None) == 1, over
            assert b"slrhip_denoise" in lib.slrhip_last_error_string()
        assert lib.slrhip_denoise(ctx.handle, None, None) == 1
        ctx.synchronize()
        for ptr, shape in ((out, (h, w, comps)), (out_v, (h, w)), (big, (2 * h * w * comps,))):
            assert (dev.get(ptr, shape) == sentinel).all(), "a refused call wrote"
        for name, a in inputs.items():
            assert_bit_equal(dev.get(p[name], a.shape), a, "input %s after the refused calls" % name)
        # adjacent ranges do not overlap: output directly behind output_variance
        d = desc(output=big + 4 * h * w, output_variance=big)
        assert lib.slrhip_denoise(ctx.handle, C.byref(d), None) == 0
        ctx.synchronize()
        assert_result((dev.get(big + 4 * h * w, (h, w, comps)), dev.get(big, (h, w))), k["want"], "adjacent outputs")
        # the good descriptor works after all the refusals
        d = desc()
        assert lib.slrhip_denoise(ctx.handle, C.byref(d), None) == 0
        ctx.synchronize()
        assert_result((dev.get(out, (h, w, comps)), dev.get(out_v, (h, w))), k["want"], "after the refused calls")


@pytest.mark.gpu
def test_scratch_is_reused_by_a_smaller_call():
    """A fresh context: the first call allocates for 130 x 66 x 16; 37 x 21 x 3 then fits the scratch it finds, 130 x 66 x 16
    again as well."""
    fresh = Context()
    try:
        for width, height, comps in ((130, 66, 16), (37, 21, 3), (1, 1, 16), (130, 66, 16)):
            k = case(width, height, comps, 5)
            got = fresh.denoise(iterations=5, want_variance=True, **k["inputs"], **PARAMS)
            assert_result(got, k["want"], "%d x %d x %d on a reused scratch" % (width, height, comps))
    finally:
        fresh.close()


def cornell(mode=abi.MODE_RGB):
    c = Context(mode=mode)
    c.upload_scene(scenes.cornell_box_spheres(1.0, 16, 8, "matte"))
    return c


@pytest.mark.gpu
def test_render_is_independent_of_a_denoise_call_in_between():
    st = ob.settings(32, 24, seed=5)
    k = case(37, 21, 3, 5)
    c = cornell()
    try:
        c.render_begin(st)
        c.render(0, 4)
        want = c.read_framebuffer()
        c.render_begin(st)
        c.render(0, 2)
        got = c.denoise(iterations=5, want_variance=True, **k["inputs"], **PARAMS)          # an unrelated buffer
        c.render(2, 2)
        assert_bit_equal(c.read_framebuffer(), want, "render 2 + denoise + render 2 vs render 4")
        assert np.array_equal(c.read_framebuffer().view(np.uint32), want.view(np.uint32))
        assert_result(got, k["want"], "the denoise call in between")
        assert c.counters().samples == 4 * 32 * 24
    finally:
        c.close()


GUIDES = abi.FEATURE_SHADING_NORMAL | abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE


def render_with_guides(c, st, spp):
    c.render_begin(st)
    c.statistics_begin()
    c.render(0, spp)
    c.render_features(GUIDES, spp)
    return dict(color=c.read_framebuffer_mean(), variance=c.statistics(abi.STATISTICS_VARIANCE_OF_MEAN),
                normal=c.features(abi.FEATURE_SHADING_NORMAL), distance=c.features(abi.FEATURE_DISTANCE), coverage=c.features(abi.FEATURE_COVERAGE))


@pytest.fixture(scope="module")
def cornell_case():
    st = ob.settings(64, 48, seed=5)
    c = cornell()
    inputs = render_with_guides(c, st, 8)
    yield dict(ctx=c, settings=st, inputs=inputs, denoised=c.denoised(want_variance=True))
    c.close()


@pytest.mark.gpu
def test_denoised_equals_the_restatement_on_the_read_outs(cornell_case):
    """Context.denoised() resolves the five buffers on the device; the restatement takes the same five through the read-outs."""
    inputs = cornell_case["inputs"]
    assert (inputs["coverage"] > 0).any() and (inputs["variance"] > 0).mean() > 0.5
    params = dict(iterations=5, sigma_luminance=4.0, sigma_distance=abi.DENOISE_SIGMA_DISTANCE, normal_power_log2=7)
    want = restate(**inputs, **params)
    assert_result(cornell_case["denoised"], want, "Context.denoised() vs the restatement")
    assert_bit_equal(cornell_case["ctx"].denoise(**inputs), want[0], "Context.denoise() with its defaults")
    c = cornell_case["ctx"]
    c.render_begin(cornell_case["settings"], (1, 3))
    with pytest.raises(binding.SlrHipError, match="whole image"):
        c.denoised()


@pytest.mark.gpu
def test_denoised_frame_is_closer_to_the_converged_one(cornell_case):
    """The purpose of the filter: the RMS luminance difference to a 1024-spp render of the same context is strictly smaller for the
    denoised 8-spp frame than for the raw 8-spp mean frame, with the defaults of Context.denoised().  Measured on MI355X
    (cornell_box_spheres(1.0, 16, 8, "matte"), 64 x 48, seed 5): raw 8 spp 0.00127945, denoised 0.00113794."""
    c, st = cornell_case["ctx"], cornell_case["settings"]
    c.render_begin(st)
    c.render(0, 1024)
    converged = luminance(c.read_framebuffer()).astype(np.float64) / 1024.0

    def rms(frame):
        return float(np.sqrt(np.mean((luminance(frame).astype(np.float64) - converged) ** 2)))
    raw, den = rms(cornell_case["inputs"]["color"]), rms(cornell_case["denoised"][0])
    print("RMS luminance difference to 1024 spp: raw 8 spp %.6g, denoised 8 spp %.6g" % (raw, den))
    assert den < raw, (den, raw)


@pytest.mark.gpu
def test_spectral_context_end_to_end():
    """16 components through Context.denoised(): the mean resolve of a spectral frame feeds the filter's four float4s per pixel."""
    st = ob.settings(32, 24, seed=5)
    c = cornell(abi.MODE_SPECTRAL)
    try:
        inputs = render_with_guides(c, st, 4)
        assert inputs["color"].shape == (24, 32, 16)
        got = c.denoised(want_variance=True, iterations=3)
        want = restate(iterations=3, sigma_luminance=4.0, sigma_distance=abi.DENOISE_SIGMA_DISTANCE, normal_power_log2=7, **inputs)
        assert_result(got, want, "spectral Context.denoised()")
    finally:
        c.close()


@pytest.mark.gpu
def test_host_program_writes_the_denoised_image(tmp_path, capsys):
    """python -m slr_amd.host --denoise: the ordinary images are the ones of a run without the flag, byte for byte, and
    <name>_denoised.bmp appears next to the last of them; with --features the guides ride with the channels asked for."""
    from test_scene_language import cornell_script
    script = tmp_path / "box.txt"
    script.write_text(cornell_script("matte").replace('"width": 320, "height": 240', '"width": 48, "height": 36'))
    plain, with_flag = tmp_path / "plain", tmp_path / "denoise"
    plain.mkdir()
    with_flag.mkdir()
    assert host.main([str(script), "--samples", "4", "--out", str(plain)]) == 0
    assert host.main([str(script), "--samples", "4", "--out", str(with_flag), "--denoise", "3", "--features", str(with_flag)]) == 0
    assert "denoised (3 iterations): 002_denoised.bmp" in capsys.readouterr().out
    for name in ("000.bmp", "001.bmp", "002.bmp"):
        assert (plain / name).read_bytes() == (with_flag / name).read_bytes(), name
    assert not (plain / "002_denoised.bmp").exists()
    raw, den = (with_flag / "002.bmp").read_bytes(), (with_flag / "002_denoised.bmp").read_bytes()
    assert len(raw) == len(den) and raw[:54] == den[:54] and raw != den
    saved = np.load(str(with_flag / "features.npz"))
    assert {"shading_normal", "distance", "coverage", "geometric_normal"} <= set(saved.files)
