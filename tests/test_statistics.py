"""Per-pixel noise statistics (slrhip_statistics_begin / slrhip_resolve_statistics / slrhip_statistics_summary) and rendering to
a noise target (slrhip_render_until).

Expected values come from PER-PASS FRAMES — render_begin; render(p, 1); read_framebuffer: the path without statistics, where the
sensor's Kahan sum of one value from zero is that value — and a numpy float32 restatement, written here, of the sample luminance
and of the Welford update the fold kernel applies in pass order.  Everything is compared bit for bit; the only tolerance is that
of the summary's three double sums against numpy's float64 sums of the same float32 values, which differ in the ORDER of at most
2^20 non-negative additions: relative 2^20 x 2^-53 = 1.2e-10 at worst, bound used 1e-9."""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import assert_bit_equal, summary_double_sum
from oracle import binding as ob
from slr_amd import Context, abi, binding, host, scenes, spectra
from test_cabi import render_plan

F = np.float32
CHANNELS = (abi.STATISTICS_MEAN, abi.STATISTICS_VARIANCE, abi.STATISTICS_VARIANCE_OF_MEAN, abi.STATISTICS_COUNT, abi.STATISTICS_MAX)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def cmf16():
    """(ybar[16], integralCMF) of the 16-bin storage spectrum, as dumped from the compiled reference (slr_amd/data)."""
    t = np.asarray(spectra.tables()["cmf16"], F)
    return t[16:32].copy(), F(t[48])


def luminance(v):
    """Y of samples [..., 3] or [..., 16] (float32), as include/slrhip.h states it."""
    v = np.asarray(v, F)
    if v.shape[-1] == 3:
        d = v.astype(np.float64)
        return ((0.222485 * d[..., 0] + 0.716905 * d[..., 1]) + 0.060610 * d[..., 2]).astype(F)
    w, integral = cmf16()
    p = []
    for q in range(4):
        a = ((w[4 * q] * v[..., 4 * q] + w[4 * q + 1] * v[..., 4 * q + 1]) + w[4 * q + 2] * v[..., 4 * q + 2]) + w[4 * q + 3] * v[..., 4 * q + 3]
        assert a.dtype == F
        p.append(a)
    return ((p[0] + p[1]) + (p[2] + p[3])) / integral


def welford(frames):
    """The five channels after the per-pass frames [passes][H][W][C], float32 steps in pass order."""
    shape = frames[0].shape[:2] if len(frames) else None
    mean = m2 = mx = None
    n = 0
    with np.errstate(all="ignore"):
        for fr in frames:
            y = luminance(fr)
            if mean is None:
                mean, m2, mx = np.zeros(shape, F), np.zeros(shape, F), np.zeros(shape, F)
            n += 1
            d = y - mean
            mean = mean + d / F(n)
            m2 = m2 + d * (y - mean)
            mx = np.fmax(mx, y)
            assert mean.dtype == F and m2.dtype == F
    zero = np.zeros_like(mean)
    return {abi.STATISTICS_MEAN: mean, abi.STATISTICS_VARIANCE: m2 / F(n - 1) if n >= 2 else zero,
            abi.STATISTICS_VARIANCE_OF_MEAN: m2 / (F(n - 1) * F(n)) if n >= 2 else zero,
            abi.STATISTICS_COUNT: np.full_like(mean, F(n)), abi.STATISTICS_MAX: mx}


def assert_same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, what
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), "%s: %d of %d floats differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


# ---- GPU helpers ----------------------------------------------------------------------------------------------------------------
def per_pass_frames(ctx, st, passes):
    out = []
    for p in range(passes):
        ctx.render_begin(st)
        ctx.render(p, 1)
        out.append(ctx.read_framebuffer())
    return out


def channels_of(ctx):
    return {c: ctx.statistics(c) for c in CHANNELS}


def render_with_statistics(ctx, st, calls, shard=(0, 1)):
    ctx.render_begin(st, shard)
    ctx.statistics_begin()
    for begin, count in calls:
        ctx.render(begin, count)
    return channels_of(ctx)


def make_case(mode, material, width, height, passes):
    sc = scenes.cornell_box_spheres(1.0, 16, 8, material)
    st = ob.settings(width, height, seed=5)
    ctx = Context(mode=mode)
    ctx.upload_scene(sc)
    frames = per_pass_frames(ctx, st, passes)
    got = render_with_statistics(ctx, st, [(0, passes)])
    return dict(scene=sc, settings=st, ctx=ctx, frames=frames, got=got, passes=passes)


@pytest.fixture(scope="module")
def rgb_case():
    case = make_case(abi.MODE_RGB, "matte", 64, 48, 7)
    yield case
    case["ctx"].close()


@pytest.fixture(scope="module")
def spectral_case():
    case = make_case(abi.MODE_SPECTRAL, "glass", 32, 24, 5)
    yield case
    case["ctx"].close()


# ---- 1, 2: bit-exact moments ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_moments_rgb_bit_exact(rgb_case):
    """7 passes: one trip of the four-entry loop and three of the remainder."""
    want = welford(rgb_case["frames"])
    assert float(want[abi.STATISTICS_VARIANCE].max()) > 0
    for c in CHANNELS:
        assert_same_bits(rgb_case["got"][c], want[c], abi.STATISTICS_CHANNELS[c])


@pytest.mark.gpu
def test_moments_rgb_from_oracle_frames(rgb_case, oracle_rgb):
    """The same with the per-pass frames of the CPU oracle.  That they equal the GPU's per-pass frames is the existing parity of
    the render path, asserted first so that a failure names its cause."""
    osc = oracle_rgb.scene(rgb_case["scene"])
    frames = [osc.render(rgb_case["settings"], 1, spp_begin=p)[0].astype(F) for p in range(rgb_case["passes"])]
    for p, (a, b) in enumerate(zip(frames, rgb_case["frames"])):
        assert_bit_equal(a, b, "existing parity: oracle vs GPU frame of pass %d" % p)
    want = welford(frames)
    for c in (abi.STATISTICS_VARIANCE, abi.STATISTICS_VARIANCE_OF_MEAN, abi.STATISTICS_COUNT):
        assert_same_bits(rgb_case["got"][c], want[c], abi.STATISTICS_CHANNELS[c])
    for c in (abi.STATISTICS_MEAN, abi.STATISTICS_MAX):          # a -0 sample of the oracle is a +0 one here: the same luminance
        assert_bit_equal(rgb_case["got"][c], want[c], abi.STATISTICS_CHANNELS[c])


@pytest.mark.gpu
def test_moments_spectral_bit_exact(spectral_case):
    """Four lanes per pixel: the quad exchange and the order of the bin sum.  5 passes: the four-entry loop and the remainder."""
    want = welford(spectral_case["frames"])
    assert float(want[abi.STATISTICS_VARIANCE].max()) > 0
    for c in CHANNELS:
        assert_same_bits(spectral_case["got"][c], want[c], abi.STATISTICS_CHANNELS[c])


# ---- 3: split independence ------------------------------------------------------------------------------------------------------
def summary_matches(summary, ch, pixels, passes):
    assert summary["pixels"] == pixels and summary["samples"] == pixels * passes
    assert F(summary["max_sample"]) == ch[abi.STATISTICS_MAX].max()
    mean = ch[abi.STATISTICS_MEAN].astype(np.float64)
    for name, want in (("sum_mean", mean.sum()), ("sum_mean_sq", (mean * mean).sum()),
                       ("sum_variance_of_mean", ch[abi.STATISTICS_VARIANCE_OF_MEAN].astype(np.float64).sum())):
        print("summary %s: %r, numpy %r" % (name, summary[name], want))
        assert want > 0 and abs(summary[name] - want) <= 1e-9 * want, name


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_statistics_do_not_depend_on_how_the_passes_are_cut(mode):
    sc = scenes.cornell_box_spheres(1.0, 24, 12, "glass")
    st = ob.settings(64, 64, seed=5)
    amode = abi.MODE_RGB if mode == "rgb" else abi.MODE_SPECTRAL
    ctx = Context(mode=amode, stripes=1)
    ctx.upload_scene(sc)
    seven = render_with_statistics(ctx, st, [(0, 7)])
    cut = render_with_statistics(ctx, st, [(0, 3), (3, 4)])
    for c in CHANNELS:
        assert_same_bits(cut[c], seven[c], "render(0,3) + render(3,4) vs render(0,7): " + abi.STATISTICS_CHANNELS[c])
    whole = render_with_statistics(ctx, st, [(0, 32)])
    first = ctx.statistics_summary()
    assert first == ctx.statistics_summary(), "two summary calls on the same state"
    summary_matches(first, whole, 64 * 64, 32)
    two = render_with_statistics(ctx, st, [(0, 13), (13, 19)])
    os.environ["SLRHIP_RESULT_WINDOW_MB"] = "1"           # 64 x 64 pixels x 16 B (64 B spectral) per pass: windows of 16 (4) passes
    try:
        windows = render_with_statistics(ctx, st, [(0, 32)])
    finally:
        del os.environ["SLRHIP_RESULT_WINDOW_MB"]
    parts = [render_with_statistics(ctx, st, [(0, 32)], shard=(i, 2)) for i in range(2)]
    part_summaries = []
    for i in range(2):
        ctx.render_begin(st, (i, 2))
        ctx.statistics_begin()
        ctx.render(0, 32)
        part_summaries.append(ctx.statistics_summary())
    ctx.close()
    auto = Context(mode=amode, stripes=0)
    auto.upload_scene(sc)
    stripes = render_with_statistics(auto, st, [(0, 32)])
    auto.close()
    for c in CHANNELS:
        name = abi.STATISTICS_CHANNELS[c]
        assert_same_bits(two[c], whole[c], "two render calls vs one: " + name)
        assert_same_bits(windows[c], whole[c], "result windows of 1 MiB vs one window: " + name)
        assert_same_bits(stripes[c], whole[c], "automatic slot count vs stripes = 1: " + name)
        assert ((parts[0][c] == 0) | (parts[1][c] == 0)).all()
        assert_same_bits(parts[0][c] + parts[1][c], whole[c], "two shards added vs the whole frame: " + name)
    assert part_summaries[0]["pixels"] + part_summaries[1]["pixels"] == 64 * 64
    assert part_summaries[0]["samples"] + part_summaries[1]["samples"] == 64 * 64 * 32
    assert max(part_summaries[0]["max_sample"], part_summaries[1]["max_sample"]) == first["max_sample"]
    for name in ("sum_mean", "sum_mean_sq", "sum_variance_of_mean"):
        assert abs(part_summaries[0][name] + part_summaries[1][name] - first[name]) <= 1e-9 * first[name], name


@pytest.mark.gpu
def test_summary_sums_in_the_fixed_order_over_two_blocks():
    """67 x 63 = 4221 pixels: one full block of the summary's first stage and a second one of 125 pixels (less than a row of 256
    threads, less than two waves), so the block loop, the guard past the last pixel and the partial wave all run.  The three double
    sums equal, bit for bit, the restatement of their fixed order (helpers.summary_double_sum) over the float32 channels in
    pixel-list order; the products mean x mean are exact in double."""
    width, height, passes = 67, 63, 3
    st = ob.settings(width, height, seed=5)
    ctx = Context(mode=abi.MODE_RGB)
    ctx.upload_scene(scenes.cornell_box_spheres(1.0, 16, 8, "matte"))
    ch = render_with_statistics(ctx, st, [(0, passes)])
    got = ctx.statistics_summary()
    xy = render_plan(ctx.lib, width, height, (0, 1), 0, abi.MODE_RGB, want_pixels=True)[2]
    ctx.close()
    assert xy.size == width * height == 4221 and 4096 < xy.size < 4096 + 128
    x, y = xy & 0xFFFF, xy >> 16
    mean = ch[abi.STATISTICS_MEAN][y, x].astype(np.float64)
    want = dict(pixels=xy.size, samples=xy.size * passes, sum_mean=summary_double_sum(mean), sum_mean_sq=summary_double_sum(mean * mean),
                sum_variance_of_mean=summary_double_sum(ch[abi.STATISTICS_VARIANCE_OF_MEAN][y, x].astype(np.float64)),
                max_sample=float(ch[abi.STATISTICS_MAX].max()))
    print("summary %r, restated %r" % (got, want))
    assert want["sum_mean"] > 0 and want["sum_variance_of_mean"] > 0
    for name in ("pixels", "samples", "max_sample", "sum_mean", "sum_mean_sq", "sum_variance_of_mean"):
        assert got[name] == want[name], name


# ---- 4: edge counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_pass_and_no_pass(rgb_case):
    ctx, st = rgb_case["ctx"], rgb_case["settings"]
    one = render_with_statistics(ctx, st, [(0, 1)])
    assert not one[abi.STATISTICS_VARIANCE].any() and not one[abi.STATISTICS_VARIANCE_OF_MEAN].any()
    assert (one[abi.STATISTICS_COUNT] == 1).all()
    y = luminance(rgb_case["frames"][0])
    assert y.max() > 0
    assert_same_bits(one[abi.STATISTICS_MEAN], y, "mean of one sample")
    assert_same_bits(one[abi.STATISTICS_MAX], np.fmax(F(0), y), "max of one sample")
    for calls in ([], [(0, 0)]):                          # no render call at all; a call of zero passes
        none = render_with_statistics(ctx, st, calls)
        for c in CHANNELS:
            assert not none[c].view(np.uint32).any(), abi.STATISTICS_CHANNELS[c]
        s = ctx.statistics_summary()
        assert s == dict(pixels=64 * 48, samples=0, sum_mean=0.0, sum_mean_sq=0.0, sum_variance_of_mean=0.0, max_sample=0.0)


# ---- 5: the frame is untouched --------------------------------------------------------------------------------------------------
def counters_of(ctx):
    c = ctx.counters()
    return (c.samples, c.extension_rays, c.shadow_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["rgb_case", "spectral_case"])
def test_statistics_leave_the_frame_alone(request, case_name):
    case = request.getfixturevalue(case_name)
    ctx, st, passes = case["ctx"], case["settings"], case["passes"]
    plain = Context(mode=ctx.mode)                        # a context that never enabled statistics
    plain.upload_scene(case["scene"])
    plain.render_begin(st)
    plain.render(0, passes)
    want, want_counters = plain.read_framebuffer(), counters_of(plain)
    plain.close()
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.render(0, passes)                                 # (a raised device error word would fail this call)
    assert_same_bits(ctx.read_framebuffer(), want, "frame with statistics on")
    assert counters_of(ctx) == want_counters
    ctx.render_begin(st)                                  # statistics are per render: off again
    with pytest.raises(binding.SlrHipError, match=r"\(1\).*statistics are off"):
        ctx.statistics(abi.STATISTICS_MEAN)
    with pytest.raises(binding.SlrHipError, match=r"\(1\).*statistics are off"):
        ctx.statistics_summary()
    ctx.render(0, passes)
    assert_same_bits(ctx.read_framebuffer(), want, "frame of the next render, statistics off")


# ---- 6: render_until ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("metric", [abi.NOISE_RMSE, abi.NOISE_RELATIVE])
def test_render_until_stops_at_the_block_that_reaches_the_target(rgb_case, metric):
    ctx, st = rgb_case["ctx"], rgb_case["settings"]
    step, spp_max = 4, 24
    # the metric after 4, 8, 12, ... passes, by plain render calls
    ctx.render_begin(st)
    ctx.statistics_begin()
    values, frames = [], {}
    for done in range(step, spp_max + 1, step):
        ctx.render(done - step, step)
        values.append(abi.noise_metric(ctx.statistics_summary(), metric))
        frames[done] = ctx.read_framebuffer()
    print("metric %d after %s passes: %r" % (metric, list(range(step, spp_max + 1, step)), values))
    assert np.isfinite(values).all() and min(values) > 0
    pairs = [1] + [k for k in range(len(values) - 1) if k != 1]           # the 8- and 12-pass values first, else the first decreasing pair
    k = next((k for k in pairs if values[k + 1] < values[k]), None)
    assert k is not None, "the metric never decreases from one block to the next"
    target = 0.5 * (values[k] + values[k + 1])
    assert values[k + 1] < F(target) < values[k]                           # (the ABI takes the target as float32)
    stop = next(i for i, v in enumerate(values) if v <= F(target))         # the first block at or under the target: k + 1 when the values fall
    assert stop <= k + 1

    def run(target, step, spp_max):
        ctx.render_begin(st)
        ctx.statistics_begin()
        done, last = ctx.render_until(metric, target, step, spp_max)
        assert last == ctx.statistics_summary(), "`last` is the summary of the state render_until left"
        return done, last, ctx.read_framebuffer()

    done, last, fb = run(target, step, spp_max)
    assert done == step * (stop + 1)
    assert abi.noise_metric(last, metric) == values[stop]
    assert_same_bits(fb, frames[done], "render_until vs render(0, spp_done)")
    done, last, fb = run(0.0, step, spp_max)                                # never reached: the sample limit
    assert done == spp_max and last["samples"] == 64 * 48 * spp_max
    assert_same_bits(fb, frames[spp_max], "target 0")
    done, last, fb = run(0.0, 5, 22)                                        # a limit that is no multiple of the step: the last block is cut
    assert done == 22 and last["samples"] == 64 * 48 * 22
    ctx.render_begin(st)
    ctx.render(0, 22)
    assert_same_bits(fb, ctx.read_framebuffer(), "spp_max 22 in steps of 5 vs render(0, 22)")
    done, last, fb = run(float("inf"), step, spp_max)                       # reached at once
    assert done == step and last["samples"] == 64 * 48 * step
    assert_same_bits(fb, frames[step], "target infinity")
    done, last, fb = run(float("inf"), 1, spp_max)                          # ... but not before every pixel holds two samples
    assert done == 2


# ---- 7: argument errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(rgb_case):
    INVALID, NO_SCENE = r"\(1\)", r"\(4\)"
    fresh = Context()
    fresh.settings = rgb_case["settings"]
    for call in (fresh.statistics_begin, lambda: fresh.statistics(abi.STATISTICS_MEAN), fresh.statistics_summary,
                 lambda: fresh.statistics_into(abi.STATISTICS_MEAN, 16, 1 << 20), lambda: fresh.render_until(abi.NOISE_RMSE, 0.1, 4, 8)):
        with pytest.raises(binding.SlrHipError, match=NO_SCENE):          # before render_begin
            call()
    fresh.upload_scene(rgb_case["scene"])
    with pytest.raises(binding.SlrHipError, match=NO_SCENE):              # a scene, but still no render_begin
        fresh.statistics_begin()
    fresh.close()

    ctx, st = rgb_case["ctx"], rgb_case["settings"]
    ctx.render_begin(st)
    for call in (lambda: ctx.statistics(abi.STATISTICS_MEAN), ctx.statistics_summary, lambda: ctx.render_until(abi.NOISE_RMSE, 0.1, 4, 8),
                 lambda: ctx.statistics_into(abi.STATISTICS_MEAN, 16, 1 << 20)):
        with pytest.raises(binding.SlrHipError, match=INVALID + ".*statistics are off"):
            call()
    ctx.render(0, 3)
    before = ctx.read_framebuffer()
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*this render has begun"):
        ctx.statistics_begin()
    assert_same_bits(ctx.read_framebuffer(), before, "frame after the refused statistics_begin")
    ctx.render(3, 4)                                                       # the render goes on ...
    plain = Context()
    plain.upload_scene(rgb_case["scene"])
    plain.render_begin(st)
    plain.render(0, 7)
    assert_same_bits(ctx.read_framebuffer(), plain.read_framebuffer(), "... to the frame of an undisturbed render")
    plain.close()
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*statistics are off"):
        ctx.statistics(abi.STATISTICS_MEAN)

    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.statistics_begin()                                                 # twice before the first render: nothing new
    for channel in (0, 3, 32, abi.STATISTICS_ALL, 1 << 31):
        with pytest.raises(binding.SlrHipError, match=INVALID + ".*one SLRHIP_STATISTICS"):
            ctx.statistics(channel)
        with pytest.raises(binding.SlrHipError, match=INVALID + ".*one SLRHIP_STATISTICS"):
            ctx.statistics_into(channel, 16, 1 << 20)
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*null"):
        ctx.statistics_into(abi.STATISTICS_MEAN, None, 1 << 20)
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*too small"):
        ctx.statistics_into(abi.STATISTICS_MEAN, 16, 64 * 48 - 1)
    for args in ((abi.NOISE_RMSE, 0.1, 0, 8), (abi.NOISE_RMSE, 0.1, 4, 0), (2, 0.1, 4, 8), (abi.NOISE_RELATIVE, float("nan"), 4, 8)):
        with pytest.raises(binding.SlrHipError, match=INVALID):
            ctx.render_until(*args)
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*2\\^32"):
        ctx.render_until(abi.NOISE_RMSE, 0.1, 4, 8, spp_begin=0xFFFFFFFC)
    # none of the refusals began the render: statistics are still on and empty
    assert ctx.statistics_summary()["samples"] == 0
    done, _ = ctx.render_until(abi.NOISE_RMSE, 0.0, 4, 7)
    assert done == 7
    for c in CHANNELS:
        assert_same_bits(ctx.statistics(c), rgb_case["got"][c], abi.STATISTICS_CHANNELS[c])


# ---- 8: CPU ---------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("slrhip_statistics_begin", "slrhip_resolve_statistics", "slrhip_read_statistics", "slrhip_statistics_summary",
               "slrhip_render_until", "slrhip_sample_luminance")


def test_library_exports_the_statistics_symbols():
    lib = binding.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in binding.EXPORTS
    assert lib.slrhip_version() == 7
    assert C.sizeof(abi.StatisticsSummary) == 48 and abi.StatisticsSummary.max_sample.offset == 40
    assert C.sizeof(abi.NoiseTarget) == 16
    assert lib.slrhip_statistics_begin(None) == 1 and lib.slrhip_statistics_summary(None, None, None) == 1      # no GPU needed to refuse


def host_luminance(values):
    lib = binding.load_library()
    v = np.ascontiguousarray(values, F)
    return np.array([lib.slrhip_sample_luminance(v.shape[1], row.ctypes.data) for row in v], F)


@pytest.mark.parametrize("components", [3, 16])
def test_sample_luminance_equals_the_restatement(components):
    rng = np.random.default_rng(7 + components)
    v = rng.random((4096, components)).astype(F) * F(8)
    v[::7] *= F(1e-3)
    v[::11] *= F(1e4)
    v[5] = 0
    v[6, 0] = -v[6, 0]                                     # no clamp
    assert_same_bits(host_luminance(v), luminance(v), "slrhip_sample_luminance, %d components" % components)
    with np.errstate(all="ignore"):
        v[0, 1] = np.inf                                   # not filtered
        v[1, 2] = np.nan
        got = host_luminance(v[:2])
    assert np.isinf(got[0]) and np.isnan(got[1])
    assert np.isnan(binding.load_library().slrhip_sample_luminance(4, v.ctypes.data))


def library_weights():
    """The per-bin weights of the library, read through the export: Y of the unit sample of bin b is ybar[b] / integralCMF (the
    other terms of the sum are exact zeros)."""
    return host_luminance(np.eye(16, dtype=F))


def test_spectral_weights_equal_the_table():
    w, integral = cmf16()
    assert w.min() > 0 and integral > 0
    assert_same_bits(library_weights(), w / integral, "ybar[b] / integralCMF")


def test_spectral_weights_equal_the_reference(ref_spectral):
    f = ref_spectral.lib.slr_ref_dump_table
    f.restype = C.c_long
    f.argtypes = [C.c_int, C.c_char_p, C.c_void_p, C.c_long]
    n = f(5, None, None, 0)                                # xbar[16], ybar[16], zbar[16], integralCMF of DiscretizedSpectrum
    assert n == 49
    t = np.zeros(n, F)
    f(5, None, t.ctypes.data, n)
    assert_same_bits(library_weights(), t[16:32] / t[48], "DiscretizedSpectrum::ybar / integralCMF")


def test_host_program_parses_the_noise_flags(capsys):
    ap = host.build_parser()
    a = ap.parse_args(["scene.txt"])
    assert a.noise_target is None and a.noise_metric == "rmse" and a.noise_step == 16 and a.max_spp == 0 and a.noise_map is None
    a = ap.parse_args(["scene.txt", "--noise-target", "0.01", "--noise-metric", "relative", "--noise-step", "8", "--max-spp", "256",
                       "--noise-map", "noise.npy"])
    assert (a.noise_target, a.noise_metric, a.noise_step, a.max_spp, a.noise_map) == (0.01, "relative", 8, 256, "noise.npy")
    assert abi.NOISE_METRICS[a.noise_metric] == abi.NOISE_RELATIVE
    with pytest.raises(SystemExit):
        ap.parse_args(["scene.txt", "--noise-metric", "psnr"])
    with pytest.raises(SystemExit):                        # the map and the limit belong to --noise-target
        host.main(["scene.txt", "--noise-map", "noise.npy"])
    capsys.readouterr()
