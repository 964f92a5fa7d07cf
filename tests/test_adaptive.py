"""Adaptive sampling (slrhip_render_adaptive / slrhip_read_framebuffer_mean / slrhip_adaptive_active): pixels retire on their own
noise record, later blocks render only the rest.

The yardstick is the render path without any of this: PER-PASS FRAMES — render_begin; render(p, 1); read_framebuffer, where the
sensor's Kahan sum of one value from zero is that value (in one test: the CPU oracle's per-pass frames, after the existing
oracle-vs-GPU parity) — and a numpy float32 restatement, written here, of the sample luminance, the Welford update, the sensor's
Kahan sum and the retirement rule of include/slrhip.h.  The restatement says which pixel gets how many passes; the adaptive
render must then give, bit for bit, the Kahan sum and the Welford record of each pixel's first n(x, y) per-pass values.

Input condition.  scenes.cornell_box_spheres(1.0, 16, 8, "matte"), 64 x 48, seed 5, spp_min = 4, spp_step = 4, spp_max = 24,
floor = 0.05, threshold = 2^-9 = 0.001953125, chosen on the CPU with the oracle's per-pass frames: at 0.25, 0.125 and 0.5 the
input is degenerate (nearly every pixel is darker than the floor and retires at the first check), so the threshold was halved
until the condition below held with a wide margin.  Pixels by the count at which they retired (0: still active at spp_max), from
the oracle's per-pass frames on the CPU with expect_adaptive below:
    RGB, 3072 pixels, min 4 step 4 max 24
        0.5      {4: 3072}
        0.25     {4: 3030, 8: 42}
        0.125    {4: 3029, 8: 2, 12: 7, 16: 1, 20: 8, 24: 25}
        2^-7     {0: 48, 4: 2860, 8: 135, 12: 22, 16: 3, 20: 4}
        2^-8     {0: 76, 4: 2318, 8: 425, 12: 146, 16: 67, 20: 27, 24: 13}
        2^-9     {0: 380, 4: 1782, 8: 343, 12: 190, 16: 170, 20: 110, 24: 97}        chosen
        2^-10    {0: 1244, 4: 1178, 8: 251, 12: 152, 16: 100, 20: 75, 24: 72}
    RGB at 2^-9, min 3 step 5: max 23 {0: 360, 3: 1850, 8: 367, 13: 207, 18: 168, 23: 120}; max 22 {0: 383, ..., 18: 168, 22: 97}
    spectral ("glass", 32 x 24 = 768 pixels), min 4 step 4 max 12
        0.25     {0: 1, 4: 751, 8: 16}
        2^-8     {0: 57, 4: 578, 8: 103, 12: 30}
        2^-9     {0: 204, 4: 438, 8: 88, 12: 38}                                      chosen
Every test that relies on it asserts on the restated expectation, BEFORE it looks at the GPU result, that at least 5 % of the
pixels retire at the first check, at least 5 % are still active at spp_max and at least three distinct retirement passes occur
(spectral case: two), so that a degenerate input fails loudly."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, host, scenes, spectra

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHANNELS = (abi.STATISTICS_MEAN, abi.STATISTICS_VARIANCE, abi.STATISTICS_VARIANCE_OF_MEAN, abi.STATISTICS_COUNT, abi.STATISTICS_MAX)
FLOOR = 0.05
THRESHOLD = 2.0 ** -9             # both cases, see above


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


class Sensor:
    """The sensor and the noise records of a frame, float32 steps: add(frame, take) adds the per-pass frame to the pixels of the
    mask `take` — the Kahan sum of BasicTypes/CompensatedSum.h per component, the Welford step of include/slrhip.h on the
    luminance — and retires(threshold, floor) evaluates the retirement rule on every pixel's record."""

    def __init__(self, height, width, components):
        self.sum, self.comp = np.zeros((height, width, components), F), np.zeros((height, width, components), F)
        self.mean, self.m2, self.max = np.zeros((height, width), F), np.zeros((height, width), F), np.zeros((height, width), F)
        self.n = np.zeros((height, width), np.uint32)

    def add(self, frame, take):
        with np.errstate(all="ignore"):
            v = np.asarray(frame, F)
            c_input = v - self.comp
            sum_temp = self.sum + c_input
            comp = (sum_temp - self.sum) - c_input
            y = luminance(v)
            n = self.n + np.uint32(1)
            d = y - self.mean
            mean = self.mean + d / n.astype(F)
            m2 = self.m2 + d * (y - mean)
            mx = np.fmax(self.max, y)
        for a in (sum_temp, comp, mean, m2, mx):
            assert a.dtype == F
        t3 = take[:, :, None]
        self.sum, self.comp = np.where(t3, sum_temp, self.sum), np.where(t3, comp, self.comp)
        self.mean, self.m2, self.max = np.where(take, mean, self.mean), np.where(take, m2, self.m2), np.where(take, mx, self.max)
        self.n = np.where(take, n, self.n)

    def retires(self, threshold, floor):
        with np.errstate(all="ignore"):
            n = self.n
            vom = self.m2 / ((n - np.uint32(1)).astype(F) * n.astype(F))
            m = np.fmax(self.mean, F(floor))
            a = F(threshold) * m
            aa = a * a
            assert vom.dtype == F and aa.dtype == F
            return (n >= 2) & ~np.isnan(self.mean) & (vom <= aa)          # a comparison with NaN is False

    def channels(self):
        with np.errstate(all="ignore"):
            n, two = self.n, self.n >= 2
            zero = np.zeros_like(self.mean)
            return {abi.STATISTICS_MEAN: self.mean, abi.STATISTICS_MAX: self.max, abi.STATISTICS_COUNT: n.astype(F),
                    abi.STATISTICS_VARIANCE: np.where(two, self.m2 / (n - np.uint32(1)).astype(F), zero),
                    abi.STATISTICS_VARIANCE_OF_MEAN: np.where(two, self.m2 / ((n - np.uint32(1)).astype(F) * n.astype(F)), zero)}

    def mean_frame(self):
        with np.errstate(all="ignore"):
            n = self.n[:, :, None]
            return np.where(n > 0, self.sum / n.astype(F), F(0)).astype(F)


def block_lengths(spp_min, spp_step, spp_max):
    """The blocks of a call, restated: spp_min, then spp_step each, the last cut to fit spp_max."""
    out, done = [spp_min], spp_min
    while done < spp_max:
        out.append(min(spp_step, spp_max - done))
        done += out[-1]
    return out


def expect_adaptive(frames, threshold, floor, spp_min, spp_step, spp_max, spp_begin=0, sensor=None, active=None):
    """One adaptive call on per-pass frames frames[pass]: dict(sensor, active, retired_at, spp_done, samples)."""
    h, w, comps = frames[0].shape
    sensor = sensor or Sensor(h, w, comps)
    active = np.ones((h, w), bool) if active is None else active.copy()
    retired_at = np.zeros((h, w), np.uint32)              # the pixel's count when it retired in this call; 0: it did not
    done = samples = 0
    for block in block_lengths(spp_min, spp_step, spp_max):
        if not active.any():
            break
        for p in range(spp_begin + done, spp_begin + done + block):
            sensor.add(frames[p], active)
        done += block
        samples += int(active.sum()) * block
        retire = active & sensor.retires(threshold, floor)
        retired_at[retire] = sensor.n[retire]
        active &= ~retire
    return dict(sensor=sensor, active=active, retired_at=retired_at, spp_done=done, samples=samples)


def histogram(want):
    values, counts = np.unique(want["retired_at"], return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


def assert_input_condition(want, spp_min, distinct):
    """At least 5 % retire at the first check, at least 5 % stay active to the end, `distinct` different retirement passes."""
    hist = histogram(want)
    print("retirement histogram (count at retirement: pixels; 0 = still active):", hist)
    pixels = want["active"].size
    assert hist.get(spp_min, 0) >= 0.05 * pixels, hist
    assert hist.get(0, 0) >= 0.05 * pixels and hist.get(0, 0) == int(want["active"].sum()), hist
    assert len([k for k in hist if k != 0]) >= distinct, hist


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


def snapshot(ctx, **more):
    got = dict(frame=ctx.read_framebuffer(), mean_frame=ctx.read_framebuffer_mean(), active=ctx.adaptive_active(),
               counter_samples=ctx.counters().samples, **more)
    got.update({c: ctx.statistics(c) for c in CHANNELS})
    return got


def run_adaptive(ctx, st, target, shard=(0, 1), calls=1):
    """render_begin, statistics_begin, then `calls` adaptive calls of the target (threshold, floor, min, step, max) — or one call
    per target of a list — each from where the one before stopped."""
    ctx.render_begin(st, shard)
    ctx.statistics_begin()
    begin, done_list, samples = 0, [], 0
    for target in (target if isinstance(target, list) else [target] * calls):
        done, s = ctx.render_adaptive(begin, *target)
        begin += done
        samples += s
        done_list.append(done)
    return snapshot(ctx, spp_done=done_list, samples=samples)


def assert_matches(got, want, exact_zero_sign=True):
    """A GPU snapshot against an expectation of expect_adaptive, bit for bit (exact_zero_sign False: -0 equals +0 where the
    oracle's frames may hold a -0 sample)."""
    sensor = want["sensor"]
    loose = assert_same_bits if exact_zero_sign else assert_bit_equal
    assert_same_bits(got[abi.STATISTICS_COUNT], sensor.n.astype(F), "COUNT")
    loose(got["frame"], sensor.sum, "frame = Kahan sum of each pixel's first n per-pass values")
    ch = sensor.channels()
    for c in (abi.STATISTICS_VARIANCE, abi.STATISTICS_VARIANCE_OF_MEAN):
        assert_same_bits(got[c], ch[c], abi.STATISTICS_CHANNELS[c])
    for c in (abi.STATISTICS_MEAN, abi.STATISTICS_MAX):
        loose(got[c], ch[c], abi.STATISTICS_CHANNELS[c])
    loose(got["mean_frame"], sensor.mean_frame(), "mean frame = sum / n")
    assert sum(got["spp_done"]) == want["spp_done"]
    assert got["samples"] == want["samples"] == int(sensor.n.sum())
    assert got["counter_samples"] == want["samples"]
    assert got["active"] == int(want["active"].sum())


def make_case(mode, material, width, height, passes):
    sc = scenes.cornell_box_spheres(1.0, 16, 8, material)
    st = ob.settings(width, height, seed=5)
    ctx = Context(mode=mode)
    ctx.upload_scene(sc)
    return dict(scene=sc, settings=st, ctx=ctx, frames=per_pass_frames(ctx, st, passes), passes=passes)


@pytest.fixture(scope="module")
def rgb_case():
    case = make_case(abi.MODE_RGB, "matte", 64, 48, 24)
    case["target"] = (THRESHOLD, FLOOR, 4, 4, 24)
    case["got"] = run_adaptive(case["ctx"], case["settings"], case["target"])
    yield case
    case["ctx"].close()


@pytest.fixture(scope="module")
def spectral_case():
    case = make_case(abi.MODE_SPECTRAL, "glass", 32, 24, 12)
    case["target"] = (THRESHOLD, FLOOR, 4, 4, 12)
    case["got"] = run_adaptive(case["ctx"], case["settings"], case["target"])
    yield case
    case["ctx"].close()


# ---- 1, 2, 3: bit-exact against the restatement ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rgb_bit_exact(rgb_case):
    """24 passes in blocks of 4: the four-entry loop of the indexed fold, over lists that shrink from check to check.
    Threshold 2^-9; expected retirement histogram (count at retirement: pixels, 0 = active at spp_max), from the oracle's frames:
    {0: 380, 4: 1782, 8: 343, 12: 190, 16: 170, 20: 110, 24: 97} of 3072 pixels."""
    want = expect_adaptive(rgb_case["frames"], *rgb_case["target"])
    assert_input_condition(want, 4, 3)
    assert_matches(rgb_case["got"], want)


@pytest.mark.gpu
def test_rgb_bit_exact_remainder_loop_and_cut_last_block(rgb_case):
    """spp_min 3, step 5, max 23: blocks 3, 5, 5, 5, 5 — the remainder loop of the fold (3 = 0 x 4 + 3, 5 = 4 + 1); max 22 cuts
    the last block: 3, 5, 5, 5, 4."""
    for spp_max, blocks in ((23, [3, 5, 5, 5, 5]), (22, [3, 5, 5, 5, 4])):
        assert block_lengths(3, 5, spp_max) == blocks
        target = (THRESHOLD, FLOOR, 3, 5, spp_max)
        want = expect_adaptive(rgb_case["frames"], *target)
        assert_input_condition(want, 3, 3)
        assert_matches(run_adaptive(rgb_case["ctx"], rgb_case["settings"], target), want)


@pytest.mark.gpu
def test_rgb_from_oracle_frames(rgb_case, oracle_rgb):
    """The same with the per-pass frames of the CPU oracle.  That they equal the GPU's per-pass frames is the existing parity of
    the render path, asserted first so that a failure names its cause."""
    osc = oracle_rgb.scene(rgb_case["scene"])
    frames = [osc.render(rgb_case["settings"], 1, spp_begin=p)[0].astype(F) for p in range(rgb_case["passes"])]
    for p, (a, b) in enumerate(zip(frames, rgb_case["frames"])):
        assert_bit_equal(a, b, "existing parity: oracle vs GPU frame of pass %d" % p)
    want = expect_adaptive(frames, *rgb_case["target"])
    assert_input_condition(want, 4, 3)
    assert_matches(rgb_case["got"], want, exact_zero_sign=False)          # a -0 sample of the oracle is a +0 one here


@pytest.mark.gpu
def test_spectral_bit_exact(spectral_case):
    """Four lanes per pixel in the indexed fold: the quad of compact pixel i adds into the four planes of pixel activeIndex[i], and
    the quad exchange gives all four the same luminance.  Threshold 2^-9; expected retirement histogram from the oracle's frames:
    {0: 204, 4: 438, 8: 88, 12: 38} of 768 pixels."""
    want = expect_adaptive(spectral_case["frames"], *spectral_case["target"])
    assert_input_condition(want, 4, 2)
    assert_matches(spectral_case["got"], want)


# ---- 4: independence ------------------------------------------------------------------------------------------------------------
INDEPENDENCE = dict(width=160, height=120, target=(THRESHOLD, FLOOR, 4, 4, 12))
KEYS = ("frame", "mean_frame") + CHANNELS

CHILD = """
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import test_adaptive as t
from oracle import binding as ob
from slr_amd import Context, abi, scenes
cfg = t.INDEPENDENCE
ctx = Context(mode=abi.MODE_RGB, stripes=1)
ctx.upload_scene(scenes.cornell_box_spheres(1.0, 16, 8, "matte"))
got = t.run_adaptive(ctx, ob.settings(cfg["width"], cfg["height"], seed=5), cfg["target"])
ctx.close()
np.savez(sys.argv[1], **{str(k): np.asarray(v) for k, v in got.items()})
"""


@pytest.mark.gpu
def test_result_does_not_depend_on_slots_shards_windows_or_calls(tmp_path):
    """160 x 120 pixels: a block of 4 passes is 1.2 MB of results, so SLRHIP_RESULT_WINDOW_MB=1 cuts the first block into windows of
    3 + 1 passes, and later blocks as the active count allows."""
    cfg = INDEPENDENCE
    sc, st = scenes.cornell_box_spheres(1.0, 16, 8, "matte"), ob.settings(cfg["width"], cfg["height"], seed=5)
    pixels = cfg["width"] * cfg["height"]
    assert pixels * 16 * 4 > (1 << 20) > pixels * 16 * 3
    env = dict(os.environ, SLRHIP_RESULT_WINDOW_MB="1")
    child = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests")), str(tmp_path / "child.npz")], env=env)
    try:
        ctx = Context(mode=abi.MODE_RGB, stripes=1)
        ctx.upload_scene(sc)
        whole = run_adaptive(ctx, st, cfg["target"])
        counts = whole[abi.STATISTICS_COUNT]
        assert 0 < whole["active"] < pixels and len(np.unique(counts)) >= 3, "the input retires nothing, or everything at once"
        assert whole["spp_done"] == [12] and whole["samples"] == int(counts.sum()) == whole["counter_samples"]
        t, f, spp_min, step, _ = cfg["target"]
        two = run_adaptive(ctx, st, (t, f, spp_min, step, 4), calls=3)          # three calls of one block each, cut at the block boundaries
        parts = [run_adaptive(ctx, st, cfg["target"], shard=(i, 3)) for i in range(3)]
        # spp_min != spp_step: blocks 4, 2, 2, 2, 2 in one call; cut after 8 passes, the second call takes the STEP as its spp_min
        uneven = run_adaptive(ctx, st, (t, f, 4, 2, 12))
        uneven_cut = run_adaptive(ctx, st, [(t, f, 4, 2, 8), (t, f, 2, 2, 4)])
        ctx.close()
        auto = Context(mode=abi.MODE_RGB, stripes=0)
        auto.upload_scene(sc)
        stripes = run_adaptive(auto, st, cfg["target"])
        auto.close()
    finally:
        assert child.wait(timeout=120) == 0
    windows = np.load(str(tmp_path / "child.npz"))
    for k in KEYS:
        name = k if isinstance(k, str) else abi.STATISTICS_CHANNELS[k]
        assert_same_bits(two[k], whole[k], "three calls vs one: " + name)
        assert_same_bits(uneven_cut[k], uneven[k], "min 4 step 2 max 12 vs (4, 2, 8) then (2, 2, 4): " + name)
        assert_same_bits(stripes[k], whole[k], "automatic slot count vs stripes = 1: " + name)
        assert_same_bits(windows[str(k)], whole[k], "result windows of 1 MiB (child process) vs one window: " + name)
        assert_same_bits(parts[0][k] + parts[1][k] + parts[2][k], whole[k], "three shards added vs the whole frame: " + name)
        assert (((parts[0][k] != 0).astype(int) + (parts[1][k] != 0) + (parts[2][k] != 0)) <= 1).all()
    assert two["spp_done"] == [4, 4, 4]
    assert uneven["spp_done"] == [12] and uneven_cut["spp_done"] == [8, 4] and len(np.unique(uneven[abi.STATISTICS_COUNT])) >= 4
    assert (uneven_cut["active"], uneven_cut["samples"]) == (uneven["active"], uneven["samples"])
    for other in (two, stripes, dict(active=int(windows["active"]), samples=int(windows["samples"]))):
        assert (other["active"], other["samples"]) == (whole["active"], whole["samples"])
    assert sum(p["active"] for p in parts) == whole["active"] and sum(p["samples"] for p in parts) == whole["samples"]


# ---- 5: the ordinary path is untouched ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ordinary_render_after_an_adaptive_one(rgb_case):
    ctx, st, sc = rgb_case["ctx"], rgb_case["settings"], rgb_case["scene"]
    fresh = Context(mode=abi.MODE_RGB)
    fresh.upload_scene(sc)
    fresh.render_begin(st)
    fresh.render(0, 8)
    want_frame = fresh.read_framebuffer()
    fresh.render_features(abi.FEATURE_ALL, 2)
    want_features = {c: fresh.features(c) for c in abi.FEATURE_CHANNELS}
    want_rays = fresh.camera_rays(3)
    fresh.close()

    got = run_adaptive(ctx, st, rgb_case["target"])
    assert 0 < got["active"] < 64 * 48
    ctx.render_features(abi.FEATURE_ALL, 2)                                  # the shard's pixel list, not the active one
    for c in abi.FEATURE_CHANNELS:
        assert np.array_equal(ctx.features(c).view(np.uint32), want_features[c].view(np.uint32)), abi.FEATURE_CHANNELS[c][0]
    rows, xy = ctx.camera_rays(3)
    assert len(xy) == 64 * 48 and np.array_equal(xy, want_rays[1]) and np.array_equal(rows.view(np.uint32), want_rays[0].view(np.uint32))
    before = got[abi.STATISTICS_COUNT]
    ctx.render(24, 5)                                                        # slrhip_render after retirement: every pixel, retired or not
    assert_same_bits(ctx.statistics(abi.STATISTICS_COUNT), before + F(5), "COUNT after render(24, 5)")
    assert ctx.adaptive_active() == got["active"], "slrhip_render retires nothing and revives nothing"
    assert ctx.counters().samples == got["samples"] + 5 * 64 * 48
    ctx.render_begin(st)                                                     # every pixel is active again
    assert ctx.adaptive_active() == 64 * 48
    ctx.render(0, 8)
    assert_same_bits(ctx.read_framebuffer(), want_frame, "render_begin + render(0, 8) after an adaptive render vs a fresh context")


# ---- 6: edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_threshold_zero_and_infinity(rgb_case):
    ctx, st, frames = rgb_case["ctx"], rgb_case["settings"], rgb_case["frames"]
    # threshold 0: only a pixel whose samples all had the same luminance retires (M2 == 0); the rest get spp_max passes
    target = (0.0, FLOOR, 4, 4, 12)
    want = expect_adaptive(frames, *target)
    noisy = want["sensor"].m2 > 0
    assert noisy.mean() >= 0.5 and (want["sensor"].n[noisy] == 12).all()
    assert (want["retired_at"][~noisy] == 4).all()
    got = run_adaptive(ctx, st, target)
    assert_matches(got, want)
    ctx.render_begin(st)
    ctx.render(0, 12)
    plain = ctx.read_framebuffer()
    assert_same_bits(got["frame"][noisy], plain[noisy], "threshold 0 vs render(0, 12) on the pixels with noise")
    # threshold infinity (floor > 0): every pixel retires at spp_min, the frame is render(0, spp_min)'s
    target = (float("inf"), FLOOR, 4, 4, 12)
    want = expect_adaptive(frames, *target)
    assert not want["active"].any() and (want["sensor"].n == 4).all()
    got = run_adaptive(ctx, st, target)
    assert_matches(got, want)
    assert got["spp_done"] == [4] and got["active"] == 0
    # nothing is active: a second call renders nothing
    assert ctx.render_adaptive(4, *target) == (0, 0)
    assert_same_bits(ctx.read_framebuffer(), got["frame"], "frame after an adaptive call with no active pixel")
    ctx.render_begin(st)
    ctx.render(0, 4)
    assert_same_bits(got["frame"], ctx.read_framebuffer(), "threshold infinity vs render(0, 4)")


@pytest.mark.gpu
def test_image_smaller_than_one_wave_and_a_shard_mean():
    """8 x 8 pixels: one partial workgroup of the select.  Then the mean resolve of a shard: sum / n, zeros outside it."""
    sc = scenes.cornell_box_spheres(1.0, 16, 8, "matte")
    ctx = Context(mode=abi.MODE_RGB)
    ctx.upload_scene(sc)
    st = ob.settings(8, 8, seed=5)
    frames = per_pass_frames(ctx, st, 12)
    target = (THRESHOLD, FLOOR, 4, 4, 12)
    want = expect_adaptive(frames, *target)
    assert 0 < int(want["active"].sum()) < 64, histogram(want)
    assert_matches(run_adaptive(ctx, st, target), want)
    st = ob.settings(64, 48, seed=5)
    got = run_adaptive(ctx, st, target, shard=(1, 3))
    ctx.close()
    n, total = got[abi.STATISTICS_COUNT], got["frame"]
    inside = n > 0
    assert 0.3 * n.size < inside.sum() < 0.4 * n.size and len(np.unique(n[inside])) >= 2
    with np.errstate(all="ignore"):
        want_mean = np.where(inside[:, :, None], total / n[:, :, None], F(0)).astype(F)
    assert_same_bits(got["mean_frame"], want_mean, "mean resolve of shard (1, 3)")
    assert not got["mean_frame"][~inside].view(np.uint32).any()


# ---- 7: argument errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(rgb_case):
    INVALID, NO_SCENE = r"\(1\)", r"\(4\)"
    good = (THRESHOLD, FLOOR, 4, 4, 8)
    fresh = Context()
    fresh.settings = rgb_case["settings"]
    for call in (lambda: fresh.render_adaptive(0, *good), fresh.read_framebuffer_mean, fresh.adaptive_active, lambda: fresh.mean_into(16, 1 << 20)):
        with pytest.raises(binding.SlrHipError, match=NO_SCENE):          # before render_begin
            call()
    fresh.close()

    ctx, st = rgb_case["ctx"], rgb_case["settings"]
    ctx.render_begin(st)
    for call in (lambda: ctx.render_adaptive(0, *good), ctx.read_framebuffer_mean, lambda: ctx.mean_into(16, 1 << 20)):
        with pytest.raises(binding.SlrHipError, match=INVALID + ".*statistics are off"):
            call()
    assert ctx.adaptive_active() == 64 * 48                                # needs no statistics
    ctx.statistics_begin()
    ctx.render(0, 3)
    before = ctx.read_framebuffer()
    nan, inf = float("nan"), float("inf")
    for target in ((nan, FLOOR, 4, 4, 8), (-0.5, FLOOR, 4, 4, 8), (THRESHOLD, nan, 4, 4, 8), (THRESHOLD, -1.0, 4, 4, 8), (-inf, FLOOR, 4, 4, 8),
                   (THRESHOLD, FLOOR, 1, 4, 8), (THRESHOLD, FLOOR, 0, 4, 8), (THRESHOLD, FLOOR, 4, 0, 8), (THRESHOLD, FLOOR, 4, 4, 3)):
        with pytest.raises(binding.SlrHipError, match=INVALID):
            ctx.render_adaptive(3, *target)
        assert ctx.counters().samples == 3 * 64 * 48 and ctx.adaptive_active() == 64 * 48
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*2\\^32"):
        ctx.render_adaptive(0xFFFFFFFC, *good)
    lib = ctx.lib
    t, done = abi.AdaptiveTarget(*good), C.c_uint32(7)
    assert lib.slrhip_render_adaptive(ctx.handle, 3, None, C.byref(done), None, None) == 1 and done.value == 0
    assert lib.slrhip_render_adaptive(ctx.handle, 3, C.byref(t), None, None, None) == 1
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*null"):
        ctx.mean_into(None, 1 << 20)
    with pytest.raises(binding.SlrHipError, match=INVALID + ".*too small"):
        ctx.mean_into(16, 64 * 48 * 3 - 1)
    assert_same_bits(ctx.read_framebuffer(), before, "frame after the refused calls")
    # the render is still usable: it goes on adaptively from pass 3 as if nothing had been refused
    sensor = Sensor(48, 64, 3)
    for p in range(3):
        sensor.add(rgb_case["frames"][p], np.ones((48, 64), bool))
    want = expect_adaptive(rgb_case["frames"], *good, spp_begin=3, sensor=sensor)
    done, samples = ctx.render_adaptive(3, *good)
    want["samples"] += 3 * 64 * 48
    assert_matches(snapshot(ctx, spp_done=[done], samples=samples + 3 * 64 * 48), want)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("slrhip_render_adaptive", "slrhip_resolve_framebuffer_mean", "slrhip_read_framebuffer_mean", "slrhip_adaptive_active")


def test_library_exports_the_adaptive_symbols():
    lib = binding.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in binding.EXPORTS
    assert lib.slrhip_version() == 7
    assert C.sizeof(abi.AdaptiveTarget) == 20 and abi.AdaptiveTarget.spp_max.offset == 16
    done, count = C.c_uint32(7), C.c_uint32(7)
    assert lib.slrhip_render_adaptive(None, 0, None, C.byref(done), None, None) == 1 and done.value == 0      # no GPU needed to refuse
    assert lib.slrhip_resolve_framebuffer_mean(None, None, 0, None) == 1 and lib.slrhip_read_framebuffer_mean(None, None, 0) == 1
    assert lib.slrhip_adaptive_active(None, C.byref(count), None) == 1


def planned_blocks(spp_min, spp_step, spp_max, room=64):
    lib = binding.load_library()
    blocks, n = np.zeros(room, np.uint32), C.c_uint32(0)
    assert lib.slrhip_debug_adaptive_blocks(spp_min, spp_step, spp_max, blocks.ctypes.data, room, C.byref(n)) == 0
    return [int(b) for b in blocks[:min(n.value, room)]], n.value


@pytest.mark.parametrize("triple, blocks",
                         [((4, 4, 24), [4, 4, 4, 4, 4, 4]),
                          ((3, 5, 23), [3, 5, 5, 5, 5]),
                          ((3, 5, 22), [3, 5, 5, 5, 4]),          # the last block is cut
                          ((4, 4, 4), [4]),                       # max == min: one block
                          ((2, 1, 5), [2, 1, 1, 1]),
                          ((16, 64, 17), [16, 1]),                # a step longer than what is left
                          ((8, 100, 256), [8, 100, 100, 48])])
def test_block_plan(triple, blocks):
    """Values derived by hand from the rule: spp_min, then spp_step each, the last cut to fit spp_max."""
    got, n = planned_blocks(*triple)
    assert got == blocks and n == len(blocks) and sum(got) == triple[2]
    assert block_lengths(*triple) == blocks                       # the restatement the GPU tests use


def test_block_plan_refuses_what_the_entry_point_refuses():
    for triple in ((1, 4, 8), (0, 4, 8), (4, 0, 8), (4, 4, 3)):
        assert planned_blocks(*triple) == ([], 0)
    assert planned_blocks(2, 1, 100, room=3) == ([2, 1, 1], 99)    # more blocks than room: the count is still the plan's


def test_host_program_parses_the_adaptive_flags(capsys):
    ap = host.build_parser()
    a = ap.parse_args(["scene.txt"])
    assert a.adaptive is None and a.adaptive_floor == 0.05 and a.spp_min == 16
    a = ap.parse_args(["scene.txt", "--adaptive", "0.25", "--adaptive-floor", "0.1", "--spp-min", "4", "--noise-step", "8", "--max-spp", "64"])
    assert (a.adaptive, a.adaptive_floor, a.spp_min, a.noise_step, a.max_spp) == (0.25, 0.1, 4, 8, 64)
    for bad in (["--adaptive", "0.25", "--spp-min", "1"], ["--adaptive", "-1"], ["--adaptive", "nan"], ["--adaptive", "0.25", "--adaptive-floor", "-0.1"],
                ["--adaptive", "0.25", "--noise-target", "0.01"], ["--adaptive", "0.25", "--noise-step", "0"]):
        with pytest.raises(SystemExit):                            # refused before the scene is read
            host.main(["scene.txt"] + bad)
    capsys.readouterr()
