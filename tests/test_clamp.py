"""The sample clamp (slrhip_clamp_begin / slrhip_resolve_clamp / slrhip_clamp_summary / slrhip_clamp_sample) and the diagnostic
that feeds the fold with a caller's samples (slrhip_debug_fold).

Expected values come from PER-PASS FRAMES — render_begin; render(p, 1); read_framebuffer without a clamp: the sensor's Kahan sum
of one value from zero is that value, so the frames ARE the samples — and a numpy float32 restatement, written here, of the rule of
include/slrhip.h, of the Kahan sum, of the clamp records and of the fixed order of the summary's double sum.  The luminance, the
Welford steps and the adaptive rule are the restatements of test_statistics.py and test_adaptive.py.  Every comparison is bit for
bit, with one exception the header states: where the rule GENERATES a NaN (infinity x 0, infinity - infinity) its sign and payload
are unspecified (the host gives the x86 default NaN, the device another), so two NaNs compare equal here whatever their bits.
The limit of the render cases is the median of the strictly positive sample luminances; that it clamps at least 10 % of all
samples and leaves at least 10 % of the nonzero ones alone is asserted as a condition on the input."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import summary_double_sum
from oracle import binding as ob
from slr_amd import Context, abi, binding, host, scenes
from test_adaptive import expect_adaptive
from test_cabi import render_plan
from test_statistics import CHANNELS, F, luminance, per_pass_frames, welford

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROP = abi.CLAMP_DROP_NONFINITE
CLAMP_CHANNELS = (abi.CLAMP_CLAMPED, abi.CLAMP_DROPPED, abi.CLAMP_REMOVED, abi.CLAMP_LARGEST)
INF = F(np.inf)
ERR_INVALID_ARGUMENT, ERR_NO_SCENE = 1, 4          # include/slrhip.h


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def assert_same_bits(a, b, what):
    """Bit for bit; two NaNs are equal (see the module's docstring)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    assert a.shape == b.shape, what
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    assert not bad.any(), "%s: %d of %d floats differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


def clamp_restated(v, limit, flags):
    """The rule of include/slrhip.h on samples [..., C]: (samples as the sensor receives them, Y as given, Y as received, what)
    with what = 0 kept, 1 clamped, 2 dropped."""
    v, limit = np.asarray(v, F), F(limit)
    with np.errstate(all="ignore"):
        y = luminance(v)
        drop = ~(np.abs(y) < INF) if flags & DROP else np.zeros(y.shape, bool)
        clamp = ~drop & (y > limit)
        f = limit / y
        s = v * f[..., None]
        y2 = luminance(s)
        assert f.dtype == F and s.dtype == F and y2.dtype == F
    out = np.where(drop[..., None], F(0), np.where(clamp[..., None], s, v)).astype(F)
    y_out = np.where(drop, F(0), np.where(clamp, y2, y)).astype(F)
    return out, y, y_out, np.where(drop, 2, np.where(clamp, 1, 0))


class Records:
    """The clamp records of a frame: add(y_in, y_out, what, take) is one pass of the pixels of the mask `take`."""

    def __init__(self, height, width):
        self.clamped, self.dropped = np.zeros((height, width), np.uint32), np.zeros((height, width), np.uint32)
        self.removed, self.largest = np.zeros((height, width), F), np.zeros((height, width), F)

    def add(self, y_in, y_out, what, take=True):
        c = (what == 1) & take
        with np.errstate(all="ignore"):
            removed, largest = self.removed + (y_in - y_out), np.fmax(self.largest, y_in)
        assert removed.dtype == F and largest.dtype == F
        self.clamped, self.dropped = self.clamped + c.astype(np.uint32), self.dropped + ((what == 2) & take).astype(np.uint32)
        self.removed, self.largest = np.where(c, removed, self.removed), np.where(c, largest, self.largest)

    def channels(self):
        return {abi.CLAMP_CLAMPED: self.clamped.astype(F), abi.CLAMP_DROPPED: self.dropped.astype(F), abi.CLAMP_REMOVED: self.removed,
                abi.CLAMP_LARGEST: self.largest}


def clamp_frames(frames, limit, flags, counts=None):
    """(the clamped per-pass frames, the records); counts[h][w]: pixel gets the passes below its count only (adaptive)."""
    out, rec = [], Records(*frames[0].shape[:2])
    for p, fr in enumerate(frames):
        v, y_in, y_out, what = clamp_restated(fr, limit, flags)
        rec.add(y_in, y_out, what, True if counts is None else p < counts)
        out.append(v)
    return out, rec


def kahan(frames):
    """The sensor after the per-pass frames: BasicTypes/CompensatedSum.h per component, float32."""
    s, c = np.zeros_like(frames[0]), np.zeros_like(frames[0])
    with np.errstate(all="ignore"):
        for v in frames:
            c_input = v - c
            sum_temp = s + c_input
            c = (sum_temp - s) - c_input
            s = sum_temp
            assert s.dtype == F and c.dtype == F
    return s


def expected_summary(rec, pixel_list):
    """slrhip_clamp_summary of the records of the pixels of `pixel_list` (x | y << 16, the shard's order)."""
    x, y = pixel_list & 0xFFFF, pixel_list >> 16
    return dict(clamped=int(rec.clamped[y, x].sum()), dropped=int(rec.dropped[y, x].sum()), removed=summary_double_sum(rec.removed[y, x]),
                largest=float(np.fmax.reduce(rec.largest[y, x], initial=F(0))))


def assert_summary(got, want, what):
    print("%s: summary %r, restated %r" % (what, got, want))
    assert (got["clamped"], got["dropped"]) == (want["clamped"], want["dropped"]), what
    assert got["removed"] == want["removed"] or (math.isnan(got["removed"]) and math.isnan(want["removed"])), what
    assert_same_bits(F(got["largest"]), F(want["largest"]), what + ": largest")


def pixel_list(ctx, st, shard=(0, 1), stripes=0):
    mode = abi.MODE_SPECTRAL if ctx.components == 16 else abi.MODE_RGB
    return render_plan(ctx.lib, st.image_width, st.image_height, shard, stripes, mode, want_pixels=True)[2]


# ---- the edge cases: one sample each -------------------------------------------------------------------------------------------
def edge_limit(components):
    """(limit, base): base is an ordinary sample and limit its luminance, so that base is the case Y == limit."""
    base = (np.arange(components, dtype=F) % 5 + F(1)) * F(0.2)
    return luminance(base), base


def edge_samples(components):
    """name -> sample [C] for the limit of edge_limit."""
    limit, base = edge_limit(components)
    k = 1 if components == 3 else 6                       # the component with the largest luminance weight
    above = None
    for j in range(components):                           # component j of base + 0, 1, 2, ... ulps until Y is the float after the limit
        steps = np.tile(base, (1 << 12, 1))
        steps[:, j] = (base[j:j + 1].view(np.uint32) + np.arange(1 << 12, dtype=np.uint32)).view(F)
        hit = luminance(steps) == np.nextafter(limit, INF)
        if hit.any():
            above = steps[np.argmax(hit)]
            break
    assert above is not None, "no sample one ulp above the limit within 2^12 ulps of a component"
    tiny = np.full(components, 1e-40, F)
    big = np.full(components, np.finfo(F).max, F)           # 16 components: w x v overflows; 3: the weights add up to 1, Y is the largest finite float
    with np.errstate(over="ignore"):
        assert components == 3 or np.isinf(luminance(big))
    cases = {"Y == limit": base, "Y one ulp above limit": above, "twice the limit": base * F(2), "huge": base * F(1e30),
             "NaN component": np.where(np.arange(components) == 1, F(np.nan), base), "+inf component": np.where(np.arange(components) == 0, INF, base),
             "-inf component": np.where(np.arange(components) == 2, -INF, base),
             "+inf and -inf": np.where(np.arange(components) == 0, INF, np.where(np.arange(components) == 2, -INF, base)),
             "finite components, Y overflows (16) or is the largest float (3)": big, "negative components": -base * F(3),
             "mixed signs above the limit": np.where(np.arange(components) == k, base * F(40), -base), "all zeros": np.zeros(components, F),
             "negative zeros": np.full(components, -0.0, F), "denormals": tiny, "denormal result": base * F(1e-38)}
    return {name: np.ascontiguousarray(v, F) for name, v in cases.items()}


def host_clamp(v, limit, flags):
    out = [binding.clamp_sample(row, float(limit), flags) for row in v]
    return (np.array([o[1] for o in out], F), np.array([o[2] for o in out], F), np.array([o[3] for o in out], F), np.array([o[0] for o in out]))


# ---- CPU tests ------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("slrhip_clamp_begin", "slrhip_resolve_clamp", "slrhip_read_clamp", "slrhip_clamp_summary", "slrhip_clamp_sample", "slrhip_debug_fold")


def test_library_exports_the_clamp_symbols():
    lib = binding.load_library()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in binding.EXPORTS
    assert lib.slrhip_version() == 7
    assert C.sizeof(abi.ClampDesc) == 16 and C.sizeof(abi.ClampSummary) == 32


@pytest.mark.parametrize("flags", [0, DROP])
@pytest.mark.parametrize("components", [3, 16])
def test_clamp_sample_equals_the_restatement(components, flags):
    rng = np.random.default_rng(11 + components)
    limit, _ = edge_limit(components)
    edges = edge_samples(components)
    # about a thousand random samples around the limit (luminances from far below to far above it), some with negative components
    v = (rng.random((1000, components)) * np.exp(rng.normal(0, 2, (1000, 1)))).astype(F) * limit
    v[::7] *= np.where(rng.random((v[::7].shape)) < 0.3, F(-1), F(1))
    v = np.concatenate([v, np.stack(list(edges.values()))])
    for lim in (limit, INF, F(1e-30)):
        want = clamp_restated(v, lim, flags)
        got = host_clamp(v, lim, flags)
        for g, w, name in zip(got[:3], want[:3], ("values", "Y as given", "Y as received")):
            assert_same_bits(g, w, "%d components, limit %r, flags %u: %s" % (components, lim, flags, name))
        assert (got[3] == want[3]).all()
    what = dict(zip(edges, clamp_restated(np.stack(list(edges.values())), limit, flags)[3]))
    print(what)
    # the restatement itself on the cases whose outcome the header spells out
    assert what["Y == limit"] == 0 and what["Y one ulp above limit"] == 1 and what["negative components"] == 0 and what["all zeros"] == 0
    assert what["NaN component"] == what["+inf and -inf"] == what["-inf component"] == (2 if flags else 0)
    assert what["+inf component"] == (2 if flags else 1)
    counts = np.bincount(clamp_restated(v, limit, flags)[3], minlength=3)
    assert counts[0] > 100 and counts[1] > 100


def test_clamp_sample_refuses_other_component_counts():
    lib = binding.load_library()
    v = np.ones(16, F)
    out = np.full(16, 7, F)
    assert lib.slrhip_clamp_sample(4, v.ctypes.data, 1.0, 0, out.ctypes.data, None, None) == -1
    assert lib.slrhip_clamp_sample(3, None, 1.0, 0, out.ctypes.data, None, None) == -1
    assert lib.slrhip_clamp_sample(3, v.ctypes.data, 1.0, 0, None, None, None) == -1
    assert (out == 7).all()
    assert lib.slrhip_clamp_sample(3, v.ctypes.data, 0.5, 0, out.ctypes.data, None, None) == 1          # null y_in / y_out are allowed
    assert lib.slrhip_clamp_sample(3, v.ctypes.data, 0.5, 0, v.ctypes.data, None, None) == 1 and (v[:3] == out[:3]).all()      # in place


def test_clamp_begin_refuses_a_null_context_and_a_context_without_a_render():
    lib = binding.load_library()
    d = abi.ClampDesc(1.0, 0)
    assert lib.slrhip_clamp_begin(None, C.byref(d)) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_resolve_clamp(None, abi.CLAMP_CLAMPED, None, 0, None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_read_clamp(None, abi.CLAMP_CLAMPED, None, 0) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_clamp_summary(None, None, None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_debug_fold(None, None, 1) == ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_clamp_begin_before_render_begin():
    ctx = Context()
    d = abi.ClampDesc(1.0, 0)
    assert ctx.lib.slrhip_clamp_begin(ctx.handle, C.byref(d)) == ERR_NO_SCENE
    assert ctx.lib.slrhip_clamp_begin(ctx.handle, None) == ERR_INVALID_ARGUMENT
    s = abi.ClampSummary()
    assert ctx.lib.slrhip_clamp_summary(ctx.handle, C.byref(s), None) == ERR_NO_SCENE
    ctx.close()


def test_host_program_parses_the_clamp_flags(capsys):
    ap = host.build_parser()
    a = ap.parse_args(["scene.slr", "--clamp", "12.5", "--drop-nonfinite", "--clamp-map", "m.npy", "--adaptive", "0.01", "--denoise", "--device-tonemap"])
    assert (a.clamp, a.drop_nonfinite, a.clamp_map) == (12.5, True, "m.npy")
    a = ap.parse_args(["scene.slr"])
    assert (a.clamp, a.drop_nonfinite, a.clamp_map) == (None, False, None)
    for bad in (["--clamp", "0"], ["--clamp", "-1"], ["--clamp", "nan"], ["--clamp-map", "m.npy"]):
        with pytest.raises(SystemExit):
            host.main(["scene.slr"] + bad)
    assert "--clamp" in capsys.readouterr().err


# ---- GPU cases ------------------------------------------------------------------------------------------------------------------
def snapshot(ctx, statistics=True):
    got = dict(frame=ctx.read_framebuffer(), summary=ctx.clamp_summary())
    got.update({("clamp", c): ctx.clamp(c) for c in CLAMP_CHANNELS})
    if statistics:
        got.update({c: ctx.statistics(c) for c in CHANNELS})
    return got


def render_clamped(ctx, st, limit, flags, calls, shard=(0, 1), statistics=True):
    ctx.render_begin(st, shard)
    if statistics:
        ctx.statistics_begin()
    ctx.clamp_begin(limit, bool(flags & DROP))
    for begin, count in calls:
        ctx.render(begin, count)
    return snapshot(ctx, statistics)


def array_keys(got):
    return [k for k in got if k != "summary"]


def make_case(mode, material, width, height, passes):
    sc = scenes.cornell_box_spheres(1.0, 16, 8, material)
    st = ob.settings(width, height, seed=5)
    ctx = Context(mode=mode)
    ctx.upload_scene(sc)
    frames = per_pass_frames(ctx, st, passes)
    y = luminance(np.stack(frames))
    limit = F(np.median(y[y > 0]))
    clamped, rec = clamp_frames(frames, limit, 0)
    # the condition on the input: a limit that clamps nothing or everything proves nothing
    n_clamped, nonzero = int(rec.clamped.sum()), int((y != 0).sum())
    print("limit %r: %d of %d samples clamped, %d nonzero" % (limit, n_clamped, y.size, nonzero))
    assert n_clamped >= 0.1 * y.size and nonzero - n_clamped >= 0.1 * nonzero
    got = render_clamped(ctx, st, limit, 0, [(0, passes)])
    return dict(scene=sc, settings=st, ctx=ctx, mode=mode, frames=frames, limit=limit, clamped=clamped, records=rec, got=got, passes=passes)


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


# ---- 1: frame, statistics and records ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["rgb_case", "spectral_case"])
def test_frame_statistics_and_records_bit_exact(request, case_name):
    """RGB 7 passes: one trip of the four-entry loop and three of the remainder; spectral 5: the quad exchange in both loops."""
    case = request.getfixturevalue(case_name)
    ctx, st, got = case["ctx"], case["settings"], case["got"]
    assert_same_bits(got["frame"], kahan(case["clamped"]), "frame")
    assert not np.array_equal(got["frame"], kahan(case["frames"])), "the clamp changed nothing"
    want = welford(case["clamped"])
    for c in CHANNELS:
        assert_same_bits(got[c], want[c], abi.STATISTICS_CHANNELS[c])
    for c, w in case["records"].channels().items():
        assert_same_bits(got["clamp", c], w, abi.CLAMP_CHANNELS[c])
    assert float(got["clamp", abi.CLAMP_REMOVED].max()) > 0 and float(got["clamp", abi.CLAMP_LARGEST].max()) > float(case["limit"])
    assert_summary(got["summary"], expected_summary(case["records"], pixel_list(ctx, st)), "summary")
    assert got["summary"]["clamped"] == int(got["clamp", abi.CLAMP_CLAMPED].astype(np.float64).sum())
    assert got["summary"]["dropped"] == int(got["clamp", abi.CLAMP_DROPPED].astype(np.float64).sum()) == 0
    # statistics off: the same frame and records from the instantiation without the Welford step
    off = render_clamped(ctx, st, case["limit"], 0, [(0, case["passes"])], statistics=False)
    for k in array_keys(off):
        assert_same_bits(off[k], got[k], "statistics off: %r" % (k,))
    assert off["summary"] == got["summary"]
    with pytest.raises(binding.SlrHipError):
        ctx.statistics(abi.STATISTICS_MEAN)


# ---- 2: the clamp that does nothing, and the switch-off --------------------------------------------------------------------------
def counters_of(ctx):
    c = ctx.counters()
    return (c.samples, c.extension_rays, c.shadow_rays)


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["rgb_case", "spectral_case"])
def test_infinite_limit_is_a_render_without_a_clamp(request, case_name):
    case = request.getfixturevalue(case_name)
    ctx, st, passes = case["ctx"], case["settings"], case["passes"]
    render_clamped(ctx, st, case["limit"], 0, [(0, 1)])
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.render(0, passes)
    plain = {c: ctx.statistics(c) for c in CHANNELS}
    plain.update(frame=ctx.read_framebuffer(), counters=counters_of(ctx))
    with pytest.raises(binding.SlrHipError):               # ... after a clamped render of the same context: every render_begin switches it off
        ctx.clamp_summary()
    assert_same_bits(plain["frame"], kahan(case["frames"]), "no clamp_begin after a clamped render: the frame without a clamp")
    noop = render_clamped(ctx, st, INF, 0, [(0, passes)])
    assert counters_of(ctx) == plain["counters"]
    for k in ["frame"] + list(CHANNELS):
        assert_same_bits(noop[k], plain[k], "limit = infinity, flags = 0 vs no clamp: %r" % (k,))
    for c in CLAMP_CHANNELS:
        assert not noop["clamp", c].any()
    assert noop["summary"] == dict(clamped=0, dropped=0, removed=0.0, largest=0.0)


# ---- 3: independence -----------------------------------------------------------------------------------------------------------
def assert_equal_results(a, b, what):
    for k in array_keys(b):
        assert_same_bits(a[k], b[k], "%s: %r" % (what, k))


@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["rgb_case", "spectral_case"])
def test_result_does_not_depend_on_cuts_shards_slots_or_the_tail_kernel(request, case_name):
    case = request.getfixturevalue(case_name)
    ctx, st, passes, limit, whole = case["ctx"], case["settings"], case["passes"], case["limit"], case["got"]
    cut = render_clamped(ctx, st, limit, 0, [(0, 3), (3, passes - 3)])
    assert_equal_results(cut, whole, "passes cut after 3")
    assert cut["summary"] == whole["summary"]
    parts = [render_clamped(ctx, st, limit, 0, [(0, passes)], shard=(i, 2)) for i in range(2)]
    for k in array_keys(whole):
        assert_same_bits(parts[0][k] + parts[1][k], whole[k], "two shards added: %r" % (k,))
        assert not ((parts[0][k] != 0) & (parts[1][k] != 0)).any()
    for name in ("clamped", "dropped"):
        assert parts[0]["summary"][name] + parts[1]["summary"][name] == whole["summary"][name]
    assert max(p["summary"]["largest"] for p in parts) == whole["summary"]["largest"]
    for i in range(2):
        assert_summary(parts[i]["summary"], expected_summary(case["records"], pixel_list(ctx, st, (i, 2))), "shard %d of 2" % i)
    for what, kw in (("stripes = 2", dict(stripes=2)), ("the tail kernel", dict(flags=abi.FLAG_TAIL_KERNEL, stripes=2))):
        other = Context(mode=case["mode"], **kw)
        other.upload_scene(case["scene"])
        got = render_clamped(other, st, limit, 0, [(0, passes)])
        other.close()
        assert_equal_results(got, whole, what)
        assert got["summary"] == whole["summary"]


WINDOWS = dict(width=160, height=120, passes=4, limit=3e-4)          # about the median sample luminance of the scene

CHILD = """
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import test_clamp as t
from oracle import binding as ob
from slr_amd import Context, abi, scenes
cfg = t.WINDOWS
ctx = Context(mode=abi.MODE_RGB, stripes=1)
ctx.upload_scene(scenes.cornell_box_spheres(1.0, 16, 8, "matte"))
got = t.render_clamped(ctx, ob.settings(cfg["width"], cfg["height"], seed=5), cfg["limit"], 0, [(0, cfg["passes"])])
ctx.close()
np.savez(sys.argv[1], removed=got["summary"]["removed"], **{str(k): np.asarray(got[k]) for k in t.array_keys(got)})
"""


@pytest.mark.gpu
def test_result_does_not_depend_on_the_result_window(tmp_path):
    """160 x 120 pixels: 4 passes are 1.2 MB of results, so SLRHIP_RESULT_WINDOW_MB=1 (read once per process: a fresh child) folds
    them as windows of 3 + 1 passes; the records are loaded and stored once per window."""
    cfg = WINDOWS
    pixels = cfg["width"] * cfg["height"]
    assert pixels * 16 * 4 > (1 << 20) > pixels * 16 * 3
    env = dict(os.environ, SLRHIP_RESULT_WINDOW_MB="1")
    child = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests")), str(tmp_path / "child.npz")], env=env)
    try:
        ctx = Context(mode=abi.MODE_RGB, stripes=1)
        ctx.upload_scene(scenes.cornell_box_spheres(1.0, 16, 8, "matte"))
        whole = render_clamped(ctx, ob.settings(cfg["width"], cfg["height"], seed=5), cfg["limit"], 0, [(0, cfg["passes"])])
        ctx.close()
    finally:
        assert child.wait(timeout=120) == 0
    windows = np.load(str(tmp_path / "child.npz"))
    clamped = whole["summary"]["clamped"]
    assert 0.05 * pixels * cfg["passes"] < clamped < 0.95 * pixels * cfg["passes"]
    for k in array_keys(whole):
        assert_same_bits(windows[str(k)], whole[k], "result windows of 1 MiB (child process) vs one window: %r" % (k,))
    assert float(windows["removed"]) == whole["summary"]["removed"]


# ---- 4: adaptive sampling and render-until under a clamp ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case_name", ["rgb_case", "spectral_case"])
def test_adaptive_under_a_clamp(request, case_name):
    """The retirement rule runs on the records of the CLAMPED samples: the restatement of test_adaptive.py on the clamped frames."""
    case = request.getfixturevalue(case_name)
    ctx, st, passes, limit = case["ctx"], case["settings"], case["passes"], case["limit"]
    target = (2.0 ** -3, float(limit) * 0.25, 2, 1, passes)          # the floor in the units of the samples: a quarter of the limit
    want = expect_adaptive(case["clamped"], *target)
    counts = want["sensor"].n
    assert len(np.unique(counts)) >= 3, "COUNT does not differ between pixels: %r" % (np.unique(counts),)
    assert not np.array_equal(counts, expect_adaptive(case["frames"], *target)["sensor"].n), "the clamp does not change who retires"
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.clamp_begin(limit)
    done, samples = ctx.render_adaptive(0, *target)
    got = snapshot(ctx)
    assert (done, samples, ctx.adaptive_active()) == (want["spp_done"], want["samples"], int(want["active"].sum()))
    assert_same_bits(got["frame"], want["sensor"].sum, "frame")
    for c, w in want["sensor"].channels().items():
        assert_same_bits(got[c], w, abi.STATISTICS_CHANNELS[c])
    _, rec = clamp_frames(case["frames"], limit, 0, counts)
    for c, w in rec.channels().items():
        assert_same_bits(got["clamp", c], w, abi.CLAMP_CHANNELS[c])
    assert_summary(got["summary"], expected_summary(rec, pixel_list(ctx, st)), "summary")


@pytest.mark.gpu
def test_render_until_under_a_clamp(rgb_case):
    """The stop check reads the noise records of the clamped samples: the target lies between the metric after 4 and after 6 passes
    of the CLAMPED frames, and the unclamped frames are noisier than it at 6."""
    case = rgb_case
    ctx, st, limit = case["ctx"], case["settings"], case["limit"]

    def rmse(frames, n):
        return math.sqrt(float(welford(frames[:n])[abi.STATISTICS_VARIANCE_OF_MEAN].astype(np.float64).sum()) / (st.image_width * st.image_height))
    at4, at6 = rmse(case["clamped"], 4), rmse(case["clamped"], 6)
    target = 0.5 * (at4 + at6)
    print("rmse of the clamped frames after 4 passes %r, after 6 %r; unclamped after 6 %r; target %r" % (at4, at6, rmse(case["frames"], 6), target))
    assert at6 < target < at4 < rmse(case["clamped"], 2) and rmse(case["frames"], 6) > target
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.clamp_begin(limit)
    done, _ = ctx.render_until(abi.NOISE_RMSE, target, 2, 7)
    assert done == 6
    got = snapshot(ctx)
    assert_same_bits(got["frame"], kahan(case["clamped"][:6]), "frame")
    want = welford(case["clamped"][:6])
    for c in CHANNELS:
        assert_same_bits(got[c], want[c], abi.STATISTICS_CHANNELS[c])
    _, rec = clamp_frames(case["frames"][:6], limit, 0)
    for c, w in rec.channels().items():
        assert_same_bits(got["clamp", c], w, abi.CLAMP_CHANNELS[c])


# ---- 5: synthetic samples through the fold ---------------------------------------------------------------------------------------
SYNTHETIC = dict(width=13, height=5)


@pytest.fixture(scope="module")
def synthetic_contexts():
    sc = scenes.cornell_box_spheres(1.0, 16, 8, "matte")
    out = {}
    for mode in (abi.MODE_RGB, abi.MODE_SPECTRAL):
        out[mode] = Context(mode=mode)
        out[mode].upload_scene(sc)
    yield out
    for ctx in out.values():
        ctx.close()


def synthetic_samples(components, passes):
    """[passes][5][13][C]: ordinary samples around the limit, every edge case planted at a pixel of its own in pass 0 and, with
    7 passes, again in a pass of the remainder loop (pass 5) at another pixel."""
    w, h = SYNTHETIC["width"], SYNTHETIC["height"]
    limit, _ = edge_limit(components)
    rng = np.random.default_rng(3 * components + passes)
    v = (rng.random((passes, h, w, components)) * np.exp(rng.normal(0, 1.5, (passes, h, w, 1)))).astype(F) * limit
    where = {}
    for i, (name, sample) in enumerate(edge_samples(components).items()):
        pix = 3 * i + 1
        v[0, pix // w, pix % w] = sample
        where[name] = (pix // w, pix % w)
        if passes > 5:
            pix = 3 * i + 2
            v[5, pix // w, pix % w] = sample
    return v, limit, where


@pytest.mark.gpu
@pytest.mark.parametrize("statistics", [False, True])
@pytest.mark.parametrize("flags", [0, DROP])
@pytest.mark.parametrize("passes", [1, 7])
@pytest.mark.parametrize("mode", [abi.MODE_RGB, abi.MODE_SPECTRAL])
def test_synthetic_samples_through_the_fold(synthetic_contexts, mode, passes, flags, statistics):
    """13 x 5 pixels: less than one wave in RGB, 65 quads (a wave and one quad of the next) in spectral."""
    ctx = synthetic_contexts[mode]
    st = ob.settings(SYNTHETIC["width"], SYNTHETIC["height"], seed=1)
    samples, limit, where = synthetic_samples(ctx.components, passes)
    ctx.render_begin(st)
    if statistics:
        ctx.statistics_begin()
    ctx.clamp_begin(limit, bool(flags))
    before = counters_of(ctx)
    ctx.debug_fold(samples)
    got = snapshot(ctx, statistics)
    assert counters_of(ctx) == before == (0, 0, 0)
    clamped, rec = clamp_frames(list(samples), limit, flags)
    assert rec.clamped.sum() > 5 and (rec.dropped.sum() > 0) == bool(flags)
    assert_same_bits(got["frame"], kahan(clamped), "sensor")
    nan_pixel = where["NaN component"]
    assert np.isnan(got["frame"][nan_pixel]).any() == (not flags), "without the flag the NaN pixel is NaN, with it it is not"
    assert np.isfinite(got["frame"]).all() == bool(flags)
    if statistics:
        want = welford(clamped)
        # fmaxf(+0, -0) may return either zero (IEEE 754 maxNum leaves it open; numpy and the device differ): the pixel of the
        # negative-zeros sample has MAX = 0 of either sign, so the sign of a zero MAX is taken out of the comparison by adding +0
        got[abi.STATISTICS_MAX], want[abi.STATISTICS_MAX] = got[abi.STATISTICS_MAX] + F(0), want[abi.STATISTICS_MAX] + F(0)
        for c in CHANNELS:
            assert_same_bits(got[c], want[c], abi.STATISTICS_CHANNELS[c])
    for c, w in rec.channels().items():
        assert_same_bits(got["clamp", c], w, abi.CLAMP_CHANNELS[c])
    assert_summary(got["summary"], expected_summary(rec, pixel_list(ctx, st)), "summary")
    for refused in (ctx.statistics_begin, lambda: ctx.clamp_begin(1.0)):          # the fold counts as the render having begun
        with pytest.raises(binding.SlrHipError):
            refused()


@pytest.mark.gpu
def test_debug_fold_without_a_clamp_is_the_plain_fold(synthetic_contexts):
    """Clamp off: the kernels of a render without one; a second call adds to the first."""
    ctx = synthetic_contexts[abi.MODE_RGB]
    st = ob.settings(SYNTHETIC["width"], SYNTHETIC["height"], seed=1)
    samples, _, _ = synthetic_samples(3, 7)
    samples = np.nan_to_num(samples, nan=0.25, posinf=2.0, neginf=-2.0)
    ctx.render_begin(st)
    ctx.statistics_begin()
    ctx.debug_fold(samples[:3])
    ctx.debug_fold(samples[3:])
    assert_same_bits(ctx.read_framebuffer(), kahan(list(samples)), "sensor")
    want = welford(list(samples))
    for c in CHANNELS:
        assert_same_bits(ctx.statistics(c), want[c], abi.STATISTICS_CHANNELS[c])
    with pytest.raises(binding.SlrHipError):
        ctx.debug_fold(np.zeros((65,) + samples.shape[1:], F))
    with pytest.raises(binding.SlrHipError):
        ctx.debug_fold(np.zeros((0,) + samples.shape[1:], F))


# ---- 6: argument errors leave the context usable ----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(rgb_case):
    case = rgb_case
    ctx, st, lib = case["ctx"], case["settings"], case["ctx"].lib
    pixels = st.image_width * st.image_height
    # a hipMalloc'ed destination of pixels + 1 floats from the HIP runtime the library is bound to (torch's copy cannot open the
    # device in a process where libslrhip.so was loaded first)
    hip, dst = binding._hip_runtime(), C.c_void_p()
    binding._hip_check(hip.hipMalloc(C.byref(dst), 4 * (pixels + 1)), "hipMalloc")
    dst = dst.value
    summary = abi.ClampSummary()
    ctx.render_begin(st)
    # the clamp is off: resolve, read and summary refuse
    assert lib.slrhip_resolve_clamp(ctx.handle, abi.CLAMP_CLAMPED, dst, pixels, None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_clamp_summary(ctx.handle, C.byref(summary), None) == ERR_INVALID_ARGUMENT
    with pytest.raises(binding.SlrHipError):
        ctx.clamp(abi.CLAMP_CLAMPED)
    # a bad limit, bad flags, nonzero reserved: refused, the clamp stays off
    for d in (abi.ClampDesc(0.0, 0), abi.ClampDesc(-1.0, 0), abi.ClampDesc(float("nan"), 0), abi.ClampDesc(-float("inf"), 0), abi.ClampDesc(1.0, 2),
              abi.ClampDesc(1.0, 0x80000001), abi.ClampDesc(1.0, 0, (1, 0)), abi.ClampDesc(1.0, 0, (0, 1))):
        assert lib.slrhip_clamp_begin(ctx.handle, C.byref(d)) == ERR_INVALID_ARGUMENT
        assert lib.slrhip_clamp_summary(ctx.handle, C.byref(summary), None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_clamp_begin(ctx.handle, None) == ERR_INVALID_ARGUMENT
    ctx.clamp_begin(float(case["limit"]))
    ctx.clamp_begin(float(case["limit"]), False)           # a second call before the first render replaces the first
    # resolve: channel, pointer, size
    for channel in (0, 3, 16, abi.CLAMP_ALL, abi.CLAMP_CLAMPED | abi.CLAMP_LARGEST):
        assert lib.slrhip_resolve_clamp(ctx.handle, channel, dst, pixels, None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_resolve_clamp(ctx.handle, abi.CLAMP_CLAMPED, None, pixels, None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_resolve_clamp(ctx.handle, abi.CLAMP_CLAMPED, dst + 2, pixels, None) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_resolve_clamp(ctx.handle, abi.CLAMP_CLAMPED, dst, pixels - 1, None) == ERR_INVALID_ARGUMENT
    host_dst = np.zeros(pixels, F)
    assert lib.slrhip_read_clamp(ctx.handle, abi.CLAMP_CLAMPED, host_dst.ctypes.data, pixels - 1) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_read_clamp(ctx.handle, abi.CLAMP_CLAMPED, None, pixels) == ERR_INVALID_ARGUMENT
    assert lib.slrhip_clamp_summary(ctx.handle, None, None) == ERR_INVALID_ARGUMENT
    ctx.render(0, 3)
    # after the first render call: refused, the render goes on
    with pytest.raises(binding.SlrHipError):
        ctx.clamp_begin(1.0)
    ctx.render(3, case["passes"] - 3)
    # the context is usable and the refused calls changed nothing; the device resolve (offset by one float: 4-byte alignment) agrees
    got = snapshot(ctx, statistics=False)
    for k in array_keys(got):
        assert_same_bits(got[k], case["got"][k], "after the refused calls: %r" % (k,))
    ctx.clamp_into(abi.CLAMP_REMOVED, dst + 4, pixels)
    ctx.synchronize()
    back = np.empty(pixels, F)
    binding._hip_check(hip.hipMemcpy(back.ctypes.data, dst + 4, back.nbytes, 2), "hipMemcpy")
    hip.hipFree(dst)
    assert_same_bits(back.reshape(st.image_height, st.image_width), case["got"]["clamp", abi.CLAMP_REMOVED], "clamp_into")
