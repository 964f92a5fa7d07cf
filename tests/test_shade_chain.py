"""The fused start of k_shade takes a sample's stream from the primary pass: the pass's producer draws the camera
sample anyway, so it leaves the xorshift128 state behind the draws in a plane beside the result window (PathBuffers::primaryRng),
and the launch that starts the sample rebuilds the draws from that state (recoverCameraDraws, pt_camera.h) instead of seeding the
stream again.  Nothing of the arithmetic changes, so every comparison is bit for bit, against the same library with
SLRHIP_FLAG_NO_PRIMARY_PASS (the comparator of test_primary_pass.py): frames, the three counters, and the number of samples that
started from the pass (all of them where the plan runs it, none elsewhere).  Where the plan keeps the pass off the plane must not
be bound: slrhip_debug_primary_stream_entries, the size of what the window bound, says 0.  It says 0 as well in instanced scenes (and on
large, quantized trees), where the pass runs but its producer wave is the limit and the plan keeps the plane off: the fused start
seeds its own stream there, and the frames must agree all the same.

Shapes: 48 x 36 and 36 x 20 pixels (partial 8 x 8 tiles; 720 pixels are no multiple of a 256-thread block); passes 1, 3, 63, 64,
65 and 100 (runs of 64, the run-length fallback of odd counts, a wave's items spanning two pixels); 1, 64 and automatic stripes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes
from test_primary_pass import CASES, OFF, primary_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(48, 36), (36, 20)]
PASSES = (1, 3, 63, 64, 65, 100)
STRIPES = (1, 64, 0)


def render(sc, st, calls, mode=abi.MODE_RGB, stripes=1, flags=0, shard=(0, 1)):
    """frame, (samples, extension rays, shadow rays), samples started from the pass, entries of the stream plane of the last window"""
    c = Context(mode=mode, stripes=stripes, flags=flags)
    c.upload_scene(sc)
    c.render_begin(st, shard)
    for begin, count in calls:
        c.render(begin, count)
    fb = c.read_framebuffer()
    ctr = c.counters()
    out = fb, (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), c.primary_samples(), c.primary_stream_entries()
    c.close()
    return out


def runs(sc, mode, flags):
    return primary_plan(64, 4, flags, instanced=len(sc.instances) > 0, spectral=mode == abi.MODE_SPECTRAL, environment=sc.env is not None)[0] == 1


def last_window(passes):
    """Passes of the last result window of a call (render_plan.cpp, planWindows, far below the byte budget): a call of 64 passes and
    more is rendered in windows of whole runs of 64, and what is left over in a window of its own (65 = 64 + 1, 100 = 64 + 36)."""
    window = passes - passes % 64 if passes >= 64 else passes
    return passes - (passes - 1) // window * window


def test_last_window():
    assert [last_window(n) for n in (1, 3, 63, 64, 65, 100, 128, 129)] == [1, 3, 63, 64, 1, 36, 128, 1]


def compare(sc, st, calls, what, pixels, mode=abi.MODE_RGB, stripes=1, flags=0, shard=(0, 1)):
    on = render(sc, st, calls, mode, stripes, flags, shard)
    off = render(sc, st, calls, mode, stripes, flags | OFF, shard)
    samples = pixels * sum(n for _, n in calls)
    planned = runs(sc, mode, flags)
    plane = planned and len(sc.instances) == 0      # instanced scenes (and large trees) run the pass without the plane: render_plan.h
    assert on[1] == off[1], (what, on[1], off[1])
    assert on[1][0] == samples, (what, on[1][0], samples)
    assert on[2] == (samples if planned else 0) and off[2] == 0, (what, on[2], off[2])
    # the plane of the call's last window has an entry per sample of that window
    assert on[3] == (pixels * last_window(calls[-1][1]) if plane else 0) and off[3] == 0, (what, on[3], off[3])
    assert_bit_equal(on[0], off[0], "streams from the primary pass vs seeded starts: " + what)
    assert on[0].sum() > 0, what


@pytest.fixture(scope="module")
def spheres():
    return scenes.cornell_box_spheres(1.0, 8, 4, "glass")


def test_plan_of_the_stream_plane():
    """render_plan.cpp, planPrimary, on the host: the plane has an entry per sample of the window where the pass runs three consumers per
    producer — no instances, no quantized tree — and none where the pass is off or its producer is the limit."""
    import ctypes as C
    lib = binding.load_library()

    def entries(pixels, passes, flags=0, instanced=0, spectral=0, environment=0, quantized=0):
        n = C.c_uint64(99)
        assert lib.slrhip_debug_primary_stream_plan(pixels, passes, flags, instanced | spectral << 1 | environment << 2 | quantized << 3, C.byref(n)) == 0
        return n.value

    assert entries(48 * 36, 6) == 48 * 36 * 6 and entries(1280 * 720, 1024) == 1280 * 720 * 1024
    assert entries(640 * 480, 1) == 640 * 480            # whatever the window budget made of the call
    assert entries(48 * 36, 6, instanced=1) == 0 and entries(48 * 36, 6, quantized=1) == 0 and entries(48 * 36, 6, instanced=1, quantized=1) == 0
    assert primary_plan(48 * 36, 6, instanced=True)[0] == 1          # ... where the pass itself stays on
    assert entries(48 * 36, 6, spectral=1) == 0 and entries(48 * 36, 6, environment=1) == 0
    assert entries(48 * 36, 6, abi.FLAG_NO_PRIMARY_PASS) == 0 and entries(48 * 36, 6, abi.FLAG_COUNT_TRAVERSAL) == 0
    assert entries(0, 6) == 0 and entries(48 * 36, 0) == 0
    assert lib.slrhip_debug_primary_stream_plan(1, 1, 0, 0, None) == 1


# ---- recoverCameraDraws ----------------------------------------------------------------------------------------------------------
def test_exports():
    lib = binding.load_library()
    for name in ("slrhip_debug_primary_entries", "slrhip_debug_primary_stream_entries", "slrhip_debug_primary_stream_plan", "slrhip_debug_camera_draws"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    assert lib.slrhip_debug_primary_stream_entries(None, None) == 1 and lib.slrhip_debug_camera_draws(0, 1, None, None) == 1


@pytest.mark.gpu
def test_draws_recovered_from_the_stream_are_the_forward_draws():
    """65 536 (seed, x, y, pass) tuples: the corners of every argument's range crossed with each other, the rest random.  Integer
    operations and one conversion: all six draws equal in every bit; no stream is the all-zero state, and the draws lie where draws lie."""
    n = 65536
    rng = np.random.default_rng(2718)
    t = np.empty((n, 4), np.uint32)
    t[:, 0] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    t[:, 1] = rng.integers(0, 65536, n)
    t[:, 2] = rng.integers(0, 65536, n)
    t[:, 3] = rng.integers(0, 2 ** 32, n, dtype=np.uint64)
    corners = [(s, x, y, p) for s in (0, 0xFFFFFFFF, 0x80000000, 1) for x in (0, 65535) for y in (0, 65535) for p in (0, 0xFFFFFFFF, 1)]
    t[:len(corners)] = np.array(corners, np.uint64).astype(np.uint32)
    out = np.zeros((n, 16), np.uint32)
    assert binding.load_library().slrhip_debug_camera_draws(0, n, t.ctypes.data, out.ctypes.data) == 0
    forward, stream, recovered = out[:, 0:6], out[:, 6:10], out[:, 10:16]
    bad = np.nonzero((forward != recovered).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], t[bad[:8]], forward[bad[:8]], recovered[bad[:8]])
    assert (stream != 0).any(axis=1).all()
    f = forward.view(np.float32)
    assert ((f[:, 0] >= t[:, 1]) & (f[:, 0] <= t[:, 1] + 1.0)).all() and ((f[:, 1] >= t[:, 2]) & (f[:, 1] <= t[:, 2] + 1.0)).all()
    assert ((f[:, 2:] >= 0) & (f[:, 2:] < 1)).all()


# ---- the entry of a launch's sample -----------------------------------------------------------------------------------------------
def test_entries_of_a_launch_of_the_primary_pass():
    """primaryLaunchEntry on the host, against pixel x P + first + pass: launches of the whole window and of a part of it (what a
    window of 2^31 samples and more is cut into)."""
    lib = binding.load_library()
    for pixels, window, first, passes in ((720, 100, 0, 100), (720, 100, 0, 37), (720, 100, 37, 37), (720, 100, 74, 26), (1, 65, 64, 1),
                                          (1728, 1, 0, 1), (5, 7, 6, 1), (3, 64, 1, 63)):
        got = np.zeros(pixels * passes, np.uint64)
        assert lib.slrhip_debug_primary_entries(pixels, first, passes, window, got.ctypes.data) == 0
        pix, p = np.divmod(np.arange(pixels * passes, dtype=np.uint64), np.uint64(passes))
        assert (got == pix * np.uint64(window) + np.uint64(first) + p).all(), (pixels, window, first, passes)
        assert got.max() < pixels * window and len(np.unique(got)) == got.size
    got = np.zeros(4, np.uint64)
    assert lib.slrhip_debug_primary_entries(2, 3, 2, 4, got.ctypes.data) == 1      # passes outside the window
    assert lib.slrhip_debug_primary_entries(2, 0, 0, 4, got.ctypes.data) == 1 and lib.slrhip_debug_primary_entries(2, 0, 2, 4, None) == 1


# ---- small frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("passes", PASSES)
@pytest.mark.parametrize("size", SIZES, ids=["48x36", "36x20"])
def test_pass_counts_and_stripes(spheres, size, passes):
    st = ob.settings(size[0], size[1], seed=21)
    for stripes in STRIPES:
        compare(spheres, st, ((0, passes),), "%dx%d, %d passes, stripes %d" % (size + (passes, stripes)), size[0] * size[1], stripes=stripes)


@pytest.mark.gpu
@pytest.mark.parametrize("timed", [0, abi.FLAG_TIME_KERNELS], ids=["plain", "timed"])
@pytest.mark.parametrize("tail", [0, abi.FLAG_TAIL_KERNEL], ids=["wavefront", "tail"])
@pytest.mark.parametrize("size", SIZES, ids=["48x36", "36x20"])
def test_launch_loops_tail_kernel_and_a_continued_render(spheres, size, tail, timed):
    st = ob.settings(size[0], size[1], seed=22)
    for stripes, calls in ((1, ((0, 65),)), (64, ((0, 3),)), (0, ((0, 64),)), (8, ((0, 24), (24, 16)))):
        what = "%dx%d, stripes %d, calls %s, flags %d" % (size + (stripes, calls, tail | timed))
        compare(spheres, st, calls, what, size[0] * size[1], stripes=stripes, flags=tail | timed)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=["48x36", "36x20"])
def test_two_rank_shard_split(spheres, size):
    st = ob.settings(size[0], size[1], seed=23)
    whole = render(spheres, st, ((0, 12),), stripes=4)
    total = [0, 0, 0]
    frame = np.zeros_like(whole[0])
    for rank in range(2):
        on = render(spheres, st, ((0, 12),), stripes=4, shard=(rank, 2))
        off = render(spheres, st, ((0, 12),), stripes=4, shard=(rank, 2), flags=OFF)
        assert on[1] == off[1] and on[2] == on[1][0] > 0 and off[2] == 0, (rank, on[1:], off[1:])
        assert on[3] == on[1][0] and off[3] == 0, (rank, on[3], off[3])          # the shard's pixels x passes
        assert_bit_equal(on[0], off[0], "shard %d of 2" % rank)
        total = [a + b for a, b in zip(total, on[1])]
        frame += on[0]
    assert tuple(total) == whole[1] and whole[1][0] == size[0] * size[1] * 12
    assert_bit_equal(frame, whole[0], "two shards vs the unsharded frame")      # disjoint supports: the sum is a gather
    assert whole[0].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=["48x36", "36x20"])
def test_adaptive_render(spheres, size):
    """Windows over a compact pixel list: the plane is indexed by the list's pixels like the window."""
    st = ob.settings(size[0], size[1], seed=5)
    out = []
    for flags in (0, OFF):
        c = Context(stripes=4, flags=flags)
        c.upload_scene(spheres)
        c.render_begin(st)
        c.statistics_begin()
        done, samples = c.render_adaptive(0, 0.25, 0.05, 4, 4, 24)
        ctr = c.counters()
        out.append(dict(done=done, samples=samples, frame=c.read_framebuffer(), mean=c.read_framebuffer_mean(), active=c.adaptive_active(),
                        count=c.statistics(abi.STATISTICS_COUNT), counters=(int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)),
                        primary=c.primary_samples(), entries=c.primary_stream_entries()))
        c.close()
    on, off = out
    assert (on["done"], on["samples"], on["active"], on["counters"]) == (off["done"], off["samples"], off["active"], off["counters"])
    assert on["counters"][0] == on["samples"] == on["primary"] and off["primary"] == 0
    assert 0 < on["samples"] < size[0] * size[1] * 24          # some pixels retired: later windows ran over a compact list
    assert 0 < on["entries"] <= size[0] * size[1] * 4 and on["entries"] % 4 == 0 and off["entries"] == 0
    for k in ("frame", "mean", "count"):
        assert_bit_equal(on[k], off[k], "adaptive render: " + k)
    assert on["frame"].sum() > 0


# ---- several windows per call -----------------------------------------------------------------------------------------------------
WINDOWS = dict(width=160, height=120, passes=20, seed=7)
CHILD = """
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import test_shade_chain as t
frame, entries = t.windows_frame(t.%(cfg)s)
np.save(sys.argv[1], frame)
np.save(sys.argv[2], np.array([entries], np.uint64))
"""


def windows_frame(cfg):
    ctx = Context(stripes=1)
    fb = ctx.render_image(scenes.cornell_box_spheres(cfg["width"] / cfg["height"], 8, 4, "matte"), ob.settings(cfg["width"], cfg["height"], seed=cfg["seed"]),
                          cfg["passes"])
    pixels = cfg["width"] * cfg["height"]
    assert int(ctx.counters().samples) == ctx.primary_samples() == pixels * cfg["passes"]
    entries = ctx.primary_stream_entries()
    ctx.close()
    return fb, entries


@pytest.mark.gpu
def test_windows_of_unequal_length(tmp_path):
    """160 x 120 pixels, 20 passes, a window budget of 1 MiB in a fresh child (the variable is read once per process): windows of 3
    passes and a last one of 2, each with its own P in the index of the plane.  The child's frame is this process's."""
    cfg = WINDOWS
    pixels = cfg["width"] * cfg["height"]
    assert pixels * 16 * 4 > (1 << 20) > pixels * 16 * 3 and cfg["passes"] % 3 == 2
    env = dict(os.environ, SLRHIP_RESULT_WINDOW_MB="1")
    out, count = str(tmp_path / "child.npy"), str(tmp_path / "entries.npy")
    child = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), cfg="WINDOWS"), out, count], env=env)
    try:
        whole, entries = windows_frame(cfg)
    finally:
        assert child.wait(timeout=120) == 0
    assert entries == pixels * cfg["passes"] and int(np.load(count)[0]) == pixels * 2      # the last window: one of 20, one of 2 passes
    assert_bit_equal(np.load(out), whole, "result windows of 1 MiB (child process) vs one window")
    assert whole.sum() > 0


ONE_PASS_OVER_BUDGET = dict(width=640, height=480, passes=3, seed=9)


@pytest.mark.gpu
def test_a_single_pass_larger_than_the_window_budget(tmp_path):
    """640 x 480 pixels: one pass is 4.7 MiB of RGB results, more than a budget of 1 MiB.  The plan renders windows of one pass each all
    the same (planWindows: at least one pass), over the budget, and the plane of such a window is as large as its results: the call
    must not fail, and the child's frame is this process's single window."""
    cfg = ONE_PASS_OVER_BUDGET
    pixels = cfg["width"] * cfg["height"]
    assert pixels * 16 > (1 << 20)
    env = dict(os.environ, SLRHIP_RESULT_WINDOW_MB="1")
    out, count = str(tmp_path / "child.npy"), str(tmp_path / "entries.npy")
    child = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests"), cfg="ONE_PASS_OVER_BUDGET"), out, count],
                             env=env)
    try:
        whole, entries = windows_frame(cfg)
    finally:
        assert child.wait(timeout=120) == 0
    assert entries == pixels * cfg["passes"] and int(np.load(count)[0]) == pixels      # windows of one pass
    assert_bit_equal(np.load(out), whole, "one pass per window, each over the budget (child process) vs one window")
    assert whole.sum() > 0


# ---- every instantiation with a fused start, and the classes without the pass -----------------------------------------------------------
VARIANTS = [(name, make, abi.MODE_RGB) for name, make, _ in CASES] + [("boxes ggx spectral", CASES[0][1], abi.MODE_SPECTRAL)]


@pytest.mark.gpu
@pytest.mark.parametrize("name, make, mode", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_every_kernel_with_a_fused_start(name, make, mode):
    """The scenes of test_every_shade_kernel_variant_one_stripe, 48 x 36, 6 passes, one stripe, with and without the tail kernel; the
    instanced scene runs the pass with its instance plane and without the stream plane (the seeded twin of the kernel).  The spectral
    context and the scene with an environment light keep the pass off: compare() asks that no sample started from it and that no
    plane was bound."""
    sc = make()
    st = ob.settings(48, 36, seed=33)
    assert runs(sc, mode, 0) == (mode == abi.MODE_RGB and sc.env is None)
    for tail in (0, abi.FLAG_TAIL_KERNEL):
        compare(sc, st, ((0, 6),), "%s, flags %d" % (name, tail), 48 * 36, mode=mode, stripes=1, flags=tail)


@pytest.mark.gpu
def test_hipgraph_loop():
    """614 400 slots: the blocks of iterations are captured into a hipGraph and replayed."""
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "matte")
    compare(sc, ob.settings(640, 480, seed=77), ((0, 8),), "hipGraph loop, stripes 2", 640 * 480, stripes=2)
