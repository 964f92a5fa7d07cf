"""The primary pass: the camera ray of every sample of a result window is traced by one launch before the
window's iterations, and a slot shades its new sample's first hit in the k_shade launch that starts it.  The comparator is the
same library with SLRHIP_FLAG_NO_PRIMARY_PASS, where a new sample's camera ray goes through the slot state and the traversal
launch of the next iteration.  A sample's contribution is a function of (pixel, pass, seed) alone, so every comparison here is
bit for bit and the counters (samples, extension rays, shadow rays) are equal; slrhip_debug_primary_samples says how many
samples really took their first hit from the pass (all of them when it is on, none when it is off).  The plan keeps the pass off
in spectral contexts and in scenes with an environment light, where it measured slower; those cases are still rendered both ways
(the frames and counters must agree all the same) and the read-out must then be 0 — what the plan says is asked of the plan's own
function (slrhip_debug_primary_plan), never assumed here.

The launch loop of a 64 x 48 frame is the plain one with or without SLRHIP_FLAG_TIME_KERNELS: blocks of iterations are replayed
from a hipGraph only from 2^18 slots on, which 3 072 pixels x 64 stripes do not reach.  The hipGraph loop is therefore compared
on 640 x 480 with two stripes (614 400 slots), the frame of test_graph_replay_and_event_timed_launch_loops_give_the_same_frame."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes

OFF = abi.FLAG_NO_PRIMARY_PASS
MODES = [abi.MODE_RGB, abi.MODE_SPECTRAL]


def render(sc, st, calls, mode=abi.MODE_RGB, stripes=1, flags=0, shard=(0, 1)):
    """frame, (samples, extension rays, shadow rays), iterations, samples started from the primary pass's record"""
    c = Context(mode=mode, stripes=stripes, flags=flags)
    c.upload_scene(sc)
    c.render_begin(st, shard)
    for begin, count in calls:
        c.render(begin, count)
    fb = c.read_framebuffer()
    ctr = c.counters()
    primary = c.primary_samples()
    c.close()
    return fb, (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), int(ctr.iterations), primary


def runs(sc, mode=abi.MODE_RGB, flags=0):
    """Does the plan run the pass for this scene, mode and flags?  It keeps it off in spectral contexts and in scenes with an
    environment light, where it measured slower; "on" is then the old path too, and the read-out must say so."""
    return primary_plan(64, 4, flags, instanced=len(sc.instances) > 0, spectral=mode == abi.MODE_SPECTRAL, environment=sc.env is not None)[0] == 1


def compare(sc, st, calls, what, pixels, **kw):
    """default vs SLRHIP_FLAG_NO_PRIMARY_PASS for one configuration; returns the two iteration counts (default, off)"""
    flags = kw.pop("flags", 0)
    planned = pixels * sum(n for _, n in calls) if runs(sc, kw.get("mode", abi.MODE_RGB), flags) else 0
    on = render(sc, st, calls, flags=flags, **kw)
    off = render(sc, st, calls, flags=flags | OFF, **kw)
    samples = pixels * sum(n for _, n in calls)
    assert on[1] == off[1], (what, on[1], off[1])
    assert on[1][0] == samples, (what, on[1][0], samples)
    assert on[3] == planned and off[3] == 0, (what, on[3], off[3], planned)
    assert_bit_equal(on[0], off[0], "primary pass on vs off: " + what)
    assert on[0].sum() > 0, what
    return on[2], off[2]


@pytest.fixture(scope="module")
def spheres():
    return scenes.cornell_box_spheres(1.0, 16, 8, "glass")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tail", [0, abi.FLAG_TAIL_KERNEL])
@pytest.mark.parametrize("timed", [0, abi.FLAG_TIME_KERNELS])
def test_pass_on_equals_pass_off(spheres, mode, tail, timed):
    """64 x 48: one stripe / 24 passes, 8 stripes / 40 passes, 64 stripes / 16 passes (more slots than passes), and a render
    continued in a second call (24 + 16) — with and without the tail kernel, with plain and with event-timed launches."""
    st = ob.settings(64, 48, seed=21)
    for stripes, calls in ((1, ((0, 24),)), (8, ((0, 40),)), (64, ((0, 16),)), (8, ((0, 24), (24, 16)))):
        what = "mode %d, stripes %d, calls %s, flags %d" % (mode, stripes, calls, tail | timed)
        it_on, it_off = compare(spheres, st, calls, what, 64 * 48, mode=mode, stripes=stripes, flags=tail | timed)
        if stripes == 1 and len(calls) == 1 and runs(spheres, mode):
            # one slot per pixel: every sample but a slot's first saves the iteration its camera ray used to take
            assert it_on < it_off, (what, it_on, it_off)


@pytest.mark.gpu
def test_pass_on_equals_pass_off_in_the_hipgraph_loop():
    """614 400 slots: the blocks of iterations are captured into a hipGraph and replayed (no kernel timing), with a fixed slot
    count and with the automatic one (tail kernel on)."""
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "matte")
    st = ob.settings(640, 480, seed=77)
    for stripes in (2, 0):
        compare(sc, st, ((0, 8),), "hipGraph loop, stripes %d" % stripes, 640 * 480, stripes=stripes)


CASES = [("boxes ggx", lambda: scenes.cornell_box_boxes(1.0), MODES),
         ("multi", lambda: scenes.cornell_multi(1.0, 10, 5), MODES),
         ("textured", lambda: scenes.cornell_textured(1.0, 10, 5), MODES),
         ("instanced", lambda: scenes.cornell_instanced(1.0, 10, 5), MODES),          # the instance plane
         ("ward", lambda: scenes.cornell_lobes("ward", segments=8, rings=4), [abi.MODE_RGB]),
         ("environment light", lambda: scenes.ibl_test_scene(1.0, (64, 32), 8, 4), [abi.MODE_RGB])]      # a class the plan keeps off


@pytest.mark.gpu
@pytest.mark.parametrize("name, make, modes", CASES, ids=[c[0] for c in CASES])
def test_every_shade_kernel_variant_one_stripe(name, make, modes):
    """The scenes of test_tail_kernel_variants_match_the_wavefront_iterations_bit_for_bit (every k_shade / k_tail instantiation),
    48 x 36, 6 passes, one stripe, with the tail kernel (so that k_tail starts samples from records too) and without."""
    sc = make()
    st = ob.settings(48, 36, seed=33)
    for mode in modes:
        for tail in (0, abi.FLAG_TAIL_KERNEL):
            compare(sc, st, ((0, 6),), "%s, mode %d, flags %d" % (name, mode, tail), 48 * 36, mode=mode, stripes=1, flags=tail)


@pytest.mark.gpu
def test_two_rank_shard_split_sums_to_the_unsharded_frame(spheres):
    st = ob.settings(64, 48, seed=21)
    whole = render(spheres, st, ((0, 12),), stripes=4)
    parts = [render(spheres, st, ((0, 12),), stripes=4, shard=(rank, 2)) for rank in range(2)]
    off = [render(spheres, st, ((0, 12),), stripes=4, shard=(rank, 2), flags=OFF) for rank in range(2)]
    for rank in range(2):
        assert parts[rank][1] == off[rank][1], (rank, parts[rank][1], off[rank][1])
        assert parts[rank][3] == parts[rank][1][0] > 0 and off[rank][3] == 0
        assert_bit_equal(parts[rank][0], off[rank][0], "shard %d of 2: primary pass on vs off" % rank)
    assert sum(p[1][0] for p in parts) == whole[1][0] == 64 * 48 * 12
    assert tuple(sum(p[1][k] for p in parts) for k in range(3)) == whole[1]
    assert_bit_equal(parts[0][0] + parts[1][0], whole[0], "two shards vs the unsharded frame")      # disjoint supports: the sum is a gather
    assert whole[0].sum() > 0


@pytest.mark.gpu
def test_adaptive_render_on_equals_off(spheres):
    """Windows over a compact pixel list (slrhip_render_adaptive): the pass takes the window's pixel list and count."""
    st = ob.settings(64, 48, seed=5)
    out = []
    for flags in (0, OFF):
        c = Context(stripes=4, flags=flags)
        c.upload_scene(spheres)
        c.render_begin(st)
        c.statistics_begin()
        done, samples = c.render_adaptive(0, 0.25, 0.05, 4, 4, 24)
        out.append(dict(done=done, samples=samples, frame=c.read_framebuffer(), mean=c.read_framebuffer_mean(), active=c.adaptive_active(),
                        count=c.statistics(abi.STATISTICS_COUNT), counters=tuple(int(v) for v in (c.counters().samples, c.counters().extension_rays,
                                                                                                  c.counters().shadow_rays)),
                        primary=c.primary_samples()))
        c.close()
    on, off = out
    assert (on["done"], on["samples"], on["active"], on["counters"]) == (off["done"], off["samples"], off["active"], off["counters"])
    assert on["counters"][0] == on["samples"] == on["primary"] and off["primary"] == 0
    assert 0 < on["samples"] < 64 * 48 * 24          # some pixels retired: later windows ran over a compact list
    for k in ("frame", "mean", "count"):
        assert_bit_equal(on[k], off[k], "adaptive render, primary pass on vs off: " + k)
    assert on["frame"].sum() > 0


def primary_plan(num_pixels, num_passes, flags=0, instanced=False, spectral=False, environment=False):
    lib = binding.load_library()
    plan = np.zeros(4, np.uint32)
    scene_class = int(instanced) | int(spectral) << 1 | int(environment) << 2
    assert lib.slrhip_debug_primary_plan(num_pixels, num_passes, flags, scene_class, plan.ctypes.data) == 0
    return tuple(int(v) for v in plan)


def test_plan_of_the_primary_pass():
    """render_plan.cpp, planPrimary, on the host: when the pass runs, how its launches stay under 2^31 samples, and that the
    instance plane exists only for instanced scenes."""
    # on by default; off on request, in the counting build's schedule, and for an empty window
    assert primary_plan(64 * 48, 24) == (1, 24, 1, 0)
    assert primary_plan(64 * 48, 24, abi.FLAG_TAIL_KERNEL | abi.FLAG_TIME_KERNELS) == (1, 24, 1, 0)
    assert primary_plan(64 * 48, 24, abi.FLAG_NO_PRIMARY_PASS) == (0, 0, 0, 0)
    assert primary_plan(64 * 48, 24, abi.FLAG_COUNT_TRAVERSAL) == (0, 0, 0, 0)
    assert primary_plan(64 * 48, 0) == (0, 0, 0, 0) and primary_plan(0, 24) == (0, 0, 0, 0)
    # the instance plane
    assert primary_plan(48 * 36, 6, instanced=True) == (1, 6, 1, 1)
    assert primary_plan(48 * 36, 6, abi.FLAG_NO_PRIMARY_PASS, instanced=True) == (0, 0, 0, 0)
    # the two classes where the pass measured slower keep it off
    assert primary_plan(64 * 48, 24, spectral=True) == (0, 0, 0, 0) and primary_plan(64 * 48, 24, environment=True) == (0, 0, 0, 0)
    assert primary_plan(48 * 36, 6, instanced=True, spectral=True) == (0, 0, 0, 0)
    # the headline frame: 1280 x 720 x 1024 = 943 718 400 samples, one launch
    assert primary_plan(1280 * 720, 1024) == (1, 1024, 1, 0)
    # launches of whole passes, each at most 2^31 - 1 samples, together the window
    limit = 2 ** 31 - 1
    for pixels, passes in ((1280 * 720, 4096), (3840 * 2160, 448), (2 ** 31 - 1, 2), (2 ** 30, 3), (2 ** 30 + 1, 3), (limit // 7, 15)):
        on, per, launches, plane = primary_plan(pixels, passes)
        assert on == 1 and plane == 0
        assert 1 <= per <= passes and pixels * per <= limit, (pixels, passes, per)
        assert per == passes or pixels * (per + 1) > limit, (pixels, passes, per)      # as many passes per launch as fit
        assert launches == -(-passes // per), (pixels, passes, per, launches)
    assert primary_plan(2 ** 31, 1) == (0, 0, 0, 0)          # a pass of more pixels than a launch can number: the old path
    assert "slrhip_debug_primary_plan" in binding.EXPORTS and "slrhip_debug_primary_samples" in binding.EXPORTS
    assert binding.load_library().slrhip_debug_primary_samples(None, None) == 1      # no GPU needed to refuse
