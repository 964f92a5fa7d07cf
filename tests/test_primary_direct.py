"""The direct kernel of the primary pass (pt_primary_direct.hip): where a scene has no instances and its tree is not
the quantized one, the lane that traces a camera ray also makes it and stores its record and stream — no producer wave, no ring.  The
comparator is always the same library: the ring kernel (SLRHIP_FLAG_PRIMARY_RING, or `kernel` 0 of slrhip_debug_primary_pass) and the
render without a pass (SLRHIP_FLAG_NO_PRIMARY_PASS).  A record and a stream are functions of (pixel, pass, seed) alone and both
kernels call the same camera, slab, triangle and tie-rule functions, so every comparison is bit for bit; slrhip_debug_primary_kernel
says which kernel a window's pass really ran, so that no test compares a kernel with itself."""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes

RING, OFF = abi.FLAG_PRIMARY_RING, abi.FLAG_NO_PRIMARY_PASS
NONE_K, RING_K, DIRECT_K = 0, 1, 2          # slrhip_debug_primary_kernel
FILL = 0xA5C3F00D                            # what the tests put into the planes before a launch


# ---- the plan, on the host ----------------------------------------------------------------------------------------------------
def kernel_plan(pixels, passes, flags=0, instanced=0, spectral=0, environment=0, quantized=0):
    """(the pass runs, it runs the direct kernel) as the plan's own functions say"""
    lib = binding.load_library()
    scene_class = instanced | spectral << 1 | environment << 2 | quantized << 3
    direct = C.c_uint32(7)
    assert lib.slrhip_debug_primary_kernel_plan(pixels, passes, flags, scene_class, C.byref(direct)) == 0
    plan = np.zeros(4, np.uint32)
    assert lib.slrhip_debug_primary_plan(pixels, passes, flags, scene_class & 7, plan.ctypes.data) == 0
    return int(plan[0]), int(direct.value)


def test_plan_names_the_kernel():
    assert kernel_plan(37 * 19, 65) == (1, 1)                                   # the plain class: direct
    assert kernel_plan(1280 * 720, 1024) == (1, 1)                              # the headline frame
    assert kernel_plan(37 * 19, 65, abi.FLAG_TAIL_KERNEL | abi.FLAG_TIME_KERNELS) == (1, 1)
    assert kernel_plan(37 * 19, 65, instanced=1) == (1, 0)                      # ring
    assert kernel_plan(37 * 19, 65, quantized=1) == (1, 0)
    assert kernel_plan(37 * 19, 65, instanced=1, quantized=1) == (1, 0)
    assert kernel_plan(37 * 19, 65, RING) == (1, 0)                             # the comparator keeps the ring kernel on
    for kw in (dict(spectral=1), dict(environment=1), dict(flags=OFF), dict(flags=abi.FLAG_COUNT_TRAVERSAL), dict(flags=OFF | RING),
               dict(spectral=1, quantized=1), dict(environment=1, instanced=1)):
        assert kernel_plan(37 * 19, 65, **kw) == (0, 0), kw                     # neither: no pass
    assert kernel_plan(0, 65) == (0, 0) and kernel_plan(37 * 19, 0) == (0, 0)
    lib = binding.load_library()
    assert lib.slrhip_debug_primary_kernel_plan(64, 4, 0, 0, None) == 1         # no GPU needed to refuse
    assert lib.slrhip_debug_primary_kernel(None, None) == 1 and lib.slrhip_debug_primary_pass(None, 1, 0, 1, 1, None, None) == 1
    for name in ("slrhip_debug_primary_kernel_plan", "slrhip_debug_primary_kernel", "slrhip_debug_primary_pass"):
        assert name in binding.EXPORTS
    assert abi.FLAG_PRIMARY_RING == 2048


# ---- records and streams, direct against ring -----------------------------------------------------------------------------------
W, H = 37, 19          # n is no multiple of 64 or 256 for most pass counts, and waves straddle pixels


def launch_both(ctx, pixels, first, count, window, with_streams):
    """One launch of each kernel into planes filled with FILL: {kernel: (records, streams or None)} as uint32 [pixels, window, 4]."""
    out = {}
    with binding.DeviceBlocks() as dev:
        fill = np.full((pixels, window, 4), FILL, np.uint32)
        for kernel in (0, 1):
            rec = dev.put(fill)
            rng = dev.put(fill) if with_streams else 0
            ctx.primary_pass(kernel, first, count, window, rec, rng)
            out[kernel] = (dev.get(rec, fill.shape, np.uint32), dev.get(rng, fill.shape, np.uint32) if with_streams else None)
    return out


def check_launch(ctx, pixels, first, count, window, with_streams, what):
    """Both kernels give the same planes, bit for bit; entries outside the launch's passes keep the fill.  Returns the records."""
    got = launch_both(ctx, pixels, first, count, window, with_streams)
    inside = np.zeros((pixels, window), bool)
    inside[:, first:first + count] = True
    for kernel in (0, 1):
        for plane, name in zip(got[kernel], ("records", "streams")):
            if plane is None:
                continue
            assert (plane[~inside] == FILL).all(), "%s: kernel %d wrote %s outside its passes" % (what, kernel, name)
            if name == "streams":
                assert not (plane[inside] == FILL).all(axis=-1).any(), "%s: kernel %d left a stream unwritten" % (what, kernel)
    rec = got[1][0][inside]
    assert not (rec == FILL).all(axis=-1).any(), what + ": a record was left unwritten"
    assert np.array_equal(got[0][0], got[1][0]), "%s: %d records differ" % (what, (got[0][0] != got[1][0]).any(axis=-1).sum())
    if with_streams:
        assert np.array_equal(got[0][1], got[1][1]), "%s: %d streams differ" % (what, (got[0][1] != got[1][1]).any(axis=-1).sum())
    miss = rec[:, 0] == 0xFFFFFFFF
    assert (rec[miss] == np.array([0xFFFFFFFF, 0x7F800000, 0, 0], np.uint32)).all(), what + ": a miss is {none, inf, 0, 0}"
    return rec, miss


def begun(sc, st, shard=(0, 1), flags=0):
    c = Context(stripes=1, flags=flags)
    c.upload_scene(sc)
    c.render_begin(st, shard)
    return c


@pytest.fixture(scope="module")
def spheres():
    return scenes.cornell_box_spheres(1.0, 16, 8, "glass")


@pytest.mark.gpu
@pytest.mark.parametrize("with_streams", [True, False], ids=["streams", "no streams"])
def test_direct_records_and_streams_equal_the_ring_kernels(spheres, with_streams):
    """37 x 19 pixels, 1, 3, 63, 64, 65 and 100 passes as whole windows, and a launch that starts at pass 5 of a window of 100 and takes 37
    of them (primaryLaunchEntry's stride)."""
    ctx = begun(spheres, ob.settings(W, H, seed=11))
    for passes in (1, 3, 63, 64, 65, 100):
        rec, miss = check_launch(ctx, W * H, 0, passes, passes, with_streams, "%d passes" % passes)
        assert not miss.any()              # a closed box
    check_launch(ctx, W * H, 5, 37, 100, with_streams, "passes 5 .. 41 of 100")
    check_launch(ctx, W * H, 64, 64, 128, with_streams, "passes 64 .. 127 of 128")
    ctx.close()


@pytest.mark.gpu
def test_one_rank_of_a_two_rank_split(spheres):
    ctx = begun(spheres, ob.settings(W, H, seed=11), shard=(1, 2))
    ctx.render(0, 1)
    pixels = int(ctx.counters().samples)       # one pass: the rank's pixel list
    assert 0 < pixels < W * H
    check_launch(ctx, pixels, 0, 65, 65, True, "rank 1 of 2, 65 passes")
    check_launch(ctx, pixels, 3, 20, 40, False, "rank 1 of 2, passes 3 .. 22 of 40")
    ctx.close()


@pytest.mark.gpu
def test_rays_that_miss_the_scene():
    """The terrain under an open sky, no environment light: some camera rays leave the scene."""
    ctx = begun(scenes.lattice_terrain(8), ob.settings(W, H, seed=3))
    rec, miss = check_launch(ctx, W * H, 0, 65, 65, True, "open terrain")
    assert miss.any() and (~miss).any(), (int(miss.sum()), len(miss))
    ctx.close()


@pytest.mark.gpu
def test_alpha_textured_scene():
    """The TEX class: alphaPasses runs inside the traversal (the quad in front of the back wall has half of its squares cut away)."""
    ctx = begun(scenes.cornell_textured(1.0, 10, 5), ob.settings(W, H, seed=8))
    check_launch(ctx, W * H, 0, 65, 65, True, "alpha texture")
    check_launch(ctx, W * H, 2, 3, 7, False, "alpha texture, passes 2 .. 4 of 7")
    ctx.close()


def grazing_terrain():
    """lattice_terrain(160): 51 211 triangles, a host-built tree of 19 476 nodes in 10 levels, seen through a thin lens from just above
    its near edge along the ground, so that a camera ray passes many boxes."""
    sc = scenes.lattice_terrain(160)
    m = scenes._translate(80.0, 2.5, -4.0) @ scenes._rotate(0.02, (1, 0, 0))
    sc.camera = scenes.make_camera(m, 1.0, 0.6, 0.05, 1.0, 160.0)
    return sc


@pytest.mark.gpu
def test_deep_host_built_tree_at_a_grazing_angle():
    sc = grazing_terrain()
    ctx = begun(sc, ob.settings(W, H, seed=5))
    ctr = ctx.counters()
    assert ctr.bvh_depth >= 10 and ctr.bvh_nodes < 65536, (ctr.bvh_depth, ctr.bvh_nodes)
    rec, miss = check_launch(ctx, W * H, 0, 65, 65, True, "grazing terrain")
    assert (~miss).any()
    ctx.close()


@pytest.mark.gpu
def test_direct_kernel_is_refused_where_it_cannot_trace():
    for sc in (scenes.cornell_instanced(1.0, 10, 5), scenes.lattice_grid(400)):
        ctx = begun(sc, ob.settings(W, H, seed=5))
        with binding.DeviceBlocks() as dev:
            rec = dev.put(np.full((W * H, 2, 4), FILL, np.uint32))
            with pytest.raises(binding.SlrHipError, match=r"\(5\)"):
                ctx.primary_pass(1, 0, 2, 2, rec)
            assert (dev.get(rec, (W * H, 2, 4), np.uint32) == FILL).all()
            ctx.primary_pass(0, 0, 2, 2, rec)                   # the ring kernel traces it
            assert not (dev.get(rec, (W * H, 2, 4), np.uint32) == FILL).all(axis=-1).any()
            for bad in ((2, 0, 2, 2), (1, 0, 0, 2), (1, 1, 2, 2)):
                with pytest.raises(binding.SlrHipError, match=r"\(1\)"):
                    ctx.primary_pass(*bad, rec)
        ctx.close()


# ---- frames ---------------------------------------------------------------------------------------------------------------------
def frame(sc, st, calls, flags=0, stripes=1, mode=abi.MODE_RGB, adaptive=False):
    c = Context(mode=mode, stripes=stripes, flags=flags)
    c.upload_scene(sc)
    c.render_begin(st)
    extra = None
    if adaptive:
        c.statistics_begin()
        extra = c.render_adaptive(0, 0.25, 0.05, 4, 4, 24)
    else:
        for begin, count in calls:
            c.render(begin, count)
    ctr = c.counters()
    out = dict(fb=c.read_framebuffer(), counters=(int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), primary=c.primary_samples(),
               kernel=c.primary_kernel(), extra=extra)
    c.close()
    return out


def three_ways(sc, st, calls, what, flags=0, **kw):
    """default (direct), PRIMARY_RING and NO_PRIMARY_PASS: equal frames and counters; the read-outs say direct, ring and none."""
    d, r, o = (frame(sc, st, calls, flags=flags | f, **kw) for f in (0, RING, OFF))
    assert (d["kernel"], r["kernel"], o["kernel"]) == (DIRECT_K, RING_K, NONE_K), (what, d["kernel"], r["kernel"], o["kernel"])
    assert d["counters"] == r["counters"] == o["counters"], (what, d["counters"], r["counters"], o["counters"])
    assert d["extra"] == r["extra"] == o["extra"], what
    assert d["primary"] == r["primary"] == d["counters"][0] > 0 and o["primary"] == 0, (what, d["primary"], r["primary"], o["primary"])
    assert_bit_equal(d["fb"], r["fb"], what + ": direct vs ring")
    assert_bit_equal(d["fb"], o["fb"], what + ": direct vs no primary pass")
    assert d["fb"].sum() > 0, what
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(48, 36), (36, 20)], ids=["48x36", "36x20"])
@pytest.mark.parametrize("passes", [1, 64, 65, 100])
def test_frames_direct_ring_and_no_pass(spheres, size, passes):
    st = ob.settings(size[0], size[1], seed=21)
    d = three_ways(spheres, st, ((0, passes),), "%dx%d, %d passes, one stripe" % (size + (passes,)), stripes=1)
    assert d["counters"][0] == size[0] * size[1] * passes


@pytest.mark.gpu
@pytest.mark.parametrize("stripes, flags", [(64, 0), (0, 0), (1, abi.FLAG_TAIL_KERNEL), (64, abi.FLAG_TIME_KERNELS), (0, abi.FLAG_TIME_KERNELS)],
                         ids=["64 stripes", "automatic", "tail kernel", "timed, 64 stripes", "timed, automatic"])
def test_frames_with_other_slot_counts_and_launch_loops(spheres, stripes, flags):
    st = ob.settings(36, 20, seed=22)
    three_ways(spheres, st, ((0, 65),), "36x20, 65 passes, stripes %d, flags %d" % (stripes, flags), stripes=stripes, flags=flags)


@pytest.mark.gpu
def test_render_continued_in_a_second_call(spheres):
    st = ob.settings(48, 36, seed=23)
    d = three_ways(spheres, st, ((0, 24), (24, 41)), "24 + 41 passes", stripes=8)
    assert_bit_equal(d["fb"], frame(spheres, st, ((0, 65),), stripes=8)["fb"], "two calls vs one")


@pytest.mark.gpu
def test_adaptive_render(spheres):
    st = ob.settings(48, 36, seed=5)
    d = three_ways(spheres, st, (), "adaptive", stripes=4, adaptive=True)
    assert 0 < d["extra"][1] < 48 * 36 * 24          # some pixels retired: later windows ran over a compact list


@pytest.mark.gpu
def test_hipgraph_loop():
    """640 x 480 with two stripes: 614 400 slots, the smallest frame whose blocks of iterations are replayed from a hipGraph."""
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "matte")
    three_ways(sc, ob.settings(640, 480, seed=77), ((0, 4),), "hipGraph loop", stripes=2)


# ---- classes that must not change -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name, make, mode, kernel",
                         [("instanced", lambda: scenes.cornell_instanced(1.0, 10, 5), abi.MODE_RGB, RING_K),
                          ("quantized", lambda: scenes.displaced_grid(400, 4.0 / 3.0), abi.MODE_RGB, RING_K),
                          ("spectral", lambda: scenes.cornell_box_boxes(1.0), abi.MODE_SPECTRAL, NONE_K),
                          ("environment", lambda: scenes.ibl_test_scene(1.0, (64, 32), 8, 4), abi.MODE_RGB, NONE_K)],
                         ids=["instanced", "quantized", "spectral", "environment"])
def test_other_scene_classes_keep_their_kernel(name, make, mode, kernel):
    sc = make()
    st = ob.settings(48, 36, seed=33)
    d, r, o = (frame(sc, st, ((0, 6),), flags=f, mode=mode) for f in (0, RING, OFF))
    assert (d["kernel"], r["kernel"], o["kernel"]) == (kernel, kernel, NONE_K), (name, d["kernel"], r["kernel"], o["kernel"])
    assert d["counters"] == r["counters"] == o["counters"], name
    assert d["primary"] == r["primary"] == (d["counters"][0] if kernel else 0) and o["primary"] == 0, name
    assert_bit_equal(d["fb"], o["fb"], name + ": default vs no primary pass")
    assert_bit_equal(r["fb"], o["fb"], name + ": PRIMARY_RING vs no primary pass")
    assert d["fb"].sum() > 0
