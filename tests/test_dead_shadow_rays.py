"""k_shade's RGB kernels trace no shadow ray whose light sample decides nothing.

A light sample is DEAD when every component of its contribution is a zero of either sign AND the compensated add of it would leave the
path's Kahan pair (sum, compensation) bit for bit as it is.  The second half is not a formality: adding zero through kahanAdd computes
sum + (-compensation), which moves the sum where the compensation sits on a rounding boundary of it.  The first test finds such pairs
with a float32 model of the add; the device predicate (slrhip_debug_dead_light_samples: the function logicSlot decides with) must call
them "not dead".

A dead sample is counted (slrhip_counters::shadow_rays stays "rays the algorithm casts"; slrhip_debug_shadow_skipped says how many of
them were not traced) and otherwise leaves nothing that is read: no pending sample, no queue entry, no flag bit.  The comparator is
the same library with SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS: frames in every bit, and the three counters.

Shapes: the 12-triangle box at 48 x 36 (1 728 slots at one stripe: six full workgroups and one of 192; partial 8 x 8 tiles) with 1 pass
(every lane starts, most paths end at once) and 65 passes (two windows, the second of one pass), 1, 64 and automatic stripes; the
Cornell spheres at 64 x 36 with 64 passes (a whole run per wave); every kernel family (glossy, MultiBSDF, textured, instanced) small;
640 x 480 for the two launch loops."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes
from test_primary_pass import CASES, OFF
from test_shade_occupancy import HIPCC, resource_remarks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = abi.FLAG_TRACE_ALL_SHADOW_RAYS
F = np.float32


# ---- the add, on the host ---------------------------------------------------------------------------------------------------------
def kahan_add(r, c, v):
    """BasicTypes/CompensatedSum.h:24-30 in float32, operation by operation (pt_device.h, kahanAdd)."""
    r, c, v = F(r), F(c), F(v)
    c_input = v - c
    sum_temp = r + c_input
    return sum_temp, (sum_temp - r) - c_input


def bits(x):
    return np.asarray(x, F).view(np.uint32)


def moved_by_zero(r, c):
    """True where adding +0 to the pair (r, c) changes a bit of it."""
    r2, c2 = kahan_add(r, c, np.zeros_like(r))
    return (bits(r2) != bits(r)) | (bits(c2) != bits(c))


@functools.lru_cache(maxsize=None)
def boundary_pairs(count=4096, seed=20260131):
    """(r, c) next to a binade boundary of r, with |c| between a quarter and a half ulp of r — where a Kahan compensation lives.  At
    r = 2^k the floats below r are half as far apart as those above, so r - c rounds to the float below r although |c| is under half
    an ulp of r; a few ulps to either side the same c is absorbed."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-12, 12, count)
    steps = rng.integers(-2, 3, count)                       # ulps of r away from 2^k (below it: half ulps)
    r = np.ldexp(F(1.0), k).astype(F)
    for _ in range(2):
        r = np.where(steps > 0, np.nextafter(r, F(np.inf)), np.where(steps < 0, np.nextafter(r, F(0.0)), r)).astype(F)
        steps = steps - np.sign(steps)
    ulp = (np.nextafter(r, F(np.inf)) - r).astype(F)
    c = (ulp * rng.uniform(0.25, 0.5, count).astype(F) * rng.choice(np.array([-1.0, 1.0], F), count)).astype(F)
    return r, c


def test_adding_zero_is_not_the_identity_of_the_compensated_sum():
    r, c = boundary_pairs()
    moved = moved_by_zero(r, c)
    print("adding +0 moves %d of %d sampled pairs" % (moved.sum(), moved.size))
    assert moved.sum() >= 8, "adding +0 moved only %d of %d sampled pairs" % (moved.sum(), moved.size)
    assert (~moved).sum() >= 8                               # ... and the sample has the other kind too
    # the arithmetic of one of them, spelled out: r = 1, c = 3/8 ulp(1): 1 - c lies nearer to 1 - ulp / 2 than to 1
    one, comp = F(1.0), F(0.375 * 2.0 ** -23)
    r2, c2 = kahan_add(one, comp, F(0.0))
    assert r2 == np.nextafter(one, F(0.0)) and c2 != comp


def test_exports_and_flag():
    lib = binding.load_library()
    for name in ("slrhip_debug_shadow_skipped", "slrhip_debug_dead_light_samples"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    assert lib.slrhip_debug_shadow_skipped(None, None) == 1 and lib.slrhip_debug_dead_light_samples(0, 1, None, None) == 1
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert int(re.search(r"#define SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS (\d+)u", header).group(1)) == ALL == 4096


# ---- the predicate, on the device -------------------------------------------------------------------------------------------------
def device_dead(r, c, contrib):
    """slrhip_debug_dead_light_samples on [n, 3] arrays."""
    triples = np.ascontiguousarray(np.concatenate([np.asarray(x, F).reshape(-1, 3) for x in (r, c, contrib)], axis=1))
    dead = np.full(len(triples), 7, np.uint32)
    lib = binding.load_library()
    assert lib.slrhip_debug_dead_light_samples(0, len(triples), triples.ctypes.data, dead.ctypes.data) == 0
    assert ((dead == 0) | (dead == 1)).all()
    return dead == 1


def model_dead(r, c, contrib):
    r, c, contrib = (np.asarray(x, F).reshape(-1, 3) for x in (r, c, contrib))
    zero = ((bits(contrib) << np.uint32(1)) == 0).all(axis=1)
    r2, c2 = kahan_add(r, c, contrib)
    return zero & (bits(r2) == bits(r)).all(axis=1) & (bits(c2) == bits(c)).all(axis=1)


@pytest.mark.gpu
def test_predicate_on_pairs_that_zero_moves():
    r, c = boundary_pairs()
    moved = moved_by_zero(r, c)
    r, c = r[moved], c[moved]
    assert len(r) >= 8
    # the pair that moves sits in each of the three components in turn; the other two are pairs that zero leaves alone
    for comp in range(3):
        r3, c3 = np.full((len(r), 3), 0.5, F), np.zeros((len(r), 3), F)
        r3[:, comp], c3[:, comp] = r, c
        for zero in (0.0, -0.0):
            contrib = np.full((len(r), 3), zero, F)
            want = model_dead(r3, c3, contrib)
            if zero == 0.0:
                assert not want.any()
            got = device_dead(r3, c3, contrib)
            assert (got == want).all(), (comp, zero, int((got != want).sum()))


@pytest.mark.gpu
def test_predicate_on_ordinary_pairs_and_zeros():
    rng = np.random.default_rng(5)
    n = 4096
    r = rng.uniform(0.0, 8.0, (n, 3)).astype(F)
    ulp = (np.nextafter(r, F(np.inf)) - r).astype(F)
    c = (ulp * rng.uniform(-0.2, 0.2, (n, 3)).astype(F)).astype(F)          # well inside the rounding interval of r
    signs = np.array([[0.0 if s >> k & 1 else -0.0 for k in range(3)] for s in range(8)], F)
    contrib = signs[rng.integers(0, 8, n)]
    assert model_dead(r, c, contrib).all()
    assert device_dead(r, c, contrib).all()
    # a path that has gathered nothing: r = c = 0, every sign pattern of the zero
    assert device_dead(np.zeros((8, 3), F), np.zeros((8, 3), F), signs).all()
    # the boundary sample, whole: the device agrees with the model pair by pair
    rb, cb = boundary_pairs()
    rb3, cb3 = np.stack([rb, rb[::-1], np.roll(rb, 1)], axis=1), np.stack([cb, cb[::-1], np.roll(cb, 1)], axis=1)
    z = np.zeros_like(rb3)
    want = model_dead(rb3, cb3, z)
    assert want.any() and (~want).any()
    assert (device_dead(rb3, cb3, z) == want).all()


@pytest.mark.gpu
def test_predicate_refuses_what_is_not_a_zero():
    specials = [np.nan, -np.nan, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, 1.1754944e-38, 1e-30, 1.0, -1.0]
    rows = []
    for v in specials:
        for comp in range(3):
            for other in (0.0, -0.0):
                row = [other] * 3
                row[comp] = v
                rows.append(row)
    contrib = np.array(rows, F)
    assert ((bits(contrib) << np.uint32(1)) != 0).any(axis=1).all()         # every row has a component that is no zero
    for r, c in ((0.0, 0.0), (0.5, 0.0), (3.0, 1e-9)):
        got = device_dead(np.full(contrib.shape, r, F), np.full(contrib.shape, c, F), contrib)
        assert not got.any(), (r, c, contrib[got])


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def render(sc, st, calls, stripes=1, flags=0):
    """frame, (samples, extension rays, shadow rays), light samples not traced"""
    c = Context(mode=abi.MODE_RGB, stripes=stripes, flags=flags)
    c.upload_scene(sc)
    c.render_begin(st)
    for begin, count in calls:
        c.render(begin, count)
    fb = c.read_framebuffer()
    ctr = c.counters()
    out = fb, (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), c.shadow_skipped()
    c.close()
    return out


def compare(sc, st, calls, what, pixels, stripes=1, flags=0, lit=True):
    """test_shade_chain.compare with this change's comparator: default against SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS."""
    skip = render(sc, st, calls, stripes, flags)
    full = render(sc, st, calls, stripes, flags | ALL)
    print("%s: counters %s, not traced %d (%.1f %% of the shadow rays)" % (what, skip[1], skip[2], 100.0 * skip[2] / max(skip[1][2], 1)))
    assert skip[1] == full[1], (what, skip[1], full[1])
    assert skip[1][0] == pixels * sum(n for _, n in calls), (what, skip[1][0])
    assert full[2] == 0 and 0 <= skip[2] <= skip[1][2], (what, skip[2], full[2])
    assert_bit_equal(skip[0], full[0], "dead light samples not traced vs every shadow ray traced: " + what)
    if lit:
        assert skip[0].sum() > 0, what
    return skip, full


@pytest.mark.gpu
@pytest.mark.parametrize("primary", [0, OFF], ids=["primary-pass", "no-primary-pass"])
@pytest.mark.parametrize("passes", (1, 65))
def test_box(passes, primary):
    sc = scenes.tiny_box(48 / 36)
    for stripes in (1, 64, 0):
        skip, _ = compare(sc, ob.settings(48, 36, seed=51), ((0, passes),), "box, %d passes, stripes %d, flags %d" % (passes, stripes, primary),
                          48 * 36, stripes=stripes, flags=primary)
        # the ceiling, a sixth of what the camera sees, is behind the light's emitting side.  (With the automatic slot count the tail kernel
        # takes a frame this small over at once, and it traces its shadow rays inline, every one: no figure is asked there.)
        assert skip[2] > 0 or stripes == 0


@pytest.mark.gpu
@pytest.mark.parametrize("primary", [0, OFF], ids=["primary-pass", "no-primary-pass"])
def test_cornell_spheres(primary):
    sc = scenes.cornell_box_spheres(64 / 36, 8, 4, "matte")
    for stripes in (1, 0):
        skip, _ = compare(sc, ob.settings(64, 36, seed=52), ((0, 64),), "spheres, stripes %d, flags %d" % (stripes, primary), 64 * 36,
                          stripes=stripes, flags=primary)
        assert skip[2] > 0 or stripes == 0


FAMILIES = [(name, make) for name, make, _ in CASES if name != "environment light"]


@pytest.mark.gpu
@pytest.mark.parametrize("name, make", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_every_rgb_kernel_family(name, make):
    """Glossy lobes, MultiBSDF, textures, instances (the seeded twin), Ward: 48 x 36, 6 passes, with and without the primary pass and the
    tail kernel."""
    sc = make()
    for flags in (0, OFF, abi.FLAG_TAIL_KERNEL):
        skip, _ = compare(sc, ob.settings(48, 36, seed=53), ((0, 6),), "%s, flags %d" % (name, flags), 48 * 36, flags=flags)
        assert skip[2] > 0 or flags == abi.FLAG_TAIL_KERNEL


@pytest.mark.gpu
def test_environment_light_and_counting_contexts():
    """An environment light's sample is never seen from behind, yet below the horizon of the shading point it is dead as any other.  A
    counting context traces every ray: its per-ray figures are over all of them."""
    sc = scenes.ibl_test_scene(1.0, (64, 32), 8, 4)
    compare(sc, ob.settings(48, 36, seed=54), ((0, 4),), "environment light", 48 * 36)
    box = scenes.tiny_box(48 / 36)
    st = ob.settings(48, 36, seed=51)
    plain, count = render(box, st, ((0, 3),)), render(box, st, ((0, 3),), flags=abi.FLAG_COUNT_TRAVERSAL)
    assert plain[1] == count[1] and plain[2] > 0 and count[2] == 0
    assert_bit_equal(plain[0], count[0], "counting context")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [abi.FLAG_TIME_KERNELS, 0], ids=["event-timed", "hipGraph"])
def test_launch_loops(flags):
    """640 x 480, 4 passes, 614 400 slots at two stripes: the event-timed loop, and the loop that replays captured blocks of iterations."""
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "matte")
    skip, _ = compare(sc, ob.settings(640, 480, seed=79), ((0, 4),), "640x480, flags %d" % flags, 640 * 480, stripes=2, flags=flags)
    assert skip[2] > 0


def box_with_light(y, normal, light_material):
    b = scenes.SceneBuilder()
    scenes.cornell_walls(b)          # (its own light is replaced below: drop the quad, keep the walls)
    b.vertices, b.triangles = b.vertices[:5], b.triangles[:5]
    b.num_vertices = sum(len(v) for v in b.vertices)
    corners = [(-0.5, y, -0.5), (0.5, y, -0.5), (0.5, y, 0.5), (-0.5, y, 0.5)]
    b.add_quad(corners if normal[1] < 0 else corners[::-1], normal, (1, 0, 0), light_material(b))
    return b


def matte_light(b):
    return b.matte(b.spectrum_srgb_nonlinear(0.9, 0.9, 0.9), emittance=b.spectrum_d65(4.0, scenes.D65_RGB))


@pytest.mark.gpu
@pytest.mark.parametrize("y", (2.6, 2.499), ids=["above-the-ceiling", "under-the-ceiling"])
def test_light_that_faces_up(y):
    """The box's light turned to face the ceiling.  Above the ceiling (y = 2.6) no point a path can reach is in front of it: EVERY light
    sample is dead, none is traced, and the frame is black (the camera sees the light's back, which does not emit).  Under the ceiling
    (y = 2.499) the millimetre between the two is in front of the light and a grazing path can enter it, so only the equalities are
    asked.  Fixed slot counts: the pure wavefront schedule, every light sample goes through k_shade (the tail kernel traces its own
    inline and skips none); the automatic count only for the equalities."""
    b = box_with_light(y, (0, 1, 0), matte_light)
    sc = b.build(scenes.cornell_camera(48 / 36), name="light_faces_up")
    for stripes, passes in ((1, 6), (64, 3), (1, 65), (0, 65)):
        skip, full = compare(sc, ob.settings(48, 36, seed=55), ((0, passes),), "light faces up at %g, %d passes, stripes %d" % (y, passes, stripes),
                             48 * 36, stripes=stripes, lit=False)
        if stripes:
            assert skip[2] > 0
        if y > 2.5:
            assert not skip[0].any() and not full[0].any()
            if stripes:
                assert skip[2] == skip[1][2] == full[1][2], (skip[1], skip[2])


@pytest.mark.gpu
def test_scene_without_a_dead_sample():
    """A floor under a light that faces down, nothing else.  Every point of the floor is in front of the light and has it above its
    horizon.  The light itself is a mirror that emits: a path that reaches it from the floor samples no light there (a delta lobe), so no
    sample is taken on the light's own plane either."""
    b = scenes.SceneBuilder()
    white = b.matte(b.spectrum_srgb_nonlinear(0.75, 0.75, 0.75))
    b.add_quad([(-1.5, 0, 2.55), (1.5, 0, 2.55), (1.5, 0, -2.55), (-1.5, 0, -2.55)], (0, 1, 0), (1, 0, 0), white)
    one = b.spectrum_grey(1.0)
    light = b.material(abi.MAT_METAL, (one, b.spectrum_ior("Aluminium", 0, scenes.ALUMINIUM_ETA_RGB), b.spectrum_ior("Aluminium", 1, scenes.ALUMINIUM_K_RGB)),
                       emittance=b.spectrum_d65(4.0, scenes.D65_RGB))
    b.add_quad([(-0.5, 2.499, -0.5), (0.5, 2.499, -0.5), (0.5, 2.499, 0.5), (-0.5, 2.499, 0.5)], (0, -1, 0), (1, 0, 0), light)
    sc = b.build(scenes.cornell_camera(48 / 36), name="floor_under_a_light")
    skip, _ = compare(sc, ob.settings(48, 36, seed=56), ((0, 16),), "floor under a light", 48 * 36)
    assert skip[1][2] > 0 and skip[2] == 0, skip[1:]


@pytest.mark.gpu
def test_against_the_oracle(oracle_rgb):
    """Lambert + mirror (no float libm on a path): the frame of the reference's algorithm in every bit, and its ray counts."""
    sc = scenes.cornell_box_spheres(64 / 36, 8, 4, "matte")
    st = ob.settings(64, 36, seed=57)
    want, ctr = oracle_rgb.scene(sc).render(st, 8)
    for stripes in (1, 0):
        fb, counts, skipped = render(sc, st, ((0, 8),), stripes=stripes)
        assert counts == (64 * 36 * 8, int(ctr.extension_rays), int(ctr.shadow_rays)), (counts, int(ctr.extension_rays), int(ctr.shadow_rays))
        assert (0 < skipped or stripes == 0) and skipped < counts[2]
        assert_bit_equal(fb, want, "dead light samples not traced vs the oracle, stripes %d" % stripes)


# ---- the kernels that keep their code ----------------------------------------------------------------------------------------------
KEPT = os.path.join(ROOT, "tests", "golden", "dead_shadow_kept_kernels.json")


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
@pytest.mark.parametrize("source", ["pt_shade_spec16.hip", "pt_tail.hip", "pt_tail_rgb.hip", "pt_tail_spec16.hip", "pt_tail_multi_rgb.hip", "pt_tail_tex_rgb.hip"])
def test_spectral_and_tail_kernels_keep_their_resources(source, tmp_path):
    """The compiler's resource remarks of the spectral shade kernels and of the tail kernels equal those recorded from the commit before
    this change (tests/golden/dead_shadow_kept_kernels.json: all twelve translation units whose kernels keep their code).  The six that
    compile in under a minute each are checked here; the MultiBSDF and textured spectral units take several minutes apiece and are
    compared in profiles/dead_shadow_resource_remarks.txt, with the object files."""
    import json
    want = json.load(open(KEPT))[source]
    got = resource_remarks(source, tmp_path)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
