"""Which k_shade and which k_tail a window runs is decided once, on the host (render_plan.cpp, planShadeVariant), and looked up in the one
table of built kernels (pt_shade.hip).

On the host: slrhip_debug_shade_plan over all 128 combinations of its seven inputs against `parent_if_chains` below — the if-chains that
chose the kernel before there was a table (launchShade -> launchShadeMulti -> launchShade{RGB,Spec16,Tex*,Multi*}[Primary[Seeded]] and
launchTail, spread over 21 files), transcribed branch for branch — and against the rows written out in SHADE_ROWS and TAIL_ROWS, one per
explicit instantiation in pt_shade_*.hip and pt_tail_*.hip.  There are 24 k_shade rows (16 plain: RGB and spectral, tables in LDS or HBM,
with or without the glossy lobes, and the RGB ones again with the fused start resumed and seeded; 8 all-lobes: MultiBSDF and textured, RGB
plain / resumed / seeded and spectral) and 12 k_tail rows.  (The issue behind this test counted 22 k_shade instantiations: it left out the
two spectral all-lobes kernels, pt_shade_multi_spec.hip and pt_shade_tex_spec.hip, which the parent built and which stay.)

On the GPU: every row is reached by a scene, and a scene renders the same frame in every bit, with the same sample, extension-ray and
shadow-ray counts, whether it runs the plain kernel (SLRHIP_FLAG_NO_PRIMARY_PASS), the fused start, or the automatic slot count that ends
in the tail kernel; after each render slrhip_debug_shade_kernel says the row the truth table gives for the scene was the one launched."""
import ctypes as C
import itertools

import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, binding, scenes
from test_shade_occupancy import patchwork

OFF = abi.FLAG_NO_PRIMARY_PASS

# (spectral, tables in LDS, glossy lobes, MultiBSDF code, texture code, PRIMARY, RESUME): k_shade's template arguments
SHADE_ROWS = {
    # pt_shade_rgb.hip
    (0, 1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0, 0),
    # pt_shade_rgb_primary.hip
    (0, 1, 0, 0, 0, 1, 1), (0, 1, 1, 0, 0, 1, 1), (0, 0, 0, 0, 0, 1, 1), (0, 0, 1, 0, 0, 1, 1),
    # pt_shade_rgb_primary_seeded.hip
    (0, 1, 0, 0, 0, 1, 0), (0, 1, 1, 0, 0, 1, 0), (0, 0, 0, 0, 0, 1, 0), (0, 0, 1, 0, 0, 1, 0),
    # pt_shade_spec16.hip
    (1, 1, 0, 0, 0, 0, 0), (1, 1, 1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 0, 0, 0),
    # pt_shade_multi_{rgb,rgb_primary,rgb_primary_seeded,spec}.hip
    (0, 0, 1, 1, 0, 0, 0), (0, 0, 1, 1, 0, 1, 1), (0, 0, 1, 1, 0, 1, 0), (1, 0, 1, 1, 0, 0, 0),
    # pt_shade_tex_{rgb,rgb_primary,rgb_primary_seeded,spec}.hip
    (0, 0, 1, 1, 1, 0, 0), (0, 0, 1, 1, 1, 1, 1), (0, 0, 1, 1, 1, 1, 0), (1, 0, 1, 1, 1, 0, 0),
}
# k_tail has neither PRIMARY nor RESUME: pt_tail_{rgb,spec16}.hip, pt_tail_{multi,tex}_{rgb,spec}.hip
TAIL_ROWS = {
    (0, 1, 0, 0, 0, 0, 0), (0, 1, 1, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0, 0),
    (1, 1, 0, 0, 0, 0, 0), (1, 1, 1, 0, 0, 0, 0), (1, 0, 0, 0, 0, 0, 0), (1, 0, 1, 0, 0, 0, 0),
    (0, 0, 1, 1, 0, 0, 0), (1, 0, 1, 1, 0, 0, 0), (0, 0, 1, 1, 1, 0, 0), (1, 0, 1, 1, 1, 0, 0),
}


def parent_if_chains(spectral, shade_tables, has_microfacet, has_multi, num_textures, primary, primary_rng):
    """(k_shade row, k_tail row) as the launchers chose them before the table, one `if` here per `if` there."""
    lds, glossy = int(shade_tables), int(has_microfacet)
    # launchShade
    if has_multi or num_textures:
        # launchShadeMulti
        if num_textures:
            if spectral:
                shade = (1, 0, 1, 1, 1, 0, 0)                           # launchShadeTexSpec
            elif primary:
                # launchShadeTexRGBPrimary: `if (!pb.primaryRng)` -> ...Seeded
                shade = (0, 0, 1, 1, 1, 1, 0) if not primary_rng else (0, 0, 1, 1, 1, 1, 1)
            else:
                shade = (0, 0, 1, 1, 1, 0, 0)                           # launchShadeTexRGB
        elif spectral:
            shade = (1, 0, 1, 1, 0, 0, 0)                               # launchShadeMultiSpec
        elif primary:
            # launchShadeMultiRGBPrimary: `if (!pb.primaryRng)` -> ...Seeded
            shade = (0, 0, 1, 1, 0, 1, 0) if not primary_rng else (0, 0, 1, 1, 0, 1, 1)
        else:
            shade = (0, 0, 1, 1, 0, 0, 0)                               # launchShadeMultiRGB
    elif spectral:
        shade = (1, lds, glossy, 0, 0, 0, 0)                            # launchShadeSpec16: four kernels by (lds, glossy)
    elif primary:
        # launchShadeRGB -> launchShadeRGBPrimary: `if (!pb.primaryRng)` -> ...Seeded
        shade = (0, lds, glossy, 0, 0, 1, 0) if not primary_rng else (0, lds, glossy, 0, 0, 1, 1)
    else:
        shade = (0, lds, glossy, 0, 0, 0, 0)                            # launchShadeRGB
    # launchTail
    if num_textures:
        tail = (1, 0, 1, 1, 1, 0, 0) if spectral else (0, 0, 1, 1, 1, 0, 0)
    elif has_multi:
        tail = (1, 0, 1, 1, 0, 0, 0) if spectral else (0, 0, 1, 1, 0, 0, 0)
    elif spectral:
        tail = (1, lds, glossy, 0, 0, 0, 0)
    else:
        tail = (0, lds, glossy, 0, 0, 0, 0)
    return shade, tail


def shade_plan(*inputs):
    """slrhip_debug_shade_plan: (the variant, has a k_shade row, has a k_tail row)"""
    lib = binding.load_library()
    plan = (C.c_uint32 * 9)(*([7] * 9))
    assert lib.slrhip_debug_shade_plan(*inputs, plan) == 0
    assert all(x in (0, 1) for x in plan), list(plan)
    return tuple(plan[:7]), bool(plan[7]), bool(plan[8])


def test_exports():
    lib = binding.load_library()
    for name in ("slrhip_debug_shade_plan", "slrhip_debug_shade_kernel"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    assert lib.slrhip_debug_shade_plan(0, 0, 0, 0, 0, 0, 0, None) == 1 and lib.slrhip_debug_shade_kernel(None, None) == 1      # no GPU needed to refuse


def test_the_choice_is_the_parents_for_all_128_inputs():
    assert len(SHADE_ROWS) == 24 and len(TAIL_ROWS) == 12
    shade_seen, tail_seen = set(), set()
    for inputs in itertools.product((0, 1), repeat=7):
        spectral, tables, microfacet, multi, textures, primary, rng = inputs
        num_textures = 3 * textures                                     # a count, not a flag
        want_shade, want_tail = parent_if_chains(spectral, tables, microfacet, multi, num_textures, primary, rng)
        got, shade_row, tail_row = shade_plan(spectral, tables, microfacet, multi, num_textures, primary, rng)
        assert got == want_shade, (inputs, got, want_shade)
        assert shade_row and tail_row, (inputs, got)                   # never a variant without its kernels
        assert got in SHADE_ROWS and want_tail in TAIL_ROWS, (inputs, got, want_tail)
        assert got[:5] + (0, 0) == want_tail, (inputs, got, want_tail)      # the tail kernel is the twin: the same code without a start
        # what the planner never produces is canonicalised, not refused: RESUME only with PRIMARY, and no PRIMARY in a spectral context
        if not primary or spectral:
            assert got[5:] == (0, 0), (inputs, got)
        if multi or textures:
            assert got[1:4] == (0, 1, 1) and got[4] == textures, (inputs, got)      # tables in HBM, all lobes; textures win
        shade_seen.add(got)
        tail_seen.add(want_tail)
    assert shade_seen == SHADE_ROWS and tail_seen == TAIL_ROWS


# ---- every row, on the GPU ---------------------------------------------------------------------------------------------------------
def mix(*features):
    return lambda: scenes.feature_mix(features)


# name, builder, instanced, (tables in LDS, glossy lobes, MultiBSDF code, texture code) of its kernels, frame, passes, modes.  The scenes
# with instances run the primary pass without the stream plane (render_plan.h): the seeded twins.  feature_mix (scenes.py) gives the
# combinations no single-purpose builder has: "many" is test_shade_occupancy's patchwork again (more than 32 materials, more than 16
# emitting triangles: tables in HBM) with a GGX sphere in front of it where "glossy" is set.
RGB, BOTH = (abi.MODE_RGB,), (abi.MODE_RGB, abi.MODE_SPECTRAL)
SCENES = [
    ("matte, glass spheres", lambda: scenes.cornell_box_spheres(1.0, 8, 4, "glass"), 0, (1, 0, 0, 0), (48, 36), 3, BOTH),
    ("glossy", lambda: scenes.cornell_box_boxes(1.0), 0, (1, 1, 0, 0), (24, 18), 2, BOTH),
    ("patchwork", patchwork, 0, (0, 0, 0, 0), (48, 36), 6, BOTH),
    ("patchwork, glossy", mix("many", "glossy"), 0, (0, 1, 0, 0), (24, 18), 2, BOTH),
    ("MultiBSDF", lambda: scenes.cornell_multi(1.0, 10, 5), 0, (0, 1, 1, 0), (24, 18), 2, BOTH),
    ("textured", lambda: scenes.cornell_textured(1.0, 10, 5), 0, (0, 1, 1, 1), (24, 18), 2, BOTH),
    ("instanced", lambda: scenes.cornell_instanced(1.0, 10, 5), 1, (1, 0, 0, 0), (48, 36), 3, RGB),
    ("instanced, glossy", mix("inst", "glossy"), 1, (1, 1, 0, 0), (24, 18), 2, RGB),
    ("instanced, patchwork", mix("inst", "many"), 1, (0, 0, 0, 0), (24, 18), 2, RGB),
    ("instanced, patchwork, glossy", mix("inst", "many", "glossy"), 1, (0, 1, 0, 0), (24, 18), 2, RGB),
    ("instanced, MultiBSDF", mix("inst", "multi"), 1, (0, 1, 1, 0), (24, 18), 2, RGB),
    ("instanced, textured", mix("inst", "tex"), 1, (0, 1, 1, 1), (24, 18), 2, RGB),
]


def rows_of(instanced, code, mode):
    """(k_shade row with SLRHIP_FLAG_NO_PRIMARY_PASS, k_shade row without the flag, k_tail row) of a scene, by the truth table.  The
    inputs of the plan: the pass runs in RGB contexts (no scene here has an environment light) and keeps its stream plane where the
    scene has no instances (render_plan.h, planPrimary; these trees are far below the quantized size)."""
    spectral = int(mode == abi.MODE_SPECTRAL)
    lds, glossy, multi, tex = code
    plain, tail = parent_if_chains(spectral, lds, glossy, multi, 2 * tex, 0, 0)
    fused, tail2 = parent_if_chains(spectral, lds, glossy, multi, 2 * tex, 1 - spectral, 1 - instanced)
    assert plain == (spectral,) + code + (0, 0) and tail == tail2 == plain
    return plain, fused, tail


def test_the_scenes_reach_every_row():
    """The union of the rows the truth table gives for the scenes of the GPU test, which checks after every render that the row
    launched was that one."""
    shade, tail = set(), set()
    for _, _, instanced, code, _, _, modes in SCENES:
        for mode in modes:
            plain, fused, twin = rows_of(instanced, code, mode)
            shade |= {plain, fused}
            tail.add(twin)
    assert shade == SHADE_ROWS, sorted(SHADE_ROWS - shade)
    assert tail == TAIL_ROWS, sorted(TAIL_ROWS - tail)


def render(sc, st, passes, mode, stripes, flags):
    """frame, (samples, extension rays, shadow rays), slrhip_debug_shade_kernel"""
    c = Context(mode=mode, stripes=stripes, flags=flags)
    c.upload_scene(sc)
    c.render_begin(st)
    c.render(0, passes)
    fb = c.read_framebuffer()
    ctr = c.counters()
    out = fb, (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), c.shade_kernel()
    c.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name, make, instanced, code, frame, passes, modes", SCENES, ids=[s[0] for s in SCENES])
def test_every_row_renders_the_same_frame(name, make, instanced, code, frame, passes, modes):
    sc = make()
    assert (len(sc.instances) > 0) == bool(instanced) and sc.env is None, name
    st = ob.settings(frame[0], frame[1], seed=61)
    for mode in modes:
        plain, fused, _ = rows_of(instanced, code, mode)
        off = render(sc, st, passes, mode, 1, OFF)
        on = render(sc, st, passes, mode, 1, 0)
        auto = render(sc, st, passes, mode, 0, 0)
        what = "%s, mode %d" % (name, mode)
        print(what, off[1], off[2], on[2], auto[2])
        # the row launched, and the tail kernel (the twin: the row without PRIMARY and RESUME) only where the automatic count ends in it
        assert off[2] == (plain, True, False), (what, off[2], plain)
        assert on[2] == (fused, True, False), (what, on[2], fused)
        assert auto[2] == (fused, True, True), (what, auto[2], fused)
        assert off[1] == on[1] == auto[1] and off[1][0] == frame[0] * frame[1] * passes, (what, off[1], on[1], auto[1])
        assert_bit_equal(on[0], off[0], "fused start vs SLRHIP_FLAG_NO_PRIMARY_PASS: " + what)
        assert_bit_equal(auto[0], off[0], "automatic slot count (tail kernel) vs fixed stripes: " + what)
        assert off[0].sum() > 0, what
