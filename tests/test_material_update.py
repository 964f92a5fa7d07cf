"""Changing materials, spectra, textures and lights without a scene upload (slrhip_set_materials).

CPU: the exports, the struct, every refusal through the context-free check with its code and message, the three facts the host keeps
about the triangles, and the closed form of the light tables against the upload's definition (a sequential float32 Kahan sum of ones,
then a division).

GPU: the yardstick throughout is a second context freshly uploaded with the changed scene; every comparison is by bytes, no tolerance
is involved.  An update with the uploaded tables changes nothing; a change that leaves the emitting set alone works on contexts
without SLRHIP_FLAG_DYNAMIC_GEOMETRY; a change of the emitting set rebuilds the light list on the device (ranks checked against numpy:
the rank of each emitting triangle in triangle order); set_vertices, set_instance_transforms and rebuild_top_level commute with it;
nothing accumulated is reset; a refusal leaves every read-out as it was.

The terrain of the emitting-set tests: lattice_terrain(23) with its triangles re-assigned to eight matte materials as i % 8 and the two
coincident quads kept on the uploaded light.  Classes of ~130 triangles alone cannot give the light counts 1, 16, 17, 64 +- 1 and
256 +- 1, so every fourth triangle of the first 1 025 is carved out into nine further matte materials whose sizes add up to exactly
those counts (they interleave with the i % 8 pattern and span five workgroups of the scatter), and the last triangle has a material
of its own."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, SlrHipError
from test_vertex_update import SPP, assert_same, everything, kahan, query_rays, same_bytes, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
DYNAMIC, INSTANCED, DEVICE = abi.FLAG_DYNAMIC_GEOMETRY, abi.FLAG_DYNAMIC_INSTANCED, abi.FLAG_BVH_DEVICE_BUILD
RGB, SPECTRAL = abi.MODE_RGB, abi.MODE_SPECTRAL


def variant(sc, name, materials=None, spectra=None, textures=None, triangles=None, vertices=None, instances=None):
    """The scene with some of its arrays replaced: what a fresh context uploads, and whose tables set_materials takes."""
    assert sc.env is None
    pick = lambda new, old: old if new is None else new
    return abi.Scene(pick(vertices, sc.vertices), pick(triangles, sc.triangles), pick(materials, sc.materials), pick(spectra, sc.spectra), sc.spectrum_data,
                     sc.camera, None, sc.name + "_" + name, textures=pick(textures, sc.textures) if len(sc.textures) else None,
                     texture_texels=sc.texture_texels if len(sc.texture_texels) else None,
                     texture_texels_uvs=sc.texture_texels_uvs if len(sc.texture_texels_uvs) else None,
                     instances=pick(instances, sc.instances) if len(sc.instances) else None)


def tables(sc, materials=None, spectra=None, textures=None):
    """An abi.MaterialsDesc over arrays that need not make a valid abi.Scene (the arrays stay alive with it)."""
    d = sc.materials_desc()
    keep = []
    for name, array, dtype in (("materials", materials, abi.material_dtype), ("spectra", spectra, abi.spectrum_dtype), ("textures", textures, abi.texture_dtype)):
        if array is not None:
            a = np.ascontiguousarray(array, dtype)
            keep.append(a)
            setattr(d, name, a.ctypes.data)
            setattr(d, "num_" + name, len(a))
    d._keep = keep
    return d


def emitter_of(sc):
    """(the first emitting material, its emittance spectrum)."""
    m = int(np.nonzero(sc.materials["emittance"] >= 0)[0][0])
    return m, int(sc.materials["emittance"][m])


def dimmed(sc, spectra=None):
    """The spectrum table with the emittance spectrum at half its power (exact in both modes' records)."""
    sp = (sc.spectra if spectra is None else spectra).copy()
    e = emitter_of(sc)[1]
    sp["scale"][e] *= F(0.5)
    sp["rgb"][e] *= F(0.5)
    return sp


@functools.lru_cache(maxsize=None)
def base_scene(name):
    if name == "cornell":
        return scenes.cornell_box_spheres(1.0, 8, 4)
    if name == "textured":
        return scenes.cornell_textured(1.0, 8, 4)
    if name == "image":
        return scenes.cornell_image_textured(1.0, 8, 4)
    if name == "multi":
        return scenes.cornell_multi(1.0, 8, 4)
    if name == "multi_exact":
        return scenes.cornell_multi(1.0, 8, 4, libm_free=True)
    if name == "instanced":
        # the loose walls get a material of their own, so that they can start to emit (the terrain's is used by instanced triangles)
        sc = scenes.lattice_instanced()
        mats = np.concatenate([sc.materials, sc.materials[:1]])
        tris = sc.triangles.copy()
        assert (tris["material"][:4] == 0).all() and sc.instances["first_triangle"].min() >= 6
        tris["material"][:4] = len(sc.materials)
        return variant(sc, "walls", materials=mats, triangles=tris)
    assert name == "terrain"
    return terrain()[0]


# ---- the terrain of the emitting-set tests -----------------------------------------------------------------------------------------------
COUNT_SIZES = [1, 15, 1, 46, 1, 1, 190, 1, 1]            # cumulative: 1, 16, 17, 63, 64, 65, 255, 256, 257
PATTERN, LIGHT, FIRST_COUNT, LAST = range(8), 8, 9, 18


@functools.lru_cache(maxsize=None)
def terrain():
    """(the scene, the emittance spectrum): materials 0 .. 7 matte by i % 8, 8 the uploaded light, 9 .. 17 the carved count classes, 18 the
    last triangle's."""
    sc = scenes.lattice_terrain(23)
    light, spectrum = emitter_of(sc)
    ground = sc.materials[1 - light]
    mats = np.zeros(19, abi.material_dtype)
    mats[:] = ground
    mats["param"][:8] = [-1.0, 0.1, 0.2, 0.3, -1.0, 0.5, 0.6, 0.7]
    mats[LIGHT] = sc.materials[light]
    tris = sc.triangles.copy()
    was_light = tris["material"] == light
    tris["material"] = np.arange(len(tris)) % 8
    tris["material"][was_light] = LIGHT
    carved = np.repeat(np.arange(FIRST_COUNT, FIRST_COUNT + len(COUNT_SIZES)), COUNT_SIZES)
    at = 4 * np.arange(len(carved))
    assert len(carved) == 257 and at.max() < len(tris) and not was_light[at].any()
    tris["material"][at] = carved
    assert not was_light[-1]
    tris["material"][-1] = LAST
    return variant(sc, "classes", materials=mats, triangles=tris), spectrum


def emitting(sc, on, spectrum):
    """The material table with exactly the materials `on` emitting."""
    mats = sc.materials.copy()
    mats["emittance"] = -1
    mats["emittance"][list(on)] = spectrum
    return mats


COUNT = lambda k: list(range(FIRST_COUNT, FIRST_COUNT + k))      # the first k count classes
SUBSETS = [("1_first", COUNT(1), 1), ("16", COUNT(2), 16), ("17", COUNT(3), 17), ("16_again", COUNT(2), 16), ("63", COUNT(4), 63), ("64", COUNT(5), 64),
           ("65", COUNT(6), 65), ("255", COUNT(7), 255), ("256", COUNT(8), 256), ("257", COUNT(9), 257), ("pattern_and_last", list(PATTERN) + [LAST], None),
           ("all_but_first", [m for m in range(19) if m != FIRST_COUNT], None), ("uploaded", [LIGHT], 4)]
RENDERED = {"1_first", "17", "257", "pattern_and_last", "all_but_first"}


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(mode=RGB, which=0, flags=0):
        key = (mode, which, flags)
        if key not in made:
            made[key] = Context(device=0, mode=mode, flags=flags)
        return made[key]
    yield get
    for c in made.values():
        c.close()


def snapshot(ctx, geometry=False):
    """Every read-out a material update could touch; `launches` and `rebuilt` describe the last call, not the scene."""
    m = ctx.debug_materials()
    calls = dict(launches=m.pop("launches"), rebuilt=m.pop("rebuilt"))
    tree = ctx.debug_tree()
    out = dict(m, shade_tris=tree["shade_tris"], leaf_tris=tree["leaf_tris"], nodes=tree["nodes"])
    if geometry:
        g = ctx.debug_geometry()
        out.update(light_tris=g["light_tris"], geo_staged=g["staged"])
        if g["staged"]:
            out["light_tris_staged"] = g["light_tris_staged"]
    return out, calls


def assert_same_snapshot(got, want, what, skip=()):
    assert got.keys() == want.keys(), what
    for k in got:
        if k in skip:
            continue
        if isinstance(got[k], np.ndarray):
            same_bytes(got[k], want[k], "%s: %s" % (what, k))
        else:
            assert got[k] == want[k] or (got[k] != got[k] and want[k] != want[k]), (what, k, got[k], want[k])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------
def test_exports_struct_and_version():
    lib = binding.load_library()
    for name in ("slrhip_set_materials", "slrhip_set_texture_texels", "slrhip_debug_materials_update_check", "slrhip_debug_materials"):
        assert hasattr(lib, name) and name in binding.EXPORTS, name
    assert lib.slrhip_version() == 7
    header = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert re.search(r"#define SLRHIP_VERSION 7\b", header)
    body = re.search(r"typedef struct slrhip_materials_desc \{(.*?)\} slrhip_materials_desc;", header, re.S).group(1)
    fields = re.findall(r"(\w+)(?:\[2\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [f[0] for f in abi.MaterialsDesc._fields_]
    assert C.sizeof(abi.MaterialsDesc) == 72 and abi.MaterialsDesc.reserved.offset == 60
    assert re.search(r"#define SLRHIP_TEXELS_STORE_HALF 1u", header) and abi.TEXELS_STORE_HALF == 1


def refused(code, message, mode, uploaded, kept, tables, **kw):
    with pytest.raises(SlrHipError) as e:
        binding.materials_update_check(mode, uploaded, kept, tables, **kw)
    text = str(e.value)
    assert "(%d)" % code in text and "slrhip_set_materials: " in text and message in text, text


def test_refusals_through_the_check_twin():
    cornell, textured, image, inst = (base_scene(n) for n in ("cornell", "textured", "image", "instanced"))
    for mode in (RGB, SPECTRAL):
        binding.materials_update_check(mode, cornell, False, cornell)
        refused(INVALID, "null argument", mode, cornell, False, None)
        refused(INVALID, "reserved must be 0", mode, cornell, False, cornell, reserved=(0, 1))
        refused(INVALID, "reserved must be 0", mode, cornell, False, cornell, reserved=(7, 0))
        refused(NO_SCENE, "no scene uploaded", mode, None, False, cornell)
        refused(INVALID, "num_materials differs", mode, cornell, True, tables(cornell, materials=cornell.materials[:-1]))
        refused(INVALID, "num_materials differs", mode, cornell, True, textured)
        refused(INVALID, "num_textures differs", mode, textured, True, tables(textured, textures=np.concatenate([textured.textures, textured.textures[:1]])))
        refused(INVALID, "num_textures differs", mode, textured, True, tables(textured, textures=textured.textures[:-1]))
        # a texture's kind and an image's shape
        tex = image.textures.copy()
        assert tex["kind"][1] == abi.TEX_IMAGE_SPECTRUM and tuple(tex["reserved"][1]) == (8, 8, 192)
        tex["kind"][1], tex["spectrum"][1], tex["reserved"][1] = abi.TEX_CHECKER_SPECTRUM, (0, 1), (0, 0, 0)
        refused(UNSUPPORTED, "a texture changes its kind", mode, image, True, variant(image, "k", textures=tex))
        for shape in ((4, 8, 192), (8, 4, 192), (8, 8, 0)):
            tex = image.textures.copy()
            tex["reserved"][1] = shape
            refused(UNSUPPORTED, "changes its width, height or first texel", mode, image, True, variant(image, "s", textures=tex))
        # alpha maps: one taken away, one handed to another material
        alpha = int(np.nonzero(textured.materials["reserved"] >> 16)[0][0])
        mats = textured.materials.copy()
        mats["reserved"][alpha] &= 0xFFFF
        refused(UNSUPPORTED, "alpha map changes", mode, textured, True, variant(textured, "a", materials=mats))
        mats = textured.materials.copy()
        mats["reserved"][0] |= textured.materials["reserved"][alpha] & 0xFFFF0000
        refused(UNSUPPORTED, "alpha map changes", mode, textured, True, variant(textured, "a", materials=mats))
        # lights
        light, spectrum = emitter_of(inst)
        grey = int(inst.triangles["material"][inst.instances["first_triangle"][-1]])
        refused(UNSUPPORTED, "instanced triangles must not emit", mode, inst, True, variant(inst, "e", materials=emitting(inst, [light, grey], spectrum)))
        refused(UNSUPPORTED, "scene has no emitting triangle and no environment light", mode, cornell, True,
                variant(cornell, "dark", materials=emitting(cornell, [], 0)))
        light, spectrum = emitter_of(cornell)
        moved = variant(cornell, "wall", materials=emitting(cornell, [0], spectrum))
        refused(UNSUPPORTED, "the set of emitting materials changes", mode, cornell, False, moved)
        binding.materials_update_check(mode, cornell, True, moved)
        # the upload's own checks, under this call's name
        mats = cornell.materials.copy()
        mats["spectrum"][0][0] = len(cornell.spectra)
        refused(INVALID, "spectrum index out of range", mode, cornell, True, tables(cornell, materials=mats))
        mats = cornell.materials.copy()
        mats["type"][0] = 99
        refused(UNSUPPORTED, "unknown material type", mode, cornell, True, tables(cornell, materials=mats))


def test_more_than_2_to_the_24_lights_are_refused():
    """One degenerate triangle 2^24 + 1 times over: the check needs only the histogram."""
    tiny = base_scene("cornell")
    n = (1 << 24) + 1
    tris = np.zeros(n, abi.triangle_dtype)
    light, spectrum = emitter_of(tiny)
    tris["material"][:-1] = 0
    tris["material"][-1] = light
    big = variant(tiny, "big", triangles=tris)
    facts = binding.materials_update_check(RGB, big, True, big, want_facts=True)
    assert facts[0, 0] == n - 1 and facts[light, 0] == 1
    binding.materials_update_check(RGB, big, True, variant(big, "most", materials=emitting(big, [0], spectrum)))       # 2^24 lights: the limit
    refused(UNSUPPORTED, "more than 2^24 emitting triangles", RGB, big, True, variant(big, "all", materials=emitting(big, [0, light], spectrum)))


def test_the_facts_the_host_keeps_about_the_triangles():
    for name in ("cornell", "textured", "instanced", "terrain"):
        sc = base_scene(name)
        facts = binding.materials_update_check(RGB, sc, False, sc, want_facts=True)
        m = sc.triangles["material"]
        assert np.array_equal(facts[:, 0], np.bincount(m, minlength=len(sc.materials)))
        inside = np.zeros(len(m), bool)
        for inst in sc.instances:
            inside[inst["first_triangle"]:inst["first_triangle"] + inst["num_triangles"]] = True
        assert np.array_equal(facts[:, 1], np.bincount(m[inside], minlength=len(sc.materials)) > 0)
        assert np.array_equal(facts[:, 2].view(np.int32), (sc.materials["reserved"] >> 16).astype(np.int32) - 1)
    assert facts[:, 0].tolist()[FIRST_COUNT:] == COUNT_SIZES + [1]


@pytest.mark.parametrize("n", [1, 2, 3, 16, 17, 255, 4097])
def test_closed_form_of_the_light_tables(n):
    """RegularConstantDiscrete1D over n importances of 1.0f as the upload builds it (and the light_kat fixtures record it): a sequential
    float32 Kahan sum, then every entry divided by the integral."""
    pmf, cdf = np.ones(n, F), np.zeros(n + 1, F)
    result, comp = F(0), F(0)
    for i in range(n):
        c_input = F(pmf[i] - comp)
        sum_temp = F(result + c_input)
        comp = F(F(sum_temp - result) - c_input)
        result = sum_temp
        cdf[i + 1] = result
    pmf, cdf[1:] = pmf / result, cdf[1:] / result
    assert comp == 0 and result == n
    same_bytes(np.full(n, F(1) / F(n), F), pmf, "PMF")
    same_bytes(np.arange(n + 1, dtype=F) / F(n), cdf, "CDF")


# ---- GPU: the tables -----------------------------------------------------------------------------------------------------------------------
IDENTITY = [("cornell", RGB, 0), ("cornell", SPECTRAL, 0), ("textured", RGB, 0), ("image", SPECTRAL, 0), ("multi", RGB, 0), ("terrain", RGB, DYNAMIC),
            ("terrain", RGB, DYNAMIC | DEVICE), ("instanced", RGB, DYNAMIC | INSTANCED)]


@pytest.mark.gpu
@pytest.mark.parametrize("name, mode, flags", IDENTITY)
def test_identity_update_changes_nothing(contexts, name, mode, flags):
    sc = base_scene(name)
    ctx = contexts(mode, 0, flags)
    ctx.upload_scene(sc)
    rays = query_rays(sc, 512)
    before, _ = snapshot(ctx, bool(flags & DYNAMIC))
    want = everything(ctx, rays)
    ctx.set_materials(sc)
    after, calls = snapshot(ctx, bool(flags & DYNAMIC))
    assert_same_snapshot(after, before, name + " identity")
    assert calls == dict(launches=1, rebuilt=False)
    assert_same(everything(ctx, rays), want, name + " identity")


def changed(name, step):
    """The scenes of assertion 2: the emitting set stays, everything else moves."""
    sc = base_scene(name)
    mats, tex = sc.materials.copy(), sc.textures.copy()
    light, _ = emitter_of(sc)
    if name == "cornell":
        metal = int(np.nonzero(mats["type"] == abi.MAT_METAL)[0][0])
        mats["spectrum"][0], mats["spectrum"][1] = sc.materials["spectrum"][1], sc.materials["spectrum"][0]      # red <-> blue
        mats["param"][2] = 0.4                                                                                   # the white walls: Oren-Nayar
        if step == "glossy":                                                                                     # the mirror sphere: GGX
            mats["type"][metal], mats["spectrum"][metal][0], mats["param"][metal] = abi.MAT_MF_METAL, -1, 0.2
        return variant(sc, step, materials=mats, spectra=dimmed(sc))
    if name == "textured":
        checker = int(np.nonzero(tex["kind"] == abi.TEX_CHECKER_SPECTRUM)[0][0])
        tex["spectrum"][checker] = tex["spectrum"][checker][::-1]
        tex["offset"][checker], tex["scale"][checker] = (0.25, 0.125), (3.0, 2.0)
        bump = int(np.nonzero(tex["kind"] == abi.TEX_CHECKER_NORMAL)[0][0])
        tex["value"][bump][0] = 0.5
        mats["param"][mats["param"] == F(0.4)] = 0.7
        return variant(sc, step, materials=mats, textures=tex, spectra=dimmed(sc))
    if name == "image":
        tex["offset"][0], tex["scale"][0] = (0.5, 0.25), (1.0, 2.0)
        mats["param"][mats["param"] == F(0.3)] = -1.0
        # one spectrum more in the table: every later segment of the staged tables moves
        return variant(sc, step, materials=mats, textures=tex, spectra=np.concatenate([sc.spectra, sc.spectra[:1]]))
    assert name in ("multi", "multi_exact")
    multi = np.nonzero(mats["type"] == abi.MAT_MULTI)[0]
    mats["param"][multi[0]], mats["param2"][multi[0]] = 0.5, 0.5
    mats["spectrum"][multi[2]][2] = abi.MULTI_INVERSE_0
    if step == "matte":                                                   # the GGX component becomes Lambert
        ggx = int(np.nonzero(mats["type"] == abi.MAT_MF_METAL)[0][0])
        mats["type"][ggx], mats["spectrum"][ggx], mats["param"][ggx] = abi.MAT_MATTE, (sc.materials["spectrum"][0][0], -1, -1), -1.0
    return variant(sc, step, materials=mats, spectra=dimmed(sc))


SAME_SET = [("cornell", RGB, ["colours", "glossy", "colours"]), ("cornell", SPECTRAL, ["glossy", "colours"]), ("textured", RGB, ["mapping"]),
            ("textured", SPECTRAL, ["mapping"]), ("image", RGB, ["mapping"]), ("image", SPECTRAL, ["mapping"]), ("multi", RGB, ["factors", "matte", "factors"]),
            ("multi", SPECTRAL, ["matte"])]


@pytest.mark.gpu
@pytest.mark.parametrize("name, mode, steps", SAME_SET)
def test_same_emitting_set_equals_a_fresh_upload_without_kept_geometry(contexts, name, mode, steps):
    sc = base_scene(name)
    ctx, fresh = contexts(mode, 0, 0), contexts(mode, 1, 0)
    ctx.upload_scene(sc)
    rays = query_rays(sc, 512)
    flips = [ctx.debug_materials()["has_microfacet"]]
    for step in steps:
        new = changed(name, step)
        ctx.set_materials(new)
        fresh.upload_scene(new)
        got, calls = snapshot(ctx)
        assert_same_snapshot(got, snapshot(fresh)[0], "%s %s" % (name, step))
        assert calls == dict(launches=1, rebuilt=False)
        assert_same(everything(ctx, rays), everything(fresh, rays), "%s %s" % (name, step))
        flips.append(got["has_microfacet"])
    if name == "cornell" and len(steps) == 3:                       # (a MULTI record counts as glossy whatever its components are)
        assert flips == [False, False, True, False], flips


@pytest.mark.gpu
def test_changed_libm_free_cornell_equals_the_oracle(contexts):
    sc, new = base_scene("multi_exact"), changed("multi_exact", "factors")
    ctx = contexts(RGB, 0, 0)
    ctx.upload_scene(sc)
    ctx.set_materials(new)
    ctx.render_begin(settings())
    ctx.render(0, SPP)
    got = ctx.read_framebuffer()
    frame, _ = ob.load("oracle", RGB).scene(new).render(settings(), SPP)
    assert_bit_equal(got, frame, "changed libm-free Cornell vs the oracle")
    assert np.isfinite(got).all() and got.max() > 0


# ---- GPU: the emitting set changes ----------------------------------------------------------------------------------------------------------
def expected_lights(sc):
    """(ShadeTri::light of every triangle, the triangle of every light): ranks in triangle order."""
    on = sc.materials["emittance"][sc.triangles["material"]] >= 0
    light = np.where(on, np.cumsum(on) - 1, -1).astype(np.int32)
    return light, np.nonzero(on)[0].astype(np.uint32)


def check_lights(snap, sc, what, fits_otherwise=False):
    light, order = expected_lights(sc)
    n = len(order)
    assert snap["lights"] == n and snap["light_pow2"] == (1 << (n.bit_length() - 1) if n else 0) and snap["importance"] == F(n), what
    assert snap["staged"] == snap["geo_staged"] and (snap["staged"] or n > 16 or not fits_otherwise), what
    assert not (snap["staged"] and n > 16), what
    same_bytes(snap["shade_tris"]["light"], light, what + ": ShadeTri.light against numpy")
    same_bytes(snap["light_tris"][:, 3], order, what + ": LightTri.tri against numpy")
    same_bytes(snap["light_tris"][:, 7], sc.triangles["material"][order], what + ": LightTri.material against numpy")
    same_bytes(snap["pmf"], np.full(n, F(1) / F(n), F), what + ": PMF")
    same_bytes(snap["cdf"], np.arange(n + 1, dtype=F) / F(n), what + ": CDF")
    if snap["geo_staged"]:
        same_bytes(snap["light_tris_staged"], snap["light_tris"], what + ": the two copies of the lights")


@pytest.mark.gpu
@pytest.mark.parametrize("builder", [0, DEVICE])
def test_emitting_subsets_of_the_terrain_equal_a_fresh_upload(contexts, builder):
    sc, spectrum = terrain()
    ctx, fresh = contexts(RGB, 0, DYNAMIC | builder), contexts(RGB, 1, DYNAMIC | builder)
    ctx.upload_scene(sc)
    assert ctx.debug_tree(summary_only=True)["builder_name"] == ("device" if builder else "host SAH")
    rays = query_rays(sc, 512)
    nt = len(sc.triangles)
    for label, on, count in SUBSETS:
        new = variant(sc, label, materials=emitting(sc, on, spectrum))
        light, order = expected_lights(new)
        assert count is None or len(order) == count
        if label == "1_first":
            assert order[0] == 0
        if label == "pattern_and_last":
            assert len(order) >= 513 and order[-1] == nt - 1
        if label == "all_but_first":
            assert len(order) == nt - 1
        ctx.set_materials(new)
        fresh.upload_scene(new)
        got, calls = snapshot(ctx, True)
        check_lights(got, new, label, fits_otherwise=True)       # 19 materials, RGB: the tables are staged exactly while the lights fit
        assert got["staged"] == (len(order) <= 16), label
        assert_same_snapshot(got, snapshot(fresh, True)[0], label)
        assert calls == dict(launches=5, rebuilt=True), calls
        if label in RENDERED:
            assert_same(everything(ctx, rays), everything(fresh, rays), label)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [RGB, SPECTRAL])
def test_lamp_off_and_a_wall_on(contexts, mode):
    sc = base_scene("cornell")
    ctx, fresh = contexts(mode, 0, DYNAMIC), contexts(mode, 1, DYNAMIC)
    light, spectrum = emitter_of(sc)
    new = variant(sc, "wall", materials=emitting(sc, [2], spectrum), spectra=dimmed(sc))
    ctx.upload_scene(sc)
    ctx.set_materials(new)
    fresh.upload_scene(new)
    got, calls = snapshot(ctx, True)
    check_lights(got, new, "lamp off, white walls on")
    assert got["lights"] == 6 and calls["rebuilt"]
    assert_same_snapshot(got, snapshot(fresh, True)[0], "lamp off, white walls on")
    rays = query_rays(sc, 512)
    assert_same(everything(ctx, rays), everything(fresh, rays), "lamp off, white walls on")


# ---- GPU: order with the other updates ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vertices_first", [True, False])
def test_set_vertices_and_set_materials_commute(contexts, vertices_first):
    sc, spectrum = terrain()
    ctx, fresh = contexts(RGB, 0, DYNAMIC), contexts(RGB, 1, DYNAMIC)
    v = sc.vertices.copy()
    v["position"][:, 1] += (np.random.default_rng(6).integers(-2, 3, len(v)) * 0.25).astype(F)
    mats = emitting(sc, COUNT(3) + [LAST], spectrum)
    ctx.upload_scene(sc)
    if vertices_first:
        ctx.set_vertices(v)
        ctx.set_materials(variant(sc, "m", materials=mats))
    else:
        ctx.set_materials(variant(sc, "m", materials=mats))
        ctx.set_vertices(v)
    final = variant(sc, "final", materials=mats, vertices=v)
    fresh.upload_scene(final)
    got = snapshot(ctx, True)[0]
    check_lights(got, final, "vertices and materials")
    # the refitted tree keeps its shape and has exact boxes: the fresh upload builds another one (test_vertex_update.py covers the tree)
    assert_same_snapshot(got, snapshot(fresh, True)[0], "vertices and materials", skip=("nodes", "leaf_tris"))
    rays = query_rays(final, 512)
    assert_same(everything(ctx, rays), everything(fresh, rays), "vertices and materials")


@pytest.mark.gpu
def test_instanced_scene_after_transforms_and_a_top_level_rebuild(contexts):
    sc = base_scene("instanced")
    ctx, fresh = contexts(RGB, 0, DYNAMIC | INSTANCED), contexts(RGB, 1, DYNAMIC | INSTANCED)
    light, spectrum = emitter_of(sc)
    walls = len(sc.materials) - 1
    inst = sc.instances.copy()
    for k in ("local_to_world", "world_to_local"):                      # the two boxes change places: exact matrices stay exact
        inst[k][[4, 5]] = sc.instances[k][[5, 4]]
    assert inst["first_triangle"][4] == inst["first_triangle"][5]
    mats = emitting(sc, [light, walls], spectrum)
    mats["param"][1] = 0.3
    ctx.upload_scene(sc)
    ctx.set_instance_transforms(inst[4:6], first=4)
    ctx.rebuild_top_level()
    tree = ctx.debug_tree()
    ctx.set_materials(variant(sc, "m", materials=mats))
    after = ctx.debug_tree()
    for k in ("nodes", "leaf_tris", "instances"):
        same_bytes(after[k], tree[k], "the tree read-out after set_materials: " + k)
    final = variant(sc, "final", materials=mats, instances=inst)
    fresh.upload_scene(final)
    got = snapshot(ctx, True)[0]
    check_lights(got, final, "instanced")
    assert got["lights"] == 6
    assert_same_snapshot(got, snapshot(fresh, True)[0], "instanced", skip=("nodes", "leaf_tris"))
    rays = query_rays(final, 512)
    assert_same(everything(ctx, rays), everything(fresh, rays), "instanced")


# ---- GPU: nothing is reset; refusals --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_nothing_is_reset_between_two_renders(contexts):
    """render, set_materials, render with no render_begin between: the sensor holds the first passes of the old scene and the later
    passes of the new one, added in pass order."""
    sc, new = base_scene("cornell"), changed("cornell", "glossy")
    ctx, fresh = contexts(RGB, 0, 0), contexts(RGB, 1, 0)
    half = SPP // 2

    def passes(c, which):
        out = []
        for p in which:
            c.render_begin(settings())
            c.render(p, 1)
            out.append(c.read_framebuffer())
        return out
    fresh.upload_scene(sc)
    old = passes(fresh, range(SPP))
    fresh.upload_scene(new)
    late = passes(fresh, range(half, SPP))
    ctx.upload_scene(sc)
    ctx.render_begin(settings())
    ctx.render(0, half)
    ctx.set_materials(new)
    ctx.render(half, SPP - half)
    got = ctx.read_framebuffer()
    assert_bit_equal(got, kahan(old[:half] + late), "old first half + new second half")
    assert not np.array_equal(got, kahan(old))
    assert ctx.counters().samples == 32 * 32 * SPP


@pytest.mark.gpu
def test_refusals_on_a_live_context_change_nothing(contexts):
    lib = binding.load_library()
    sc = base_scene("textured")
    plain, dynamic = contexts(RGB, 0, 0), contexts(RGB, 0, DYNAMIC)
    light, spectrum = emitter_of(sc)

    def refuse(ctx, code, message, tables, reserved=(0, 0)):
        d = tables.materials_desc() if isinstance(tables, abi.Scene) else tables
        if d is not None:
            d.reserved[0], d.reserved[1] = reserved
        rc = lib.slrhip_set_materials(ctx.handle, C.byref(d) if d is not None else None, None)
        text = lib.slrhip_last_error_string().decode()
        assert rc == code and "slrhip_set_materials: " in text and message in text, (rc, text)

    empty = Context(device=0)
    refuse(empty, NO_SCENE, "no scene uploaded", sc)
    empty.close()
    assert lib.slrhip_set_materials(None, C.byref(sc.materials_desc()), None) == INVALID
    for ctx in (plain, dynamic):
        ctx.upload_scene(sc)
        kept = ctx is dynamic
        before = snapshot(ctx, kept)[0]
        refuse(ctx, INVALID, "null argument", None)
        refuse(ctx, INVALID, "reserved must be 0", sc, reserved=(1, 0))
        refuse(ctx, INVALID, "num_materials differs", tables(sc, materials=sc.materials[:-1]))
        refuse(ctx, INVALID, "num_textures differs", tables(sc, textures=sc.textures[:-1]))
        tex = sc.textures.copy()
        checker = int(np.nonzero(tex["kind"] == abi.TEX_CHECKER_SPECTRUM)[0][0])
        tex["kind"][checker] = abi.TEX_CHECKER_FLOAT
        refuse(ctx, INVALID, "names a texture that is not a spectrum texture", tables(sc, textures=tex))
        mats = sc.materials.copy()
        mats["reserved"][int(np.nonzero(mats["reserved"] >> 16)[0][0])] &= 0xFFFF
        refuse(ctx, UNSUPPORTED, "alpha map changes", variant(sc, "a", materials=mats))
        refuse(ctx, UNSUPPORTED, "no emitting triangle and no environment light", variant(sc, "dark", materials=emitting(sc, [], 0)))
        mats = sc.materials.copy()
        mats["spectrum"][0][0] = len(sc.spectra)
        refuse(ctx, INVALID, "spectrum index out of range", tables(sc, materials=mats))
        if not kept:
            refuse(ctx, UNSUPPORTED, "the set of emitting materials changes", variant(sc, "wall", materials=emitting(sc, [0, light], spectrum)))
        assert_same_snapshot(snapshot(ctx, kept)[0], before, "after the refusals")
    image = base_scene("image")
    plain.upload_scene(image)
    before = snapshot(plain)[0]
    tex = image.textures.copy()
    tex["reserved"][1] = (4, 8, 192)
    refuse(plain, UNSUPPORTED, "changes its width, height or first texel", variant(image, "s", textures=tex))
    tex = image.textures.copy()
    tex["kind"][1], tex["spectrum"][1], tex["reserved"][1] = abi.TEX_CHECKER_SPECTRUM, (0, 1), (0, 0, 0)
    refuse(plain, UNSUPPORTED, "a texture changes its kind", variant(image, "k", textures=tex))
    assert_same_snapshot(snapshot(plain)[0], before, "after the refusals")
    inst = base_scene("instanced")
    both = contexts(RGB, 0, DYNAMIC | INSTANCED)
    both.upload_scene(inst)
    before = snapshot(both, True)[0]
    light, spectrum = emitter_of(inst)
    grey = int(inst.triangles["material"][inst.instances["first_triangle"][-1]])
    refuse(both, UNSUPPORTED, "instanced triangles must not emit", variant(inst, "e", materials=emitting(inst, [light, grey], spectrum)))
    assert_same_snapshot(snapshot(both, True)[0], before, "after the refusals")
