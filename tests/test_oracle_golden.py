"""CPU: the oracle (restatement) against the golden vectors produced by the compiled
reference (tests/golden/make_golden.py).  Bit-exact: every float of every framebuffer."""
import numpy as np
import pytest

from helpers import assert_bit_equal, load_golden, scene_from_golden
from oracle import binding as ob
from slr_amd import abi

SCENES = ["rgb_tiny_box", "rgb_cornell_glass", "rgb_cornell_matte", "rgb_oren_nayar", "rgb_ggx_metal", "rgb_ggx_glass", "rgb_ward", "rgb_ashikhmin",
          "rgb_ibl", "rgb_ibl_area",
          "rgb_multi", "rgb_multi_libm_free",
          "rgb_textured"]     # checkerboard reflectance + bump-mapped sphere + alpha-cut quad     # environment sphere alone / next to a triangle light (Scene::selectLight)


def test_rng_known_answers(oracle_rgb):
    # seed 1509761209 -> 1775644678, 2835251161, 3125706222 (XORShiftRNG.cpp:21-36)
    u, f = oracle_rgb.rng(abi.DEFAULT_SEED, 3)
    assert u.tolist() == [1775644678, 2835251161, 3125706222]
    assert np.allclose(f, [0.413424, 0.660133, 0.72776], atol=1e-6)
    g = load_golden("rng_kat")
    for i, seed in enumerate(g["seeds"]):
        u, f = oracle_rgb.rng(int(seed), 64)
        assert (u == g["uints_%d" % i]).all()
        assert_bit_equal(f, g["floats_%d" % i], "floats seed %d" % seed)
        assert (f >= 0).all() and (f < 1).all()


def test_sample_seed_contract():
    import ctypes as C
    vals = [abi.sample_seed(abi.DEFAULT_SEED, x, y, s) for x, y, s in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1279, 719, 1023)]]
    assert len(set(vals)) == len(vals)
    assert all(-2**31 <= v < 2**31 for v in vals)


@pytest.mark.parametrize("name", SCENES)
def test_frame_matches_reference(oracle_rgb, name):
    g = load_golden(name)
    sc = oracle_rgb.scene(scene_from_golden(g))
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    fb, ctr = sc.render(st, int(g["spp"]), threads=0)
    assert ctr.samples == int(g["width"]) * int(g["height"]) * int(g["spp"])
    assert_bit_equal(fb, g["framebuffer"], name + " framebuffer")
    assert fb.sum() > 0


@pytest.mark.parametrize("name", SCENES)
def test_continued_render_equals_single_render(oracle_rgb, name):
    """spp/2 + spp/2 with carried Kahan state == spp in one go (sensor accumulation order)."""
    g = load_golden(name)
    sc = oracle_rgb.scene(scene_from_golden(g))
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    half = int(g["spp"]) // 2
    s0 = np.zeros_like(g["framebuffer"])
    state = (s0, np.zeros_like(s0))
    sc.render(st, half, 0, state=state, threads=2)
    assert_bit_equal(state[0], g["framebuffer_half"], name + " half")
    sc.render(st, half, half, state=state, threads=3)
    assert_bit_equal(state[0], g["framebuffer"], name + " resumed")


@pytest.mark.parametrize("name", SCENES)
def test_single_samples_match_reference(oracle_rgb, name):
    g = load_golden(name)
    sc = oracle_rgb.scene(scene_from_golden(g))
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    for (x, y, p), want in zip(g["sample_picks"], g["sample_values"]):
        got = sc.sample(st, int(x), int(y), int(p))
        assert_bit_equal(got, want, "%s sample (%d,%d,%d)" % (name, x, y, p))


@pytest.mark.parametrize("name", SCENES)
def test_closest_hits_match_reference(oracle_rgb, name):
    g = load_golden(name)
    sc = oracle_rgb.scene(scene_from_golden(g))
    hits = sc.trace(g["rays"])
    want = g["hits"]
    assert (hits["triangle"] == want["triangle"]).all()
    hit = want["triangle"] != 0xFFFFFFFF
    assert hit.sum() > 50      # the open IBL scene (a floor and a sphere) stops 58 of the 512 rays
    for f in ("dist", "b0", "b1"):
        assert_bit_equal(hits[f][hit], want[f][hit], name + " " + f)


@pytest.mark.parametrize("name", SCENES)
def test_serial_mode_matches_unmodified_reference_render(oracle_rgb, name):
    """One xorshift stream over all pixels and passes = PathTracingRenderer::render with one worker."""
    g = load_golden(name)
    sc = oracle_rgb.scene(scene_from_golden(g))
    st = ob.settings(int(g["serial_width"]), int(g["serial_height"]), int(g["seed"]))
    fb, _ = sc.render_serial(st, int(g["serial_spp"]))
    assert_bit_equal(fb, g["serial_framebuffer"], name + " serial")


def test_shards_partition_the_image(oracle_rgb):
    g = load_golden("rgb_cornell_matte")
    sc = oracle_rgb.scene(scene_from_golden(g))
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    total = np.zeros_like(g["framebuffer"])
    for i in range(3):
        fb, _ = sc.render(st, int(g["spp"]), shard=(i, 3))
        assert ((total != 0) & (fb != 0)).sum() == 0      # disjoint supports
        total += fb
    assert_bit_equal(total, g["framebuffer"], "sum of shards")


def test_rejects_bad_scene(oracle_rgb):
    g = load_golden("rgb_tiny_box")
    sc = scene_from_golden(g)
    with pytest.raises(ValueError):
        abi.Scene(sc.vertices[:2], sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera)


SPECTRAL_SCENES = ["spectral_cornell_glass", "spectral_cornell_matte", "spectral_oren_nayar", "spectral_ggx_metal", "spectral_ggx_glass", "spectral_ashikhmin",
                   "spectral_ibl", "spectral_multi", "spectral_multi_libm_free",
                   "spectral_boxes", "spectral_textured"]   # BASELINE configs[2]: Cornell_Box_Boxes-shaped, GGX titanium box, spectral build     # environment texels as (u, v, s), looked up in the Meng-15 grid at run time, + an area light


@pytest.mark.parametrize("name", SPECTRAL_SCENES)
def test_spectral_frame_matches_reference(oracle_spectral, name):
    """16 wavelength samples, upsampled / regular / irregular input spectra, 16-bin storage: every float of the frame."""
    g = load_golden(name)
    sc = oracle_spectral.scene(scene_from_golden(g))
    assert sc.components == 16
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    fb, _ = sc.render(st, int(g["spp"]), threads=0)
    assert fb.shape[2] == 16
    assert_bit_equal(fb, g["framebuffer"], name + " framebuffer")
    for (x, y, p), want in zip(g["sample_picks"][:24], g["sample_values"][:24]):
        assert_bit_equal(sc.sample(st, int(x), int(y), int(p)), want, "%s sample (%d,%d,%d)" % (name, x, y, p))
    st2 = ob.settings(int(g["serial_width"]), int(g["serial_height"]), int(g["seed"]))
    fs, _ = sc.render_serial(st2, int(g["serial_spp"]))
    assert_bit_equal(fs, g["serial_framebuffer"], name + " serial")


def procedural_scene(g):
    """Fixtures of scenes too large to store hold the generator's name and arguments; the checksum pins the arrays."""
    import zlib
    from slr_amd import scenes
    a = g["generator_args"]
    sc = getattr(scenes, str(g["generator"]))(int(a[0]), float(a[1]))
    assert (zlib.crc32(sc.vertices.tobytes()) ^ zlib.crc32(sc.triangles.tobytes())) == int(g["scene_crc"]), "generator output changed"
    assert len(sc.triangles) == int(g["num_triangles"])
    # the small tables are stored: the fixture's frame was rendered with exactly these materials and spectra
    assert sc.materials.tobytes() == g["materials"].tobytes() and sc.spectra.tobytes() == g["spectra"].tobytes()
    assert sc.spectrum_data.tobytes() == g["spectrum_data"].tobytes()
    return sc


def test_displaced_grid_matches_reference(oracle_rgb):
    """BASELINE configs[4]'s shape (320 002 triangles, thin lens r = 0.025) against the compiled reference (SBVH.h:417-442,
    TriangleMesh.cpp:131-178): all 2 048 closest hits bit-equal; the frame bit-equal except where two triangles are hit at
    the SAME distance (a shared edge): the reference keeps the last one its tree tested, the oracle the larger scene index
    (deliberate difference 2) — 6 of 43 200 floats on this frame."""
    g = load_golden("rgb_grid400")
    sc = oracle_rgb.scene(procedural_scene(g))
    hits, want = sc.trace(g["rays"]), g["hits"]
    assert (hits["triangle"] == want["triangle"]).all()
    hit = want["triangle"] != 0xFFFFFFFF
    assert hit.sum() > 1000
    for f in ("dist", "b0", "b1"):
        assert_bit_equal(hits[f][hit], want[f][hit], "grid " + f)
    fb, ctr = sc.render(ob.settings(int(g["width"]), int(g["height"]), int(g["seed"])), int(g["spp"]), threads=0)
    w = g["framebuffer"]
    exact = (fb.view(np.uint32) == w.view(np.uint32)) | ((fb == 0) & (w == 0))
    assert exact.mean() >= 0.9995, exact.mean()
    assert np.sqrt(np.mean((fb.astype(np.float64) - w) ** 2)) <= 1e-3 * w.mean()


# ---- function-level known answers: BSDF::sample / evaluate / evaluatePDF per lobe ------------------------
@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_bsdf_known_answers(oracle_rgb, oracle_spectral, mode):
    """The reference's BSDF objects, queried on both sides of the surface, with tilted geometric normals, grazing,
    retro, mirror and straight-through directions and sample numbers at 0 and 1 - ulp: every float of every answer."""
    g = load_golden("bsdf_kat_" + mode)
    sc = (oracle_rgb if mode == "rgb" else oracle_spectral).scene(scene_from_golden(g))
    C = sc.components
    for name, m in zip(g["material_names"], g["material_indices"]):
        for w, (off, ul) in enumerate(g["wavelengths"]):
            got = sc.bsdf_kat(int(m), g["queries"], float(off), float(ul))
            want = g["out_" + str(name)][w]
            assert got.shape == want.shape == (len(g["queries"]), 6 + 2 * C)
            assert_bit_equal(got, want, "%s %s wl %d" % (mode, name, w))
    # the fixture exercises what it claims to: every lobe samples and evaluates to something on a good share of the rows
    for name in g["material_names"]:
        o = g["out_" + str(name)][0]
        assert (o[:, 3] != 0).mean() > 0.75, name
        if str(name) not in ("mirror", "glass"):            # delta lobes evaluate to zero (basic_BSDFs.cpp:73-80,151-158)
            assert (o[:, 5 + C:5 + 2 * C] != 0).any(axis=1).mean() > 0.25, name
        else:
            assert not o[:, 5 + C:].any(), name


@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_image_textured_frame_matches_reference(oracle_rgb, oracle_spectral, mode):
    """Image textures in material slots (ImageSpectrumTexture, image_textures.cpp:13-79): a repeated image on the floor, one wrapped
    round a sphere, one as a mirror's coefficient.  The golden comes from the compiled reference with the texel addressing
    restated in the shim (the reference's class needs OpenEXR half: parity of that one step is unpinned), everything after the
    texel — mapping, UpsampledContinuousSpectrum::evaluate in the spectral build, the material — is the reference's own."""
    lib = oracle_rgb if mode == "rgb" else oracle_spectral
    f = load_golden(mode + "_image_textured")
    fb, _ = lib.scene(scene_from_golden(f)).render(ob.settings(int(f["width"]), int(f["height"]), int(f["seed"])), int(f["spp"]), threads=0)
    assert_bit_equal(fb, f["framebuffer"], mode + " image-textured frame")
    assert f["framebuffer"].sum() > 0


@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_instanced_frame_hits_and_samples_match_reference(oracle_rgb, oracle_spectral, mode):
    """Instanced meshes (slrhip_instance): the golden comes from the compiled reference's own TransformedSurfaceObjects over mesh
    aggregates (Core/SurfaceObject.cpp:303-392) — rotations, non-uniform scales, a mirror among the instanced materials.  Whole
    frame, single samples and closest hits (distance and barycentrics through the un-normalised local ray) bit for bit."""
    lib = oracle_rgb if mode == "rgb" else oracle_spectral
    f = load_golden(mode + "_instanced")
    sc = scene_from_golden(f)
    assert len(sc.instances) == 6 and len(np.unique(sc.instances["first_triangle"])) == 2      # two meshes, six placements
    s = lib.scene(sc)
    st = ob.settings(int(f["width"]), int(f["height"]), int(f["seed"]))
    fb, _ = s.render(st, int(f["spp"]), threads=0)
    assert_bit_equal(fb, f["framebuffer"], mode + " instanced frame")
    for (x, y, p), want in zip(f["sample_picks"], f["sample_values"]):
        assert_bit_equal(s.sample(st, int(x), int(y), int(p)), want, "sample")
    hits = s.trace(f["rays"])
    assert (hits["triangle"] == f["hits"]["triangle"]).all()
    for k in ("dist", "b0", "b1"):
        assert_bit_equal(hits[k], f["hits"][k], k)
    first = int(sc.instances["first_triangle"].min())
    hit = f["hits"]["triangle"] != 0xFFFFFFFF
    assert (f["hits"]["triangle"][hit] >= first).mean() > 0.05           # the fixture does exercise the instances


@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_nested_multibsdf_known_answers_and_frame(oracle_rgb, oracle_spectral, mode):
    """A summed / mixed material whose components are summed / mixed materials: the reference builds a MultiBSDF of MultiBSDFs
    (SummedSurfaceMaterial.cpp:13-20, MixedSurfaceMaterial.cpp:14-22) and MultiBSDF.cpp:20-59,125-212 then calls itself through
    the BSDF interface.  Every float of sample / evaluate / evaluatePDF on six nested materials (two to four lobes, an
    InverseBSDF and a two-sided delta lobe among them), and a whole frame, against the compiled reference's answers."""
    lib = oracle_rgb if mode == "rgb" else oracle_spectral
    g = load_golden("bsdf_kat_nested_" + mode)
    sc = lib.scene(scene_from_golden(g))
    C = sc.components
    for name, m in zip(g["material_names"], g["material_indices"]):
        for w, (off, ul) in enumerate(g["wavelengths"]):
            got = sc.bsdf_kat(int(m), g["queries"], float(off), float(ul))
            want = g["out_" + str(name)][w]
            assert got.shape == want.shape == (len(g["queries"]), 6 + 2 * C)
            assert_bit_equal(got, want, "%s %s wl %d" % (mode, name, w))
        assert (g["out_" + str(name)][0][:, 3] != 0).mean() > 0.75, name
    f = load_golden(mode + "_multi_nested")
    fb, ctr = lib.scene(scene_from_golden(f)).render(ob.settings(int(f["width"]), int(f["height"]), int(f["seed"])), int(f["spp"]), threads=0)
    assert_bit_equal(fb, f["framebuffer"], mode + " nested frame")
    assert f["framebuffer"].sum() > 0


@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_bsdf_queries_match_compiled_reference(request, oracle_rgb, oracle_spectral, mode):
    """Same comparison against the compiled reference itself on fresh random queries (container only)."""
    from slr_amd import scenes
    ref_lib = request.getfixturevalue("ref_" + mode)
    scene, mats = scenes.material_zoo()
    nested_scene, nested = scenes.material_zoo_nested()
    on, rn = (oracle_rgb if mode == "rgb" else oracle_spectral).scene(nested_scene), ref_lib.scene(nested_scene)
    qn = scenes.bsdf_queries(1024, 99)
    for name, m in nested.items():
        assert_bit_equal(on.bsdf_kat(m, qn, 0.25, 0.8), rn.bsdf_kat(m, qn, 0.25, 0.8), "%s nested %s" % (mode, name))
    o = (oracle_rgb if mode == "rgb" else oracle_spectral).scene(scene)
    r = ref_lib.scene(scene)
    q = scenes.bsdf_queries(1024, 7)
    for name, m in mats.items():
        assert_bit_equal(o.bsdf_kat(m, q, 0.25, 0.8), r.bsdf_kat(m, q, 0.25, 0.8), "%s %s" % (mode, name))


@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_light_sampling_known_answers(oracle_rgb, oracle_spectral, mode):
    """Scene::selectLight + Light::sample (PathTracingRenderer.cpp:169-177) of the reference: which light, its probability,
    the sampled point, normal, shading frame, area PDF and emittance — environment sphere (importance-map inversion, lat-long
    mapping) next to triangle lights, and several triangle lights; sample numbers 0 and 1 - 2^-24 included."""
    g = load_golden("light_kat_" + mode)
    lib = oracle_rgb if mode == "rgb" else oracle_spectral
    off, ul = [float(v) for v in g["wavelengths"]]
    for tag in ("env", "zoo"):
        sc = lib.scene(scene_from_golden(g, prefix=tag + "_"))
        got = sc.light_kat(g["queries"], off, ul)
        assert_bit_equal(got, g[tag + "_out"], "%s %s" % (mode, tag))
    env_picks = (g["env_out"][:, 0] < 0).mean()
    assert 0.2 < env_picks < 0.5            # 1 / (1 + number of triangle lights) of the selection samples
    assert len(np.unique(g["zoo_out"][:, 0])) > 2


def test_spectrum_zoo_known_answers(oracle_spectral):
    """Edge-case spectra (scenes.spectrum_zoo; tests/golden/spectrum_zoo_kat.npz from the compiled spectral reference): its
    ContinuousSpectrum::evaluate on every spectrum — irregular with 2 to 700 samples, inside / outside the visible range, sample
    wavelengths on tabulated ones, regular narrower and wider than [360, 830], upsampled with 0, 3 and 4 points — at offsets 0, 0.37,
    0.5, 1 - 2^-24 and 64 random ones, and its BSDF answers for the matte material of every spectrum and a mirror with irregular eta
    and k: every float bit-equal, none NaN."""
    g = load_golden("spectrum_zoo_kat")
    scene = scene_from_golden(g)
    offsets = g["offsets"]
    assert [float(o) for o in offsets[:4]] == [0.0, float(np.float32(0.37)), 0.5, 1.0 - 2.0 ** -24] and len(offsets) == 68
    assert not np.isnan(g["eval"]).any()
    for name, s, want in zip(g["spectrum_names"], g["spectrum_indices"], g["eval"]):
        got = oracle_spectral.eval_spectrum(scene, int(s), offsets)
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), str(name)
    assert {int(scene.spectra["reserved"][s]) for n, s in zip(g["spectrum_names"], g["spectrum_indices"]) if str(n).startswith("up_")} == {0, 3, 4}
    sc = oracle_spectral.scene(scene)
    for name, m in zip(g["material_names"], g["material_indices"]):
        want = g["out_" + str(name)]
        got = np.stack([sc.bsdf_kat(int(m), g["queries"], float(off), 0.5) for off in offsets])
        assert_bit_equal(got, want, "spectrum zoo " + str(name))
        assert (want[:, :, 3] != 0).mean() > 0.5, name
