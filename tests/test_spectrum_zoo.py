"""The device's spectrum evaluation (evalSpectrum, slr_amd/csrc/pt_bsdf.h; tables by prepareSpectra, scene_prep.cpp) on the edge-case
spectra of scenes.spectrum_zoo: irregular spectra with and without the one-byte cell table (at most 255 samples / more), spectra that
begin or end inside the visible range or lie outside it, sample wavelengths exactly on tabulated ones, 32 samples inside one 1-nm
cell of the table (a walk of 32 steps), regular spectra narrower and wider than [360, 830] nm, upsampled spectra of 0, 3 and 4
points.

CPU: the oracle against the compiled reference bit for bit, both against a float64 restatement within a derived bound, and which of
the two zoos fits the shade kernels' LDS tables.  GPU: slrhip_bsdf_queries, whole frames in both table placements (wavefront and
tail kernel) and the spectral albedo against the golden of the compiled reference (tests/golden/spectrum_zoo_kat.npz) and the oracle,
bit for bit: Lambert and the specular conductor call no float libm.

Sizes that decide the placement (floats of the spectrum pool, limit kLdsPoolFloats = 6144): irr_dense700 1400, reg_wide 1000 and its
scaled copy 1000, irr_low300 and irr_on_samples300 600 each, irr_256 512, irr_255 510 + 118 for its cell table, irr_cluster 74 + 118,
every upsampled spectrum 384, D65 531.  spectrum_zoo(True): 4852 floats + 7 cell tables = 5692 with their padding, 21 materials, 4
light triangles, 20 records, no texture -> staged in LDS.  spectrum_zoo(False): 9452 floats + 7 cell tables = 10292 ->
read from HBM (and the checker texture selects the HBM kernels by itself).

Deliberate breaks of evalSpectrum, tried in scratch builds on MI355X (not committed): reading cellWords[(cell + 1) >> 2] fails all
four GPU tests here (both placements of the frames: the staged copy of the table is read) — and 28 spectral tests of the older
suite; ending the table-less binary search at hi = n - 1 fails the query, HBM-frame and albedo tests here on irr_low300 and nothing
in the older suite; `<=` for `<` in the table-less forward walk fails the query test on irr_on_samples300 (and two floats of the
LDS frame, where a sample wavelength met a tabulated one of irr_256 by chance) and nothing in the older suite.  Starting the
search at lo = 1 changes no result for any input: a lower bound of 0 and of 1 both give lowIdx = 0, and t <= 0 returns values[0]
either way.  On a host transcription of the branch, `<=` in the search itself and a search begun at lo = 2 differ from the golden
only on irr_on_samples300, and a table walk capped at two steps only on irr_cluster."""
import os
import re

import numpy as np
import pytest

from helpers import assert_bit_equal, load_golden, scene_from_golden
from oracle import binding as ob
from slr_amd import abi, scenes

F = np.float32
U = 2.0 ** -24                      # unit roundoff of binary32


def lds_limits():
    """The sizes of the shade kernels' LDS tables, read from their definitions in slr_amd/csrc/pt_kernels.h."""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slr_amd", "csrc", "pt_kernels.h")).read()
    out = {}
    for key, name in (("materials", "kLdsMaterials"), ("lights", "kLdsLights"), ("spectra", "kLdsSpectra"), ("pool", "kLdsPoolFloats")):
        found = re.findall(r"static const int %s = (\d+);" % name, text)
        assert len(found) == 1, name
        out[key] = int(found[0])
    return out


LDS_LIMITS = lds_limits()


@pytest.fixture(scope="module")
def zoo():
    return scenes.spectrum_zoo(False)


@pytest.fixture(scope="module")
def golden():
    return load_golden("spectrum_zoo_kat")


# ---- the float64 restatement --------------------------------------------------------------------------------------------------
def piecewise_linear(sc, index, wavelengths):
    """Clamped piecewise-linear interpolation of a REGULAR or IRREGULAR spectrum record in float64 at the given (float32) wavelengths.
    Returns (value, bound, max(|v_lo|, |v_hi|)): bound = 4u max(|v_lo|, |v_hi|) — three float32 roundings of t and the blend — and for a regular
    spectrum + |v_hi - v_lo| (n - 1) 4u, because its bin position is itself rounded (relative error about 3u at a magnitude of up
    to n - 1).  v_lo, v_hi: the tabulated neighbours of the wavelength; beyond an end both are the end's value."""
    rec = sc.spectra[index]
    n, at = int(rec["num_samples"]), int(rec["data_offset"])
    wl = np.asarray(wavelengths, F).astype(np.float64)
    if int(rec["kind"]) == abi.SPEC_REGULAR:
        v = sc.spectrum_data[at:at + n].astype(np.float64)
        lo_l, hi_l = float(F(rec["lambda_min"])), float(F(rec["lambda_max"]))
        pos = np.clip((wl - lo_l) / (hi_l - lo_l) * (n - 1), 0.0, n - 1.0)
        lo = np.minimum(np.floor(pos).astype(np.int64), n - 1)
        hi = np.minimum(lo + 1, n - 1)
        t = pos - lo
        slope = np.abs(v[hi] - v[lo]) * (n - 1) * 4 * U
    else:
        assert int(rec["kind"]) == abi.SPEC_IRREGULAR
        lam = sc.spectrum_data[at:at + n].astype(np.float64)
        v = sc.spectrum_data[at + n:at + 2 * n].astype(np.float64)
        hi = np.clip(np.searchsorted(lam, wl, side="left"), 0, n - 1)          # first sample at or above the wavelength
        lo = np.where(wl <= lam[0], 0, np.where(wl >= lam[-1], n - 1, hi - 1))
        hi = np.where(wl <= lam[0], 0, hi)
        with np.errstate(invalid="ignore", divide="ignore"):
            t = np.where(hi > lo, (wl - lam[lo]) / (lam[hi] - lam[lo]), 0.0)
        slope = 0.0
    value = (1.0 - t) * v[lo] + t * v[hi]
    largest = np.maximum(np.abs(v[lo]), np.abs(v[hi]))
    return value, 4 * U * largest + slope, largest


def sampled_names(specs):
    return [n for n in specs if n.startswith(("irr_", "reg_"))]


# ---- CPU ----------------------------------------------------------------------------------------------------------------------
def test_zoo_holds_what_it_claims(zoo):
    sc, specs, mats = zoo
    lds, lds_specs, lds_mats = scenes.spectrum_zoo(True)
    assert set(specs) - set(lds_specs) == set(scenes.SPECTRUM_ZOO_LARGE)
    assert {int(sc.spectra["reserved"][specs[n]]) for n in specs if n.startswith("up_")} == {0, 3, 4}
    for name, s in specs.items():
        rec = sc.spectra[s]
        n, at = int(rec["num_samples"]), int(rec["data_offset"])
        if name.startswith("irr_"):
            lam = sc.spectrum_data[at:at + n]
            assert (np.diff(lam) > 0).all(), name
        if name in lds_specs:                                               # the shared spectra are the same numbers in both zoos
            other = lds.spectra[lds_specs[name]]
            size = {abi.SPEC_REGULAR: n, abi.SPEC_IRREGULAR: 2 * n, abi.SPEC_UPSAMPLED: 4 + 4 * n}[int(rec["kind"])]
            assert sc.spectrum_data[at:at + size].tobytes() == lds.spectrum_data[int(other["data_offset"]):int(other["data_offset"]) + size].tobytes(), name
    assert [int(sc.spectra["num_samples"][specs[n]]) for n in ("irr_dense700", "irr_256", "irr_255", "irr_2")] == [700, 256, 255, 2]
    # every sample wavelength of the special offsets is a tabulated wavelength of irr_on_samples, 830 nm among them
    rec = sc.spectra[specs["irr_on_samples"]]
    lam = sc.spectrum_data[int(rec["data_offset"]):int(rec["data_offset"]) + int(rec["num_samples"])]
    for off in scenes.SPECTRUM_ZOO_OFFSETS:
        assert np.isin(scenes.sample_wavelengths(off), lam).all()
    assert scenes.sample_wavelengths(scenes.SPECTRUM_ZOO_OFFSETS[3])[15] == F(830.0) and lam[-1] == F(830.0)
    # materials: the mirror's eta and k are the two spectra without a cell table; both emitters and the checker are there
    m = sc.materials[mats["mirror"]]
    assert int(m["type"]) == abi.MAT_METAL and [int(v) for v in m["spectrum"][1:]] == [specs["irr_dense700"], specs["irr_256"]]
    assert int(sc.materials[mats["emit_irr_256"]]["emittance"]) == specs["irr_256"]
    assert int(sc.materials[mats["emit_reg_wide"]]["emittance"]) == specs["reg_wide_emitted"]
    tex = sc.textures[-2 - int(sc.materials[mats["checker"]]["spectrum"][0])]
    assert [int(v) for v in tex["spectrum"]] == [specs["irr_255"], specs["irr_dense700"]]
    for name, s in specs.items():
        if name != "reg_wide_emitted":
            assert int(sc.materials[mats["matte_" + name]]["spectrum"][0]) == s


def cell_tables(sc):
    """{spectrum index: the 472 bytes} as prepareSpectra builds them: lower_bound of 360 + j in the wavelengths, for irregular
    spectra of at most 255 samples."""
    out = {}
    for i, rec in enumerate(sc.spectra):
        n, at = int(rec["num_samples"]), int(rec["data_offset"])
        if int(rec["kind"]) == abi.SPEC_IRREGULAR and n <= 255:
            out[i] = np.searchsorted(sc.spectrum_data[at:at + n], (F(360.0) + np.arange(472, dtype=F)).astype(F), side="left")
    return out


def table_sizes(sc):
    """What packShadeTables compares with the LDS limits: material records, light triangles, spectrum records and the pool with the
    118-float cell tables appended, each at a multiple of four floats, and the end padded to one."""
    pool = len(sc.spectrum_data)
    for _ in cell_tables(sc):
        pool += -pool % 4
        pool += 472 // 4
    pool += -pool % 4
    lights = int((sc.materials["emittance"][sc.triangles["material"]] >= 0).sum())
    return dict(materials=len(sc.materials), lights=lights, spectra=len(sc.spectra), pool=pool)


def test_table_placement():
    """spectrum_zoo(True) is within all four LDS limits and has neither a texture nor a MultiBSDF (either selects the kernels that
    read the tables from HBM); spectrum_zoo(False) is over the pool limit.  Measured: pool 5692 of 6144 floats against 10292; 21 / 27
    materials, 4 / 6 light triangles, 20 / 25 spectrum records.  irr_256 has no cell table in either, irr_255 has one, and byte 255 —
    the largest a table can hold — occurs in it."""
    lds, lds_specs, _ = scenes.spectrum_zoo(True)
    hbm, hbm_specs, _ = scenes.spectrum_zoo(False)
    a, b = table_sizes(lds), table_sizes(hbm)
    print("LDS zoo", a, "HBM zoo", b)
    assert all(a[k] <= LDS_LIMITS[k] for k in LDS_LIMITS), a
    assert len(lds.textures) == 0 and not (lds.materials["type"] == abi.MAT_MULTI).any()
    assert any(b[k] > LDS_LIMITS[k] for k in LDS_LIMITS), b
    assert len(hbm.spectrum_data) > LDS_LIMITS["pool"]                       # before any table
    for sc, specs in ((lds, lds_specs), (hbm, hbm_specs)):
        tables = cell_tables(sc)
        assert specs["irr_256"] not in tables and specs["irr_255"] in tables
        t = tables[specs["irr_255"]]
        assert t.max() == 255 and t.min() == 0 and (np.diff(t) >= 0).all()
        # irr_cluster: one 1-nm cell holds the whole cluster, and at lambda_1 of offset 0 (389.375 nm, above the cluster in the same
        # cell) the device's walk from the table's entry to the lower bound is as many steps long
        assert specs["irr_cluster"] in tables
        rec = sc.spectra[specs["irr_cluster"]]
        lam = sc.spectrum_data[int(rec["data_offset"]):][:int(rec["num_samples"])]
        t = tables[specs["irr_cluster"]]
        assert np.diff(t).max() == scenes.SPECTRUM_ZOO_CLUSTER
        wl = scenes.sample_wavelengths(0.0)[1]
        cell = int(F(wl - F(360.0)))
        assert wl == F(389.375) and cell == 29
        assert int(np.searchsorted(lam, wl, side="left")) - int(t[cell]) == scenes.SPECTRUM_ZOO_CLUSTER
        # ... and at most two steps for every other spectrum with a table
        for other, tt in tables.items():
            if other != specs["irr_cluster"]:
                assert np.diff(tt).max() <= 2
    assert hbm_specs["irr_dense700"] not in cell_tables(hbm)


def test_oracle_equals_the_compiled_reference_on_every_spectrum(zoo, oracle_spectral, ref_spectral):
    """slr_oracle_eval_spectrum against slr_ref_eval_spectrum (the reference's own ContinuousSpectrum::evaluate) on every zoo spectrum
    at the four special offsets and 64 seeded random ones: every float bit-equal, none NaN."""
    sc, specs, _ = zoo
    offsets = scenes.spectrum_zoo_offsets(64, 19)
    for name, s in specs.items():
        want = ref_spectral.eval_spectrum(sc, s, offsets)
        got = oracle_spectral.eval_spectrum(sc, s, offsets)
        assert not np.isnan(want).any() and not np.isnan(got).any(), name
        assert got.view(np.uint32).tobytes() == want.view(np.uint32).tobytes(), name
        assert (want != 0).any() == (name not in ("up_black", "up_outside")), name


def test_sampled_spectra_against_float64_interpolation(zoo, golden, oracle_spectral):
    """The regular and irregular spectra against clamped piecewise-linear interpolation in float64 at the float32 wavelengths, within
    the bound of piecewise_linear: first the compiled reference's values (the golden's `eval`), then the oracle's.

    Measured worst |value - float64| / (u max(|v_lo|, |v_hi|)), u = 2^-24, over the 68 offsets of the golden, reference and oracle
    alike (they are bit-equal): irr_dense700 1.68, irr_256 1.79, irr_255 1.84, irr_2 1.60, irr_inside 1.45, irr_on_samples 1.74,
    irr_cluster 1.47, irr_on_samples300 1.55, irr_below, irr_above and irr_low300 0 (clamped to an end value), reg_2 1.30,
    reg_narrow 0.83, reg_exact 7.16, reg_wide and its scaled copy 384.  As a share of the bound: at most 0.46 for the irregular
    spectra (bound 4), 0.18 reg_2, 0.08 reg_narrow, 0.25 reg_exact, 0.12 reg_wide."""
    sc, specs, _ = zoo
    offsets = golden["offsets"]
    wl = np.stack([scenes.sample_wavelengths(off) for off in offsets])
    index_of = {str(n): k for k, n in enumerate(golden["spectrum_names"])}
    for name in sampled_names(specs):
        want, bound, largest = (a.reshape(wl.shape) for a in piecewise_linear(sc, specs[name], wl.reshape(-1)))
        for who, got in (("reference", golden["eval"][index_of[name]]), ("oracle", oracle_spectral.eval_spectrum(sc, specs[name], offsets))):
            err = np.abs(got.astype(np.float64) - want)
            print("%s %s: worst %.3g u max(|v_lo|, |v_hi|), worst error / bound %.3g" % (name, who, float((err / (U * largest)).max()), float((err / bound).max())))
            assert (err <= bound).all(), (name, who, float((err - bound).max()))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def zoo_context(golden):
    from slr_amd import Context
    c = Context(device=0, mode=abi.MODE_SPECTRAL, stripes=1)
    c.upload_scene(scene_from_golden(golden))
    yield c
    c.close()


def lambert_scene(values, offsets):
    """A scene with one matte material per (row of `values`, offset) whose reflectance evaluates, at that offset, to exactly the row:
    an irregular spectrum tabulated at the offset's own 16 wavelengths (t = 1 at every sample but the first, where the reference
    returns the first value).  Returns (scene, material indices [rows][offsets])."""
    b = scenes.SceneBuilder()
    scenes.cornell_walls(b)
    mats = np.zeros(values.shape[:2], np.int64)
    for i in range(values.shape[0]):
        for k, off in enumerate(offsets):
            mats[i, k] = b.matte(b.spectrum_irregular(scenes.sample_wavelengths(off), values[i, k]))
    return b.build(scenes.cornell_camera(1.0), name="lambert_of_values"), mats


@pytest.mark.gpu
def test_bsdf_queries_on_every_spectrum_match_golden_and_oracle(golden, zoo_context, oracle_spectral):
    """slrhip_bsdf_queries (the device functions k_shade calls, tables in HBM) on the matte material of every zoo spectrum and on the
    mirror with the two table-less spectra as eta and k: the whole answer bit-equal to the compiled reference's at every offset of
    the golden and to the oracle's at 64 fresh offsets; and fs(evaluate) of each matte bit-equal to what the oracle's Lambert lobe
    makes of the reference's ContinuousSpectrum::evaluate values (the golden's `eval`) — the device's spectrum values themselves."""
    sc = scene_from_golden(golden)
    orc = oracle_spectral.scene(sc)
    q, offsets = golden["queries"], golden["offsets"]
    fresh = scenes.spectrum_zoo_offsets(64, 4711)[len(scenes.SPECTRUM_ZOO_OFFSETS):]
    with_answers = {str(n): int(m) for n, m in zip(golden["material_names"], golden["material_indices"])}
    mattes = {str(n): int(m) for n, m in zip(golden["matte_names"], golden["matte_indices"])}
    assert "mirror" in with_answers and len(mattes) == len(golden["spectrum_names"]) - 1 and len(with_answers) == len(mattes) - 2
    at_golden_offsets = {}
    for name, m in {**mattes, **with_answers}.items():
        got = at_golden_offsets[name] = np.stack([zoo_context.bsdf_queries(m, q, float(off), 0.5) for off in offsets])
        if name in with_answers:                  # (irr_low300, irr_on_samples300 and irr_cluster have no stored answers: below)
            assert_bit_equal(got, golden["out_" + name], name + " vs golden")
            assert (golden["out_" + name][:, :, 3] != 0).any(), name
        got = np.stack([zoo_context.bsdf_queries(m, q, float(off), 0.5) for off in fresh])
        want = np.stack([orc.bsdf_kat(m, q, float(off), 0.5) for off in fresh])
        assert_bit_equal(got, want, name + " vs oracle, fresh offsets")
    # the spectrum values, through the oracle's Lambert
    values = golden["eval"][golden["matte_spectra"]]
    lam_sc, lam_mats = lambert_scene(values, offsets)
    lam = oracle_spectral.scene(lam_sc)
    lo, hi = 5 + 16, 5 + 32                                                   # fs(evaluate), slr_oracle.h
    for i, name in enumerate(mattes):
        assert str(golden["spectrum_names"][golden["matte_spectra"][i]]) == name[len("matte_"):]
        for k, off in enumerate(offsets):
            want = lam.bsdf_kat(int(lam_mats[i, k]), q, float(off), 0.5)[:, lo:hi]
            got = at_golden_offsets[name][k][:, lo:hi]
            assert_bit_equal(got, want, "%s offset %r: fs(evaluate) vs Lambert of the reference's values" % (name, float(off)))
            if values[i, k].any():
                assert want.any(), name                                       # some query has both directions on the upper side


def _render(sc, st, spp, flags):
    from slr_amd import Context
    c = Context(mode=abi.MODE_SPECTRAL, stripes=1, flags=flags | abi.FLAG_TIME_KERNELS)
    try:
        fb = c.render_image(sc, st, spp)
        ctr, prof = c.counters(), c.profile()
        return fb, (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), int(prof.launches[2])
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fit_lds", [True, False], ids=["lds", "hbm"])
def test_frames_in_both_table_placements(oracle_spectral, fit_lds):
    """Whole frames of the zoo: spectrum_zoo(True) through the kernels that stage materials, spectrum records and the pool — cell
    tables included — in LDS, spectrum_zoo(False) with the tables in HBM, the emitters and the checker of two irregular spectra;
    each with the wavefront schedule and through the tail kernel.  Bit-equal to the oracle's frame, the same ray counts."""
    sc, _, _ = scenes.spectrum_zoo(fit_lds)
    assert all(table_sizes(sc)[k] <= LDS_LIMITS[k] for k in LDS_LIMITS) == fit_lds
    st = ob.settings(48, 36, seed=830)
    want, ctr = oracle_spectral.scene(sc).render(st, 4)
    assert want.sum() > 0
    counts = (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays))
    cases = [("wavefront", 0, 0)]
    if os.environ.get("SLRHIP_TAIL_SLOTS") != "0":           # (an environment can switch the tail kernel off: test_gpu_parity.py)
        cases.append(("tail kernel", abi.FLAG_TAIL_KERNEL, 1))
    for what, flags, tails in cases:
        fb, got_counts, launches = _render(sc, st, 4, flags)
        assert launches == tails, (what, launches)
        assert got_counts == counts, (what, got_counts, counts)
        assert_bit_equal(fb, want, "%s, %s" % (sc.name, what))
        assert fb.sum() > 0


@pytest.mark.gpu
def test_spectral_albedo_is_the_spectrum_at_the_samples_wavelengths(zoo, oracle_rgb, oracle_spectral):
    """One albedo pass over the whole zoo: at every pixel whose first hit is the matte material of a spectrum, the 16 components are
    the oracle's evaluation of that spectrum at the sample's own wavelength offset (the fourth float of its stream), bit for bit.
    The fold reads the HBM copy of the pool.  Pixels land on irr_dense700 and irr_256, the spectra that are searched."""
    from slr_amd import binding
    from test_albedo import ids_of_pass, one_albedo_pass
    sc, specs, mats = zoo
    spectrum_of = {mats["matte_" + n]: (n, s) for n, s in specs.items() if n != "reg_wide_emitted"}
    w, h = 48, 36
    st = ob.settings(w, h, seed=23)
    rgb, ctx = binding.Context(), binding.Context(mode=abi.MODE_SPECTRAL)
    seen = {}
    try:
        rgb.upload_scene(sc)
        ctx.upload_scene(sc)
        _, material = ids_of_pass(rgb, st, 0)
        got = one_albedo_pass(ctx, st, 0)
        for y, x in zip(*np.nonzero(np.isin(material, list(spectrum_of)))):
            name, s = spectrum_of[int(material[y, x])]
            offset = oracle_rgb.rng(abi.sample_seed(st.rng_seed, int(x), int(y), 0), 4)[1][3]
            want = oracle_spectral.eval_spectrum(sc, s, [offset])[0]
            assert_bit_equal(got[y, x], want, "%s at pixel (%d, %d), offset %r" % (name, x, y, float(offset)))
            seen[name] = seen.get(name, 0) + 1
        assert ctx.features_status() == 0
    finally:
        rgb.close()
        ctx.close()
    assert seen.get("irr_dense700", 0) >= 1 and seen.get("irr_256", 0) >= 1, seen
    assert len(seen) == len(spectrum_of), sorted(set(n for n, _ in spectrum_of.values()) - set(seen))
