"""Scene classes in combination: instances, textures / bump / alpha, MultiBSDF, environment, glossy lobes and tables in HBM in ONE
scene (scenes.feature_mix), where every other render test has one of them at a time.  The device code picks its kernels and its
branches by scene class, and these mixes run the code where the classes meet: a textured component inside a MULTI material, bump
then instance transform, alpha cuts inside the instanced traversal, the environment's NEE and MIS through glossy and MULTI lobes.

CPU: the oracle against the compiled reference on all mixes in both modes (frames and aimed rays, bit for bit), every feature of
every mix shown to change the frame, the aimed rays shown to reach what they are aimed at.  GPU: frames at matched seeds against
the oracle (and the reference's goldens for the two largest mixes), the launch schedules against one another, and the three ray
query entry points on rays through the alpha-cut instances."""
import functools

import numpy as np
import pytest

from helpers import assert_bit_equal, libm_tolerance, load_golden, scene_from_golden
from oracle import binding as ob
from slr_amd import Context, abi, scenes

MIXES = {"A": ("inst", "tex"), "B": ("inst", "multi"), "C": ("tex", "multi"), "D": ("inst", "tex", "multi"),
         "E": ("env", "inst"), "F": ("env", "tex"), "G": ("env", "glossy", "many"), "H": ("env", "multi", "glossy"),
         "I": ("inst", "tex", "multi", "env", "glossy", "many")}
LIBM_FREE, LIBM = ("A", "B", "C", "D"), ("E", "F", "G", "H", "I")
MODES = ("rgb", "spectral")
GOLDEN = {"D": "mix_free", "I": "mix_all"}
WIDTH, HEIGHT, SPP, SEED = 48, 36, 8, 4712      # a seed at which every sample stays in its pixel: test_every_sample_stays_in_its_pixel
MISS = 0xFFFFFFFF
MIX_MODE = [(m, mode) for m in MIXES for mode in MODES]


def amode(mode):
    return abi.MODE_RGB if mode == "rgb" else abi.MODE_SPECTRAL


def settings():
    return ob.settings(WIDTH, HEIGHT, seed=SEED)


@functools.lru_cache(maxsize=None)
def mix_scene(features):
    return scenes.feature_mix(frozenset(features), WIDTH / HEIGHT)


@functools.lru_cache(maxsize=None)
def oracle_scene(features, mode):
    return ob.load("oracle", amode(mode)).scene(mix_scene(features))


@functools.lru_cache(maxsize=None)
def oracle_frame(features, mode):
    """(frame, counters) of the oracle at the tests' size and seed: computed once per (features, mode), shared, read-only."""
    fb, ctr = oracle_scene(features, mode).render(settings(), SPP)
    fb.setflags(write=False)
    return fb, ctr


def aimed_rays():
    rows = scenes.feature_mix_rays(512, 2025)
    rays = np.zeros(len(rows), ob.ray_dtype)
    rays["org"], rays["dist_min"], rays["dir"], rays["dist_max"] = rows[:, 0:3], rows[:, 3], rows[:, 4:7], rows[:, 7]
    return rows, rays


@functools.lru_cache(maxsize=None)
def oracle_hits(features):
    """The oracle's closest hits on the aimed rays (traversal and alpha test do not depend on the colour mode)."""
    hits = oracle_scene(features, "rgb").trace(aimed_rays()[1])
    hits.setflags(write=False)
    return hits


def instanced_mask(sc, tri):
    mesh = np.zeros(len(sc.triangles) + 1, bool)
    for rec in sc.instances:
        mesh[int(rec["first_triangle"]):int(rec["first_triangle"]) + int(rec["num_triangles"])] = True
    return mesh[np.where(tri == MISS, len(sc.triangles), tri)]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_generator_builds_what_it_says():
    everything = mix_scene(MIXES["I"])
    assert 200 < len(everything.triangles) < 1000
    assert len(everything.materials) > 32
    emitting = everything.materials["emittance"][everything.triangles["material"]] >= 0
    assert emitting.sum() > 16 and not instanced_mask(everything, np.arange(len(everything.triangles)))[emitting].any()
    assert len(everything.instances) == 6 and len(np.unique(everything.instances["first_triangle"])) == 2
    kinds = set(int(k) for k in everything.textures["kind"])
    assert kinds == {abi.TEX_CHECKER_SPECTRUM, abi.TEX_IMAGE_SPECTRUM, abi.TEX_CHECKER_NORMAL, abi.TEX_CHECKER_FLOAT}
    multi = everything.materials[everything.materials["type"] == abi.MAT_MULTI]
    assert (multi["reserved"] & 0xFFFF).any() and (multi["reserved"] >> 16).any()      # a MULTI record with a normal map, one with an alpha map
    assert everything.env is not None and everything.env_uvs is not None
    for key in ("B", "E", "G", "H"):
        assert mix_scene(MIXES[key]).textures is None or len(mix_scene(MIXES[key]).textures) == 0, key
    plain = mix_scene(MIXES["G"])
    assert len(plain.materials) > 32 and (plain.materials["type"] != abi.MAT_MULTI).all() and len(plain.instances) == 0
    for key in LIBM_FREE:
        types = set(int(t) for t in mix_scene(MIXES[key]).materials["type"])
        assert types <= {abi.MAT_MATTE, abi.MAT_METAL, abi.MAT_GLASS, abi.MAT_MULTI} and mix_scene(MIXES[key]).env is None, key
    a, b = scenes.feature_mix(MIXES["I"], 1.0), scenes.feature_mix(MIXES["I"], 1.0)      # deterministic
    assert a.vertices.tobytes() == b.vertices.tobytes() and a.materials.tobytes() == b.materials.tobytes()


def test_every_sample_stays_in_its_pixel():
    """The precondition of the frame comparison with the compiled reference.  ImageSensor::add adds at (uint32_t)p.x, and
    basePixelX + u rounds up to the next integer for u within half an ulp of it (about two samples in a million).  The oracle
    and the device keep such a sample in the pixel that drew it; the reference's sensor adds it to the neighbour, whose sums
    the shim's per-pixel render then overwrites.  Seed 4711 has one (pixel (42, 8), pass 6, p.x = 43.0), which showed as one
    differing pixel in every mix with an environment; the seed used here has none (positions are the same in every scene)."""
    s, st = oracle_scene(MIXES["A"], "rgb"), settings()
    for y in range(HEIGHT):
        for x in range(WIDTH):
            for p in range(SPP):
                px, py = s.sample(st, x, y, p)[3:5]
                assert (int(px), int(py)) == (x, y), (x, y, p, float(px), float(py))


@pytest.mark.parametrize("mix, mode", MIX_MODE)
def test_oracle_equals_compiled_reference(request, mix, mode):
    """The restatement against the reference's own classes on every mix: whole frames bit for bit, and the closest hits of the
    aimed rays (through the holes of the alpha-cut cubes, instanced or baked) equal in triangle, distance and barycentrics."""
    ref = request.getfixturevalue("ref_" + mode)
    sr = ref.scene(mix_scene(MIXES[mix]))
    fr, _ = sr.render(settings(), SPP)
    fo, _ = oracle_frame(MIXES[mix], mode)
    assert_bit_equal(fo, fr, "mix %s %s" % (mix, mode))
    assert np.isfinite(fo).all() and fo.sum() > 0
    ho, hr = oracle_scene(MIXES[mix], mode).trace(aimed_rays()[1]), sr.trace(aimed_rays()[1])
    assert (ho["triangle"] == hr["triangle"]).all(), int((ho["triangle"] != hr["triangle"]).sum())
    hit = hr["triangle"] != MISS
    assert hit.mean() > 0.5
    for k in ("dist", "b0", "b1"):
        assert_bit_equal(ho[k][hit], hr[k][hit], k)


@pytest.mark.parametrize("mix, mode", MIX_MODE)
def test_every_feature_is_live(mix, mode):
    """Taking any one feature out of a mix changes the oracle's frame: more than 1 % relative in at least 5 % of the pixels.
    A mix in which a feature did not show would test nothing of it."""
    fo = oracle_frame(MIXES[mix], mode)[0].astype(np.float64)
    for feature in MIXES[mix]:
        rest = tuple(f for f in MIXES[mix] if f != feature)
        fw = oracle_frame(rest, mode)[0].astype(np.float64)
        moved = (np.abs(fo - fw) > 0.01 * np.maximum(np.abs(fo), np.abs(fw))).any(axis=2)
        print(mix, mode, feature, "pixels moved: %.3f" % moved.mean())
        assert moved.mean() >= 0.05, (mix, mode, feature, float(moved.mean()))


@pytest.mark.parametrize("mix", [m for m in MIXES if "inst" in MIXES[m] or "tex" in MIXES[m]])
def test_aimed_rays_reach_the_instances_and_the_holes(mix):
    """The aimed rays do what random rays did not (7 % on instanced triangles, 0.2 % through a hole): at least 20 % have their
    closest hit on an instanced triangle, and at least 20 % get another answer once the alpha maps are stripped."""
    rows, rays = aimed_rays()
    assert len(rows) == 512 and np.isfinite(rows[:, 7]).sum() == 128
    sc = mix_scene(MIXES[mix])
    hits = oracle_hits(MIXES[mix])
    if "inst" in MIXES[mix]:
        on_instance = instanced_mask(sc, hits["triangle"])
        print(mix, "closest hit on an instanced triangle: %.3f" % on_instance.mean())
        assert on_instance.mean() >= 0.2
    if "tex" in MIXES[mix]:
        stripped = scenes.feature_mix(frozenset(MIXES[mix]), WIDTH / HEIGHT)
        assert (stripped.materials["reserved"] >> 16).any()
        stripped.materials["reserved"] &= 0xFFFF
        solid = ob.load("oracle").scene(stripped).trace(rays)
        changed = solid["triangle"] != hits["triangle"]
        print(mix, "another answer without the alpha maps: %.3f" % changed.mean())
        assert changed.mean() >= 0.2


@pytest.mark.parametrize("mix, mode", [(m, mode) for m in GOLDEN for mode in MODES])
def test_oracle_equals_the_mix_goldens(mix, mode):
    """The two committed mixes (the compiled reference's frames, single samples and closest hits on the aimed rays)."""
    g = load_golden(mode + "_" + GOLDEN[mix])
    sc = scene_from_golden(g)
    s = ob.load("oracle", amode(mode)).scene(sc)
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    fb, _ = s.render(st, int(g["spp"]), threads=0)
    assert_bit_equal(fb, g["framebuffer"], "%s mix %s frame" % (mode, mix))
    for (x, y, p), want in zip(g["sample_picks"], g["sample_values"]):
        assert_bit_equal(s.sample(st, int(x), int(y), int(p)), want, "sample")
    assert np.array_equal(g["rays"], aimed_rays()[1])
    hits = s.trace(g["rays"])
    assert (hits["triangle"] == g["hits"]["triangle"]).all()
    hit = g["hits"]["triangle"] != MISS
    for k in ("dist", "b0", "b1"):
        assert_bit_equal(hits[k][hit], g["hits"][k][hit], k)
    assert instanced_mask(sc, g["hits"]["triangle"]).mean() >= 0.2


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def gpu_render(sc, st, calls, mode, stripes=1, flags=0, shard=(0, 1)):
    """frame, (samples, extension rays, shadow rays), tail launches, samples started from the primary pass's record"""
    c = Context(mode=amode(mode), stripes=stripes, flags=flags)
    try:
        c.upload_scene(sc)
        c.render_begin(st, shard)
        for begin, count in calls:
            c.render(begin, count)
        fb = c.read_framebuffer()
        ctr, prof = c.counters(), c.profile()
        return fb, (int(ctr.samples), int(ctr.extension_rays), int(ctr.shadow_rays)), int(prof.launches[2]), c.primary_samples()
    finally:
        c.close()


def golden_frame(mix, mode, flags=0):
    g = load_golden(mode + "_" + GOLDEN[mix])
    st = ob.settings(int(g["width"]), int(g["height"]), int(g["seed"]))
    fb, counts, _, _ = gpu_render(scene_from_golden(g), st, ((0, int(g["spp"])),), mode, flags=flags)
    assert counts[0] == int(g["width"]) * int(g["height"]) * int(g["spp"])
    return fb, g["framebuffer"]


@pytest.mark.gpu
@pytest.mark.parametrize("mix, mode", [(m, mode) for m in LIBM_FREE for mode in MODES])
def test_libm_free_mix_equals_the_oracle_bit_for_bit(mix, mode):
    """No float libm on any path of these mixes (fmod in the texture mappings aside, which is exact): the frame equals the
    oracle's bit for bit with one slot per pixel and with the automatic slot count, every sample is rendered once, and both ray
    counts are the oracle's.  Mix D also against the compiled reference's golden."""
    want, ctr = oracle_frame(MIXES[mix], mode)
    for stripes in (1, 0):
        fb, counts, _, _ = gpu_render(mix_scene(MIXES[mix]), settings(), ((0, SPP),), mode, stripes=stripes)
        assert_bit_equal(fb, want, "mix %s %s, stripes %d, vs the oracle" % (mix, mode, stripes))
        assert counts[0] == WIDTH * HEIGHT * SPP == int(ctr.samples)
        assert counts[1:] == (int(ctr.extension_rays), int(ctr.shadow_rays)), (mix, mode, stripes, counts)
    if mix in GOLDEN:
        fb, golden = golden_frame(mix, mode)
        assert_bit_equal(fb, golden, "mix %s %s vs the reference's golden" % (mix, mode))


def libm_floor(mix, mode):
    """The floor of helpers.libm_tolerance for a mix, from the floors the suite already holds for each libm-calling feature alone
    (test_gpu_parity.TOL): a float may leave the 2e-6 band through any of them, so the shortfalls add.
    within = 1 - sum(1 - TOL[k]): env -> *_ibl, glossy -> *_ggx_metal, a MULTI with a GGX component -> *_multi."""
    from test_gpu_parity import TOL
    f = MIXES[mix]
    keys = (["ibl"] if "env" in f else []) + (["ggx_metal"] if "glossy" in f else []) + (["multi"] if "multi" in f and "glossy" in f else [])
    return 1.0 - sum(1.0 - TOL[mode + "_" + k] for k in keys)


def test_libm_floors_are_the_stated_ones():
    want = {"E": (0.9995, 0.9995), "F": (0.9995, 0.9995), "G": (0.9975, 0.9975), "H": (0.9965, 0.9970), "I": (0.9965, 0.9970)}
    for mix, (rgb, spectral) in want.items():
        assert abs(libm_floor(mix, "rgb") - rgb) < 1e-12 and abs(libm_floor(mix, "spectral") - spectral) < 1e-12, mix


@pytest.mark.gpu
@pytest.mark.parametrize("mix, mode", [(m, mode) for m in LIBM for mode in MODES])
def test_libm_mix_within_tolerance_of_the_oracle(mix, mode):
    """Float libm on the path (the environment's acosf / atan2f / sinf / cosf, the GGX lobes): helpers.libm_tolerance with the
    floor of libm_floor, the RMSE on frames clipped at 10 x the mean as in the environment tests; every sample rendered once,
    ray counts within 1e-4 of the oracle's.  Mix I also against the compiled reference's golden.  The figures measured on
    MI355X are in profiles/r17_feature_mix_parity_stats.jsonl."""
    want, ctr = oracle_frame(MIXES[mix], mode)
    fb, counts, _, _ = gpu_render(mix_scene(MIXES[mix]), settings(), ((0, SPP),), mode)
    libm_tolerance(fb, want, "feature mix %s %s vs oracle" % (mix, mode), within=libm_floor(mix, mode), cap=10)
    assert counts[0] == WIDTH * HEIGHT * SPP == int(ctr.samples)
    assert abs(counts[1] - int(ctr.extension_rays)) <= ctr.extension_rays * 1e-4, (counts, int(ctr.extension_rays))
    assert abs(counts[2] - int(ctr.shadow_rays)) <= ctr.shadow_rays * 1e-4, (counts, int(ctr.shadow_rays))
    if mix in GOLDEN:
        fb, golden = golden_frame(mix, mode)
        libm_tolerance(fb, golden, "feature mix %s %s vs reference golden" % (mix, mode), within=libm_floor(mix, mode), cap=10)


@pytest.mark.gpu
@pytest.mark.parametrize("mix, mode", [(m, mode) for m in GOLDEN for mode in MODES])
def test_schedules_give_the_same_frame(mix, mode):
    """Device code against device code, so bit for bit even with libm on the path: the tail kernel against the wavefront
    iterations (one slot per pixel; the profile shows that the tail ran), a render cut into two calls against one, two shards
    summed against the whole frame; RGB mix D: the primary pass against SLRHIP_FLAG_NO_PRIMARY_PASS, every sample started from
    the pass's record when it is on."""
    sc, st = mix_scene(MIXES[mix]), settings()
    timed = abi.FLAG_TIME_KERNELS
    whole = gpu_render(sc, st, ((0, SPP),), mode, flags=timed)
    assert whole[1][0] == WIDTH * HEIGHT * SPP and whole[2] == 0 and whole[0].sum() > 0
    tail = gpu_render(sc, st, ((0, SPP),), mode, flags=timed | abi.FLAG_TAIL_KERNEL)
    assert tail[2] == 1, tail[2]
    assert tail[1] == whole[1], (tail[1], whole[1])
    assert_bit_equal(tail[0], whole[0], "tail kernel vs wavefront iterations")
    two = gpu_render(sc, st, ((0, 3), (3, SPP - 3)), mode, flags=timed)
    assert two[1] == whole[1], (two[1], whole[1])
    assert_bit_equal(two[0], whole[0], "two render calls vs one")
    parts = [gpu_render(sc, st, ((0, SPP),), mode, flags=timed, shard=(rank, 2)) for rank in range(2)]
    assert tuple(sum(p[1][k] for p in parts) for k in range(3)) == whole[1]
    assert not ((parts[0][0] != 0) & (parts[1][0] != 0)).any()
    assert_bit_equal(parts[0][0] + parts[1][0], whole[0], "two shards vs the unsharded frame")
    if mix == "D" and mode == "rgb":
        off = gpu_render(sc, st, ((0, SPP),), mode, flags=timed | abi.FLAG_NO_PRIMARY_PASS)
        assert whole[3] == whole[1][0] and off[3] == 0, (whole[3], whole[1][0], off[3])
        assert off[1] == whole[1], (off[1], whole[1])
        assert_bit_equal(whole[0], off[0], "primary pass on vs off")


def expected_instances(sc, rows, tri, dist, b0, b1):
    """Which placement a hit lies on: the instance of the hit triangle's mesh whose transformed triangle holds org + dir * dist at
    (b0, b1).  The placements stand apart, so the nearest one is nearer than 1e-4 and every other is far."""
    want = np.full(len(rows), -1, np.int64)
    pos = sc.vertices["position"].astype(np.float64)
    for i in np.nonzero(instanced_mask(sc, tri))[0]:
        p = rows[i, 0:3].astype(np.float64) + rows[i, 4:7].astype(np.float64) * float(dist[i])
        v = pos[sc.triangles["v"][tri[i]]]
        local = float(b0[i]) * v[0] + float(b1[i]) * v[1] + (1.0 - float(b0[i]) - float(b1[i])) * v[2]
        err = []
        for rec in sc.instances:
            inside = int(rec["first_triangle"]) <= tri[i] < int(rec["first_triangle"]) + int(rec["num_triangles"])
            m = np.asarray(rec["local_to_world"], np.float64).reshape(4, 4).T
            err.append(np.linalg.norm(m[:3, :3] @ local + m[:3, 3] - p) if inside else np.inf)
        assert min(err) < 1e-4 and sorted(err)[1] > 1e-2, (i, err)
        want[i] = int(np.argmin(err))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("mix, mode", [(m, mode) for m in GOLDEN for mode in MODES])
def test_queries_through_alpha_cut_instances(mix, mode):
    """slrhip_trace_rays, slrhip_intersect_rays and slrhip_test_visibility on the aimed rays: alpha cuts INSIDE instances for all
    three traversal entry points.  Triangle, hit or miss and the instance equal the oracle's closest hits; dist, b0, b1 bit-equal
    on hits; visible exactly where the oracle misses."""
    sc = mix_scene(MIXES[mix])
    rows, _ = aimed_rays()
    want = oracle_hits(MIXES[mix])
    hit = want["triangle"] != MISS
    assert 0.2 < hit.mean() < 1.0 and instanced_mask(sc, want["triangle"]).mean() >= 0.2
    c = Context(mode=amode(mode))
    try:
        c.upload_scene(sc)
        tri, dist, b0, b1 = c.trace_rays(rows[:, 0:3], rows[:, 4:7], rows[:, 3], rows[:, 7])
        hits, inst = c.intersect_rays(rows, want_instances=True)
        vis = c.test_visibility(rows)
    finally:
        c.close()
    assert (tri == want["triangle"]).all(), int((tri != want["triangle"]).sum())
    qtri = np.ascontiguousarray(hits[:, 0]).view(np.uint32)
    assert (qtri == want["triangle"]).all(), int((qtri != want["triangle"]).sum())
    for k, batch, query in (("dist", dist, hits[:, 1]), ("b0", b0, hits[:, 2]), ("b1", b1, hits[:, 3])):
        assert_bit_equal(batch[hit], want[k][hit], "slrhip_trace_rays " + k)
        assert_bit_equal(query[hit], want[k][hit], "slrhip_intersect_rays " + k)
    assert (vis == (want["triangle"] == MISS)).all(), int((vis != (want["triangle"] == MISS)).sum())
    assert (inst == expected_instances(sc, rows, want["triangle"], want["dist"], want["b0"], want["b1"])).all()
