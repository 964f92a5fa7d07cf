"""The environment light from device memory (slrhip_set_environment) and its preprocessing on the host (slrhip_env_importance,
slrhip_env_texels_to_uvs).

CPU: the two host exports against the committed fixtures (written by the compiled reference) and, bit for bit, against the
repository's independent Python restatements (scenes.ibl_importance, ibl_importance_uvs, sky_to_uvs) on seeded half-valued images that
hold zeros, binary16 subnormals, block averages that are binary16 rounding ties, and 4 094 (a block sum of 65 504); every refusal.

GPU: the importance map and the sampling tables built on the device equal the host's in every bit (the yardstick of the tables is a
fresh slrhip_upload_scene with the Python importance map: numpy's sin stays out of it); a context whose environment was swapped
renders, bit for bit, what a context freshly uploaded with that environment renders, and swapping back gives the first frame back;
the flags; the refusals change nothing; feature and query calls never see the environment."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal, bits, load_golden
from oracle import binding as ob
from slr_amd import abi, binding, scenes
from slr_amd.binding import Context, DeviceBlocks, SlrHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, NO_SCENE, UNSUPPORTED = 1, 4, 5
SIZES = [(4, 4), (64, 32), (264, 132)]           # width x height; maps 1x1, 16x8, 66x33 (wider than a wave, odd row count, partial tiles)


def half(a):
    with np.errstate(over="ignore"):                 # beyond 65504: infinity, as the reference's image
        return np.asarray(a, F).astype(np.float16).astype(F)


@functools.lru_cache(maxsize=None)
def seeded_rgb(width, height, seed=0):
    """A seeded half-valued (r, g, b) image with the special values planted block by block (a block = one map cell)."""
    rng = np.random.default_rng(1000 * width + height + seed)
    t = half(rng.uniform(0.0, 4.0, (height, width, 3)) ** 3)
    t[rng.random((height, width)) < 0.05] = 0.0                       # black texels: the b == 0 branch of the uvs conversion
    t[0, 0] = 0.0
    blocks = [(by, bx) for by in range(height // 4) for bx in range(width // 4)]
    rng.shuffle(blocks)

    def block(k):
        by, bx = blocks[k % len(blocks)]
        return t[4 * by:4 * by + 4, 4 * bx:4 * bx + 4]
    if len(blocks) >= 6:
        block(0)[:] = 4094.0                                          # sum 65 504, average 4 094
        block(1)[:] = half(rng.integers(0, 40, (4, 4, 3)) * 2.0 ** -24)      # binary16 subnormals (and zeros)
        b = block(2); b[:] = 1.0; b[1, 2] = 1.0 + 2.0 ** -7           # average 1 + 2^-11: a tie, to even = down
        b = block(3); b[:] = 1.0; b[2, 1] = 1.0 + 3 * 2.0 ** -7       # average 1 + 3 * 2^-11: a tie, to even = up
        block(4)[:] = 0.0                                             # a black cell
        b = block(5); b[:] = 2.0 ** -24; b[0, 0] = 0.0                # average 15/16 of the smallest subnormal: rounds to it
    else:
        t[1, 2] = (4094.0, 2.0 ** -24, 1.0 + 2.0 ** -7)
    assert (half(t) == t).all()
    return t


def scale_of(width, height):
    return 0.5 + 0.25 * (width % 7)


# ---------------------------------------------------------------- CPU --------------------------------------------------------------------
def test_exports_and_struct_layout():
    lib = binding.load_library()
    for name in ("slrhip_set_environment", "slrhip_env_importance", "slrhip_env_texels_to_uvs", "slrhip_debug_environment_check",
                 "slrhip_debug_environment"):
        assert name in binding.EXPORTS and hasattr(lib, name)
    d = abi.EnvironmentDesc
    assert C.sizeof(d) == 32 and (d.width.offset, d.height.offset, d.texels.offset, d.scale.offset, d.flags.offset, d.reserved.offset) == (0, 4, 8, 16, 20, 24)
    assert (abi.ENV_TEXELS_RGB, abi.ENV_STORE_HALF) == (1, 2)
    text = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert "#define SLRHIP_ENV_TEXELS_RGB 1u" in text and "#define SLRHIP_ENV_STORE_HALF 2u" in text


@pytest.mark.parametrize("name", ["rgb_ibl", "rgb_ibl_area", "spectral_ibl"])
def test_importance_equals_the_reference_fixtures(name):
    g = load_golden(name)
    assert_bit_equal(binding.env_importance(g["env_texels"], abi.MODE_RGB), g["env_importance"], name + " env_importance")
    if name == "spectral_ibl":
        assert_bit_equal(binding.env_importance(g["env_texels_uvs"], abi.MODE_SPECTRAL), g["env_importance_uvs"], "env_importance_uvs")
        assert_bit_equal(binding.env_texels_to_uvs(g["env_texels"]), g["env_texels_uvs"], "env_texels_uvs")


@pytest.mark.parametrize("width, height", [(4, 4), (8, 4), (64, 32)])
def test_host_exports_equal_the_python_restatements(width, height):
    rgb = seeded_rgb(width, height)
    assert_bit_equal(binding.env_importance(rgb, abi.MODE_RGB), scenes.ibl_importance(rgb), "RGB importance")
    uvs = scenes.sky_to_uvs(rgb)
    got = binding.env_texels_to_uvs(rgb)
    assert np.array_equal(bits(got), bits(uvs)), "uvs: %d texel components differ" % (bits(got) != bits(uvs)).sum()
    black = (rgb == 0).all(axis=2)
    assert black.any() and (got[black][:, 2] == 0).all()
    with np.errstate(all="ignore"):
        assert_bit_equal(binding.env_importance(uvs, abi.MODE_SPECTRAL), scenes.ibl_importance_uvs(uvs), "spectral importance")
    in_place = rgb.copy()                                             # rgb and uvs may be the same array
    lib = binding.load_library()
    assert lib.slrhip_env_texels_to_uvs(in_place.ctypes.data, width * height, in_place.ctypes.data) == 0
    assert np.array_equal(bits(in_place), bits(uvs))


def test_special_values_are_what_the_definition_says():
    """The planted blocks, by hand: 4 094 stays 4 094; the two ties go to even; 15/16 of the smallest subnormal rounds up to it."""
    lum = lambda a: F(F(F(0.222485) * a + F(0.716905) * a) + F(0.060610) * a)
    for fill, one, want in ((4094.0, 4094.0, 4094.0), (1.0, 1.0 + 2.0 ** -7, 1.0), (1.0, 1.0 + 3 * 2.0 ** -7, 1.0 + 2.0 ** -9),
                            (2.0 ** -24, 0.0, 2.0 ** -24), (0.0, 0.0, 0.0)):
        t = np.full((4, 4, 3), fill, F)
        t[1, 2] = one
        got = binding.env_importance(t, abi.MODE_RGB)
        assert got.shape == (1, 1) and bits(got)[0, 0] == bits(lum(F(want))), (fill, one, got)


def test_host_export_refusals_write_nothing():
    lib = binding.load_library()
    t = seeded_rgb(8, 4)
    out = np.full(8, -7.0, F)
    ok = (abi.MODE_RGB, t.ctypes.data, 8, 4, out.ctypes.data, 2)
    for k, bad in ((0, 2), (0, -1), (1, None), (4, None), (2, 6), (2, 0), (2, 32772), (3, 2), (3, 0), (3, 32772), (5, 1)):
        args = list(ok)
        args[k] = bad
        assert lib.slrhip_env_importance(*args) == INVALID, (k, bad)
        assert (out == -7.0).all(), (k, bad)
    assert lib.slrhip_env_importance(*ok) == 0 and (out[:2] != -7.0).all() and (out[2:] == -7.0).all()
    uvs = np.full((2, 3), -7.0, F)
    assert lib.slrhip_env_texels_to_uvs(None, 2, uvs.ctypes.data) == INVALID
    assert lib.slrhip_env_texels_to_uvs(t.ctypes.data, 2, None) == INVALID
    assert (uvs == -7.0).all()
    with pytest.raises(ValueError):
        binding.env_importance(np.zeros((6, 8, 3), F))


def test_descriptor_check_refusals():
    """environmentRefusal (render_plan.cpp) through slrhip_debug_environment_check: the pointer is only compared, never followed."""
    lib = binding.load_library()

    def check(width=8, height=4, texels=0x10000, scale=1.0, flags=0, reserved=(0, 0)):
        return lib.slrhip_debug_environment_check(C.byref(abi.EnvironmentDesc(width, height, texels, scale, flags, (C.c_uint32 * 2)(*reserved))))
    assert check() == 0 and check(32768, 32768, flags=3, scale=0.0) == 0
    for over in (dict(width=6), dict(width=0), dict(height=2), dict(height=7), dict(width=32772), dict(height=65536), dict(texels=None),
                 dict(texels=0x10004), dict(texels=0x10008), dict(flags=4), dict(flags=0x80000001), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
                 dict(scale=float("nan")), dict(scale=float("inf")), dict(scale=-1.0)):
        assert check(**over) == INVALID, over
        assert b"slrhip_set_environment" in lib.slrhip_last_error_string()
    assert lib.slrhip_debug_environment_check(None) == INVALID
    assert lib.slrhip_set_environment(None, None, None) == INVALID


def test_host_program_parses_the_flags():
    from slr_amd import host
    args = host.build_parser().parse_args(["scene.txt", "--environment", "sky.npy", "--environment-scale", "2.5"])
    assert args.environment == "sky.npy" and args.environment_scale == 2.5
    assert host.build_parser().parse_args(["scene.txt"]).environment is None


def test_host_program_environment_tuple(tmp_path):
    """The tuple the host program hands to load_scene: the image rounded to binary16, and the importance maps and uvs texels of the
    two C exports, which equal the Python restatements."""
    from slr_amd import host
    rgb = seeded_rgb(8, 4) * F(1.0003)                                # not half-representable
    path = str(tmp_path / "sky.npy")
    np.save(path, rgb)
    env = host.environment_from_file(path, 2.0, spectral=True)
    assert len(env) == 5 and env[1] == 2.0
    assert np.array_equal(env[0], half(rgb))
    assert_bit_equal(env[2], scenes.ibl_importance(half(rgb)), "importance")
    assert np.array_equal(bits(env[3]), bits(scenes.sky_to_uvs(half(rgb))))
    with np.errstate(all="ignore"):
        assert_bit_equal(env[4], scenes.ibl_importance_uvs(env[3]), "importance uvs")
    assert len(host.environment_from_file(path, 1.0, spectral=False)) == 3


# ---------------------------------------------------------------- GPU --------------------------------------------------------------------
SPP = 8


def settings(seed=9):
    return ob.settings(32, 32, seed=seed)


@functools.lru_cache(maxsize=None)
def environment(width, height, seed=0):
    """(rgb, scale, importance, uvs, importance_uvs): the tuple SceneBuilder.build takes, from the Python restatements, computed once."""
    rgb = seeded_rgb(width, height, seed)
    uvs = scenes.sky_to_uvs(rgb)
    with np.errstate(all="ignore"):
        return (rgb, scale_of(width, height), scenes.ibl_importance(rgb), uvs, scenes.ibl_importance_uvs(uvs))


def with_env(sc, env):
    return abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, env, sc.name, textures=sc.textures,
                     texture_texels=sc.texture_texels, texture_texels_uvs=sc.texture_texels_uvs, instances=sc.instances)


@functools.lru_cache(maxsize=None)
def base_scene(kind):
    if kind == "cornell":
        return scenes.cornell_box_spheres(1.0, 8, 4, "glass")
    return scenes.ibl_test_scene(1.0, (64, 32), 8, 4, area_light=(kind == "ibl_area"))


def native(env, mode):
    """The texels slrhip_envmap::texels holds for the mode."""
    return env[3] if mode == abi.MODE_SPECTRAL else env[0]


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(mode, which=0):
        if (mode, which) not in made:
            made[(mode, which)] = Context(device=0, mode=mode, stripes=1)
        return made[(mode, which)]
    yield get
    for c in made.values():
        c.close()


def tables(ctx, whats=(0, 2, 3, 4, 5)):
    return {w: ctx.debug_environment(w) for w in whats}


def assert_same_tables(got, want, what):
    assert got.keys() == want.keys()
    for w in got:
        assert got[w].shape == want[w].shape, (what, w)
        differ = bits(got[w]) != bits(want[w])
        assert not differ.any(), "%s: read-out %d: %d of %d floats differ" % (what, w, differ.sum(), differ.size)


def render(ctx, seed=9):
    ctx.render_begin(settings(seed))
    ctx.render(0, SPP)
    c = ctx.counters()
    return ctx.read_framebuffer(), (c.samples, c.extension_rays, c.shadow_rays)


MODES = [pytest.param(abi.MODE_RGB, id="rgb"), pytest.param(abi.MODE_SPECTRAL, id="spectral")]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("width, height", SIZES)
def test_importance_map_and_tables_equal_the_host_path(contexts, mode, width, height):
    env = environment(width, height)
    ctx, fresh = contexts(mode), contexts(mode, 1)
    ctx.upload_scene(base_scene("ibl"))
    ctx.set_environment(native(env, mode), env[1])
    want_map = env[4] if mode == abi.MODE_SPECTRAL else env[2]
    got_map = ctx.debug_environment(1)
    assert got_map.shape == (height // 4, width // 4)
    assert_bit_equal(got_map, want_map, "importance map %dx%d" % (width, height))
    got = tables(ctx)
    fresh.upload_scene(with_env(base_scene("ibl"), env))
    assert_same_tables(got, tables(fresh), "%dx%d" % (width, height))
    assert np.array_equal(bits(got[0]), bits(native(env, mode)))
    with pytest.raises(SlrHipError, match=r"\(1\).*keeps no importance map"):
        fresh.debug_environment(1)                                    # the host path keeps no map


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["ibl", "ibl_area", "cornell"])
def test_swapped_environment_renders_what_a_fresh_upload_renders(contexts, kind, mode):
    env_a, env_b = environment(64, 32, seed=1), environment(264, 132)
    assert env_a[1] != env_b[1]
    ctx, fresh = contexts(mode), contexts(mode, 1)
    base = base_scene(kind)
    if kind == "cornell":
        ctx.upload_scene(base, upsampling=True)                       # no environment yet; a spectral context gets the tables for later
        with pytest.raises(SlrHipError):
            ctx.debug_environment(2)
    else:
        ctx.upload_scene(with_env(base, env_a))
    first, first_counters = render(ctx)
    ctx.set_environment(native(env_b, mode), env_b[1])
    got, got_counters = render(ctx)
    fresh.upload_scene(with_env(base, env_b))
    want, want_counters = render(fresh)
    assert np.array_equal(bits(got), bits(want)), "%d of %d floats differ" % ((bits(got) != bits(want)).sum(), got.size)
    assert got_counters == want_counters
    assert not np.array_equal(bits(got), bits(first)) and np.isfinite(got).all() and got.max() > 0
    assert_same_tables(tables(ctx), tables(fresh), kind)
    if kind != "cornell":
        ctx.set_environment(native(env_a, mode), env_a[1])            # the larger arrays are kept: a smaller map in them
        again, again_counters = render(ctx)
        assert np.array_equal(bits(again), bits(first)) and again_counters == first_counters


@pytest.mark.gpu
def test_rgb_texels_flag_in_a_spectral_context(contexts):
    env = environment(64, 32)
    ctx, fresh = contexts(abi.MODE_SPECTRAL), contexts(abi.MODE_SPECTRAL, 1)
    for c, texels, rgb in ((ctx, env[0], True), (fresh, env[3], False)):
        c.upload_scene(base_scene("ibl"))
        c.set_environment(texels, env[1], rgb=rgb)
    assert_same_tables(tables(ctx, range(6)), tables(fresh, range(6)), "rgb=True")
    a, b = render(ctx), render(fresh)
    assert np.array_equal(bits(a[0]), bits(b[0])) and a[1] == b[1]
    # an RGB context ignores the bit
    r = contexts(abi.MODE_RGB)
    r.upload_scene(base_scene("ibl"))
    r.set_environment(env[0], env[1], rgb=True)
    got = tables(r, range(6))
    r.set_environment(env[0], env[1])
    assert_same_tables(got, tables(r, range(6)), "RGB context")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_store_half_flag(contexts, mode):
    env = environment(64, 32)
    raw = (env[0] * F(1.0003) + F(1e-9)).astype(F)
    raw[0, 1] = (70000.0, 65519.0, 65520.0)                           # beyond 65504: infinity from 65520 on, as the reference's image
    assert (half(raw) != raw).mean() > 0.5
    spectral = mode == abi.MODE_SPECTRAL
    ctx, fresh = contexts(mode), contexts(mode, 1)
    for c, texels, flag in ((ctx, raw, True), (fresh, half(raw), False)):
        c.upload_scene(base_scene("ibl"))
        c.set_environment(texels, env[1], rgb=spectral, store_half=flag)
    got = tables(ctx, range(6))
    assert_same_tables(got, tables(fresh, range(6)), "store_half")
    if not spectral:
        assert np.array_equal(bits(got[0]), bits(half(raw))) and np.isinf(got[0][0, 1]).tolist() == [True, False, True]


@pytest.mark.gpu
def test_refusals_change_nothing(contexts):
    lib = binding.load_library()
    env = environment(64, 32)
    empty = Context(device=0, mode=abi.MODE_RGB, stripes=1)
    try:
        with pytest.raises(SlrHipError, match=r"slrhip_set_environment failed \(%d\)" % NO_SCENE):
            empty.set_environment(env[0], 1.0)
    finally:
        empty.close()
    sctx = contexts(abi.MODE_SPECTRAL)
    sctx.upload_scene(base_scene("cornell"))                          # uploaded without the upsampling tables
    with pytest.raises(SlrHipError, match=r"slrhip_set_environment failed \(%d\)" % UNSUPPORTED):
        sctx.set_environment(env[3], 1.0)

    ctx = contexts(abi.MODE_RGB)
    ctx.upload_scene(with_env(base_scene("ibl"), env))
    before, before_counters = render(ctx)
    before_tables = tables(ctx)
    with DeviceBlocks() as dev:
        p = dev.put(np.concatenate([env[0].reshape(-1), np.zeros(64, F)]))

        def call(width=64, height=32, texels=p, scale=3.0, flags=0, reserved=(0, 0)):
            d = abi.EnvironmentDesc(width, height, texels, scale, flags, (C.c_uint32 * 2)(*reserved))
            return lib.slrhip_set_environment(ctx.handle, C.byref(d), None)
        for over in (dict(width=6), dict(texels=p + 4), dict(reserved=(0, 7)), dict(scale=float("nan")), dict(texels=None), dict(flags=8),
                     dict(scale=-0.5), dict(height=30)):
            assert call(**over) == INVALID, over
            assert b"slrhip_set_environment" in lib.slrhip_last_error_string()
        assert lib.slrhip_set_environment(ctx.handle, None, None) == INVALID
        ctx.synchronize()
    after, after_counters = render(ctx)
    assert np.array_equal(bits(after), bits(before)) and after_counters == before_counters
    assert_same_tables(tables(ctx), before_tables, "after the refusals")
    with pytest.raises(ValueError):
        ctx.debug_environment(6)


@pytest.mark.gpu
def test_features_and_queries_do_not_see_the_environment(contexts):
    env_a, env_b = environment(64, 32, seed=1), environment(264, 132)
    ctx = contexts(abi.MODE_RGB)
    ctx.upload_scene(with_env(base_scene("ibl"), env_a))
    ctx.render_begin(settings())
    rows, _ = ctx.camera_rays(0)

    def buffers():
        ctx.render_begin(settings())
        ctx.render_features(abi.FEATURE_ALL, 2)
        feats = [ctx.features(ch) for ch in sorted(abi.FEATURE_CHANNELS)]
        return feats + [ctx.intersect_rays(rows), ctx.test_visibility(rows)]
    before = buffers()
    ctx.set_environment(env_b[0], env_b[1])
    for a, b in zip(before, buffers()):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process: the check on a torch tensor runs in
# a fresh child process that imports torch BEFORE libslrhip.so is loaded.
@pytest.mark.gpu
def test_device_tensor_and_numpy_array_give_the_same_tables():
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_environment as T\nT._torch_check()\n" % (ROOT, os.path.join(ROOT, "tests")))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert "OK _torch_check" in p.stdout, p.stdout[-4000:] + "\n" + p.stderr[-3000:]


def _torch_check():
    import torch
    env = environment(264, 132)
    ctx = Context(device=0, mode=abi.MODE_RGB, stripes=1)
    try:
        ctx.upload_scene(base_scene("ibl"))
        ctx.set_environment(env[0], env[1])
        want = tables(ctx, range(6))
        ctx.set_environment(seeded_rgb(64, 32), 1.0)                  # something else in between
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            t = torch.from_numpy(env[0].copy()).cuda()
            ctx.set_environment(t, env[1], stream=side)
            t.zero_()                                                 # ordered after the call on the same stream: the library has its copy
        side.synchronize()
        assert_same_tables(tables(ctx, range(6)), want, "torch tensor")
        with pytest.raises(ValueError):
            ctx.set_environment(t[:, ::2], 1.0)                       # not contiguous
        print("OK _torch_check", flush=True)
    finally:
        ctx.close()
