"""New texels for one image texture of the uploaded scene, in place (slrhip_set_texture_texels).

The scene is cornell_image_textured: three images of 16 x 12, 8 x 8 and 6 x 4 texels whose first texels are 0, 192 and 256.  Each is
replaced in turn, from a torch tensor, in both modes; the yardstick is a context freshly uploaded with those texels, compared by bytes.
The neighbouring images must stay untouched, STORE_HALF must equal numpy's float16 round trip, and the call must work from a captured
graph."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from slr_amd import abi, binding, scenes
from slr_amd.binding import Context
from test_vertex_update import SPP, same_bytes, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INVALID, NO_SCENE = 1, 4
RGB, SPECTRAL = abi.MODE_RGB, abi.MODE_SPECTRAL
IMAGES = [(16, 12, 0), (8, 8, 192), (6, 4, 256)]          # width, height, first texel


@functools.lru_cache(maxsize=None)
def base_scene():
    sc = scenes.cornell_image_textured(1.0, 8, 4)
    assert [tuple(int(v) for v in t["reserved"]) for t in sc.textures] == IMAGES
    return sc


@functools.lru_cache(maxsize=None)
def replacement(texture):
    """(rgb, uvs) [h, w, 3] of another seed for image `texture`."""
    w, h, _ = IMAGES[texture]
    return scenes.synthetic_image(w, h, 20 + texture)


def with_texels(sc, texture, rgb, uvs):
    w, h, first = IMAGES[texture]
    a, b = sc.texture_texels.copy(), sc.texture_texels_uvs.copy()
    a[first:first + w * h], b[first:first + w * h] = rgb.reshape(-1, 3), uvs.reshape(-1, 3)
    return abi.Scene(sc.vertices, sc.triangles, sc.materials, sc.spectra, sc.spectrum_data, sc.camera, None, "%s_image%d" % (sc.name, texture),
                     textures=sc.textures, texture_texels=a, texture_texels_uvs=b)


def frame(ctx):
    ctx.render_begin(settings())
    ctx.render(0, SPP)
    return ctx.read_framebuffer()


def test_exports_and_flag():
    lib = binding.load_library()
    assert hasattr(lib, "slrhip_set_texture_texels") and "slrhip_set_texture_texels" in binding.EXPORTS
    assert abi.TEXELS_STORE_HALF == 1 and lib.slrhip_version() == 7
    assert lib.slrhip_set_texture_texels(None, 0, 4096, 0, None) == INVALID


# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process (test_ray_queries.py): the checks on
# torch tensors run in a fresh child process that imports torch BEFORE libslrhip.so is loaded.
def in_child(check, *args):
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_texture_update as T\nT.%s(*%r)\nprint('CHILD_OK')\n"
           % (ROOT, os.path.join(ROOT, "tests"), check, args))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CHILD_OK" in p.stdout, (check, p.returncode, p.stdout[-3000:], p.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [RGB, SPECTRAL])
def test_each_image_replaced_equals_a_fresh_upload(mode):
    in_child("_replace_check", mode)


def _replace_check(mode):
    import torch
    sc = base_scene()
    ctx, fresh = Context(device=0, mode=mode), Context(device=0, mode=mode)
    try:
        ctx.upload_scene(sc)
        stored = sc.texture_texels_uvs if mode == SPECTRAL else sc.texture_texels
        same_bytes(ctx.debug_materials()["texels"], stored, "the uploaded texels")
        now = sc
        for texture, (w, h, first) in enumerate(IMAGES):
            rgb, uvs = replacement(texture)
            now = with_texels(now, texture, rgb, uvs)
            before = ctx.debug_materials()["texels"]
            t = torch.from_numpy(np.ascontiguousarray(uvs if mode == SPECTRAL else rgb)).cuda()
            ctx.set_texture_texels(texture, t)
            got = ctx.debug_materials()["texels"]
            fresh.upload_scene(now)
            same_bytes(got, fresh.debug_materials()["texels"], "image %d: the texels against the fresh upload" % texture)
            outside = np.ones(len(got), bool)
            outside[first:first + w * h] = False
            same_bytes(got[outside], before[outside], "image %d: the other images' texels" % texture)
            assert not np.array_equal(got[~outside], before[~outside])
            mine, theirs = frame(ctx), frame(fresh)
            same_bytes(mine, theirs, "image %d: the frame against the fresh upload" % texture)
            assert np.isfinite(mine).all() and mine.max() > 0
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.gpu
def test_store_half_is_the_float16_round_trip_and_a_numpy_source_works():
    sc = base_scene()
    ctx = Context(device=0)
    try:
        ctx.upload_scene(sc)
        w, h, first = IMAGES[1]
        src = np.random.default_rng(3).uniform(0.0, 2.0, (h, w, 3)).astype(F)
        src[0, 0] = (70000.0, 65504.0, 65520.0)                     # beyond the largest half, the largest half, the tie that rounds to infinity
        src[0, 1] = (1.0e-7, 5.9604645e-8, 2.0e-8)                  # subnormal halves, and below half of the smallest one
        src[0, 2] = (-0.0, -1.0e-7, 1.0 / 3.0)
        ctx.set_texture_texels(1, src, store_half=True)
        got = ctx.debug_materials()["texels"]
        with np.errstate(over="ignore"):
            want = src.astype(np.float16).astype(F).reshape(-1, 3)
        assert np.isinf(want[0, 0]) and want[1, 0] != 0 and want[1, 2] == 0
        same_bytes(got[first:first + w * h], want, "STORE_HALF against numpy's float16")
        same_bytes(got[:first], sc.texture_texels[:first], "the image before")
        same_bytes(got[first + w * h:], sc.texture_texels[first + w * h:], "the image behind")
        ctx.set_texture_texels(1, src)
        same_bytes(ctx.debug_materials()["texels"][first:first + w * h], src.reshape(-1, 3), "without the flag the floats are stored as given")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_the_call_replays_from_a_captured_graph():
    in_child("_graph_check")


def _graph_check():
    import torch
    sc = base_scene()
    ctx = Context(device=0)
    try:
        ctx.upload_scene(sc)
        w, h, first = IMAGES[2]
        rgb, _ = replacement(2)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            static = torch.from_numpy(np.ascontiguousarray(sc.texture_texels[first:first + w * h].reshape(h, w, 3))).cuda()
            ctx.set_texture_texels(2, static, stream=side)            # warm-up outside the capture: the uploaded texels again
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                ctx.set_texture_texels(2, static, stream=torch.cuda.current_stream())
            static.copy_(torch.from_numpy(rgb))
            same_bytes(ctx.debug_materials()["texels"], sc.texture_texels, "a captured call stores nothing")
            g.replay()
            torch.cuda.synchronize()
        same_bytes(ctx.debug_materials()["texels"], with_texels(sc, 2, *replacement(2)).texture_texels, "replayed from a graph")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_refusals():
    lib = binding.load_library()
    sc = scenes.cornell_textured(1.0, 8, 4)
    image = base_scene()
    ctx = Context(device=0)

    def refuse(code, message, *args):
        rc = lib.slrhip_set_texture_texels(*args)
        text = lib.slrhip_last_error_string().decode()
        assert rc == code and "slrhip_set_texture_texels: " in text and message in text, (rc, text)
    try:
        with binding.DeviceBlocks() as dev:
            block = dev.alloc(16 * 12 * 12 + 16)
            refuse(NO_SCENE, "no scene uploaded", ctx.handle, 0, block, 0, None)
            ctx.upload_scene(sc)
            for t in range(len(sc.textures)):
                refuse(INVALID, "not an IMAGE_SPECTRUM texture", ctx.handle, t, block, 0, None)
            ctx.upload_scene(image)
            before = ctx.debug_materials()["texels"]
            refuse(INVALID, "null argument", ctx.handle, 0, None, 0, None)
            refuse(INVALID, "null argument", None, 0, block, 0, None)
            refuse(INVALID, "4-byte aligned", ctx.handle, 0, block + 2, 0, None)
            refuse(INVALID, "unknown flag bits", ctx.handle, 0, block, 2, None)
            refuse(INVALID, "unknown flag bits", ctx.handle, 0, block, 0x80000001, None)
            refuse(INVALID, "texture index out of range", ctx.handle, 3, block, 0, None)
            refuse(INVALID, "texture index out of range", ctx.handle, 0xFFFFFFFF, block, 0, None)
            same_bytes(ctx.debug_materials()["texels"], before, "after the refusals")
    finally:
        ctx.close()
