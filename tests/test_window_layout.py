"""The result window is results[pixel][pass of the window]: the entry of a sample is pixel x P + pass, with P the
pass count of the window being rendered.  The layout changes no arithmetic — the sensor still adds a pixel's samples in pass
order — so every comparison here is bit for bit (helpers.assert_bit_equal).  The shapes are the smallest at which an index or a
remainder can go wrong:

  36 x 20 pixels   partial 8 x 8 tiles, and 720 pixels are not a multiple of a 256-thread block
  passes           1, 3, 8, 13, 65, 100: the fold's remainders (P % 8 in RGB, P % 4 in spectral), the default run length of 64,
                   and a call that the plan cuts into windows of 64 + 1 and 64 + 36 passes (two different P in one call)
  160 x 120        with SLRHIP_RESULT_WINDOW_MB=1 (read once per process: a fresh child): many windows, the last one shorter
  instances        the instance plane of the primary pass takes the same index
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import assert_bit_equal
from oracle import binding as ob
from slr_amd import Context, abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = 36, 20
RGB_PASSES = (1, 3, 8, 13, 65, 100)
SPECTRAL_PASSES = (1, 5, 68)
MODES = {"rgb": abi.MODE_RGB, "spectral": abi.MODE_SPECTRAL}


@pytest.fixture(scope="module")
def spheres():
    return scenes.cornell_box_spheres(W / H, 8, 4, "matte")          # Lambert + mirror: no float libm on a path


@pytest.fixture(scope="module")
def oracle_frames(spheres, oracle_rgb, oracle_spectral):
    """The oracle's frame of every (mode, pass count) of this file, rendered once."""
    st = ob.settings(W, H, seed=18)
    out = {}
    for mode, lib, passes in (("rgb", oracle_rgb, RGB_PASSES), ("spectral", oracle_spectral, SPECTRAL_PASSES)):
        sc = lib.scene(spheres)
        for n in passes:
            out[mode, n] = sc.render(st, n)[0]
    return out


@pytest.fixture(scope="module")
def contexts(spheres):
    """One context per (mode, stripes), with the scene uploaded."""
    out = {}
    for mode in MODES:
        for stripes in (1, 0):
            out[mode, stripes] = Context(mode=MODES[mode], stripes=stripes)
            out[mode, stripes].upload_scene(spheres)
    yield out
    for c in out.values():
        c.close()


def render(ctx, st, passes, shard=(0, 1)):
    ctx.render_begin(st, shard)
    ctx.render(0, passes)
    return ctx.read_framebuffer()


@pytest.mark.gpu
@pytest.mark.parametrize("stripes", [1, 0], ids=["stripes1", "auto"])
@pytest.mark.parametrize("passes", RGB_PASSES)
def test_ragged_frame_rgb_equals_the_oracle(contexts, oracle_frames, passes, stripes):
    ctx = contexts["rgb", stripes]
    st = ob.settings(W, H, seed=18)
    fb = render(ctx, st, passes)
    assert int(ctx.counters().samples) == W * H * passes
    assert ctx.primary_samples() == W * H * passes          # every sample started from its record in the window
    assert_bit_equal(fb, oracle_frames["rgb", passes], "RGB, %d passes, stripes %d vs oracle" % (passes, stripes))
    assert fb.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("stripes", [1, 0], ids=["stripes1", "auto"])
@pytest.mark.parametrize("passes", SPECTRAL_PASSES)
def test_ragged_frame_spectral_equals_the_oracle(contexts, oracle_frames, passes, stripes):
    """64-byte entries, and the fold's quads (four lanes per pixel)."""
    ctx = contexts["spectral", stripes]
    st = ob.settings(W, H, seed=18)
    fb = render(ctx, st, passes)
    assert int(ctx.counters().samples) == W * H * passes
    assert_bit_equal(fb, oracle_frames["spectral", passes], "spectral, %d passes, stripes %d vs oracle" % (passes, stripes))
    assert fb.sum() > 0


WINDOWS = dict(width=160, height=120, passes=20, seed=7)
CHILD = """
import sys
import numpy as np
sys.path[:0] = [%(root)r, %(tests)r]
import test_window_layout as t
np.save(sys.argv[2], t.windows_frame(sys.argv[1]))
"""


def windows_frame(mode):
    cfg = WINDOWS
    ctx = Context(mode=MODES[mode], stripes=1)
    fb = ctx.render_image(scenes.cornell_box_spheres(cfg["width"] / cfg["height"], 8, 4, "matte"), ob.settings(cfg["width"], cfg["height"], seed=cfg["seed"]),
                          cfg["passes"])
    assert int(ctx.counters().samples) == cfg["width"] * cfg["height"] * cfg["passes"]
    ctx.close()
    return fb


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_unequal_windows_give_the_single_window_frame(tmp_path, mode):
    """160 x 120 pixels, 20 passes: a pass is 300 KiB of RGB results, so a budget of 1 MiB renders windows of 3 passes and a last one
    of 2 (spectral: 1.2 MB per pass, windows of one pass each).  The child's frame equals this process's single-window frame."""
    cfg = WINDOWS
    pixels = cfg["width"] * cfg["height"]
    assert pixels * 16 * 4 > (1 << 20) > pixels * 16 * 3 and cfg["passes"] % 3 == 2
    env = dict(os.environ, SLRHIP_RESULT_WINDOW_MB="1")
    out = str(tmp_path / "child.npy")
    child = subprocess.Popen([sys.executable, "-c", CHILD % dict(root=ROOT, tests=os.path.join(ROOT, "tests")), mode, out], env=env)
    try:
        whole = windows_frame(mode)
    finally:
        assert child.wait(timeout=120) == 0
    assert_bit_equal(np.load(out), whole, "%s: result windows of 1 MiB (child process) vs one window" % mode)
    assert whole.sum() > 0


@pytest.mark.gpu
def test_instanced_scene_equals_the_oracle(oracle_rgb):
    """The instance plane of the primary pass (PathBuffers::primaryInstance) is indexed like the window."""
    sc = scenes.instanced_grid(tiles_x=2, tiles_z=2, cells=2, aspect=48.0 / 36.0)
    assert len(sc.instances) == 4
    st = ob.settings(48, 36, seed=33)
    want, ctr = oracle_rgb.scene(sc).render(st, 6)
    ctx = Context(mode=abi.MODE_RGB, stripes=1)
    try:
        fb = ctx.render_image(sc, st, 6)
        assert int(ctx.counters().samples) == int(ctr.samples) == 48 * 36 * 6
        assert ctx.primary_samples() == 48 * 36 * 6
    finally:
        ctx.close()
    assert_bit_equal(fb, want, "instanced grid vs oracle")
    assert fb.sum() > 0


@pytest.mark.gpu
def test_two_rank_shard_split_sums_to_the_unsharded_frame(contexts):
    ctx = contexts["rgb", 1]
    st = ob.settings(W, H, seed=18)
    whole = render(ctx, st, 13)
    parts = [render(ctx, st, 13, shard=(rank, 2)) for rank in range(2)]
    assert ((parts[0] != 0) & (parts[1] != 0)).sum() == 0          # disjoint supports: the sum is a gather
    assert parts[0].sum() > 0 and parts[1].sum() > 0
    assert_bit_equal(parts[0] + parts[1], whole, "two shards vs the unsharded frame")


def kahan(frames):
    """The sensor after the per-pass frames, added in pass order: BasicTypes/CompensatedSum.h per component, float32."""
    s, c = np.zeros_like(frames[0]), np.zeros_like(frames[0])
    for v in frames:
        c_input = v - c
        sum_temp = s + c_input
        c = (sum_temp - s) - c_input
        s = sum_temp
        assert s.dtype == F and c.dtype == F
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rgb", "spectral"])
def test_debug_fold_adds_host_samples_in_pass_order(contexts, mode):
    """5 passes of known samples spread over nine orders of magnitude, so that the order of the additions shows in the low bits."""
    ctx = contexts[mode, 1]
    rng = np.random.default_rng(5 + ctx.components)
    samples = (rng.random((5, H, W, ctx.components)) * np.exp(rng.normal(0.0, 5.0, (5, H, W, 1)))).astype(F)
    want = kahan(list(samples))
    assert not np.array_equal(want, kahan(list(samples[::-1]))), "the samples do not tell the order of the passes"
    ctx.render_begin(ob.settings(W, H, seed=1))
    ctx.debug_fold(samples)
    assert_bit_equal(ctx.read_framebuffer(), want, "%s: slrhip_debug_fold vs a Kahan sum in pass order" % mode)
