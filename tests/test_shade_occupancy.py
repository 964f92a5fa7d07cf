"""k_shade with the fused start at four waves per SIMD: the four instantiations with PRIMARY and without the glossy
lobes hold nothing of one trip in vector registers through the other, and fit 128 of them without scratch.

On the host: the compiler's resource remarks of the two translation units, built with the Makefile's flags — at most 128 VGPRs, no
scratch, 4 waves per SIMD for the kernels named below, by their mangled names.

On the GPU: nothing of the arithmetic changed, so every comparison is bit for bit against the same library with
SLRHIP_FLAG_NO_PRIMARY_PASS (test_shade_chain.compare: frames, samples, extension rays, shadow rays, samples started from the pass).
The shapes are chosen for what the change can break, a value that crosses a trip or a barrier on the wrong lane: launches in which
every lane of a workgroup starts a sample, workgroups that start none, counts that straddle a wave, paths that end in either trip,
slots that go idle in the launch in which their path ends, the twin without LDS tables and the twin that seeds its own stream."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import binding as ob
from slr_amd import abi, scenes
from test_primary_direct import begun, check_launch
from test_shade_chain import compare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slr_amd", "csrc")
KERNEL = "_ZN6slrhip7k_shadeINS_3RGBELb%dELb0ELb0ELb0ELb1ELb%dEEEvNS_8DevSceneENS_11PathBuffersENS_12RenderParamsEj"      # LDS_TABLES, RESUME
HIPCC = shutil.which(os.environ.get("HIPCC", "hipcc"))


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS = (.*)$", text, re.M).group(1).split()
    arch = re.search(r"^ARCH \?= (\S+)$", text, re.M).group(1)
    return ["--offload-arch=" + arch] + [f for f in flags if f not in ("-MMD", "-MP")]


def resource_remarks(source, tmp_path):
    """{mangled name: {remark: value}} of the kernels of one translation unit."""
    cmd = [HIPCC] + makefile_flags() + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, source),
                                        "-o", str(tmp_path / "unit.o")]
    done = subprocess.run(cmd, capture_output=True, text=True, cwd=CSRC)
    assert done.returncode == 0, done.stderr[-2000:]
    kernels, cur = {}, None
    for line in done.stderr.splitlines():
        m = re.search(r"remark: \s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif cur is not None and m.group(2).isdigit():
            cur[m.group(1)] = int(m.group(2))
    return kernels


@pytest.mark.skipif(HIPCC is None, reason="needs hipcc")
@pytest.mark.parametrize("source, resume", [("pt_shade_rgb_primary.hip", 1), ("pt_shade_rgb_primary_seeded.hip", 0)], ids=["resume", "seeded"])
def test_four_waves_without_scratch(source, resume, tmp_path):
    kernels = resource_remarks(source, tmp_path)
    assert len(kernels) == 4, sorted(kernels)
    for lds in (1, 0):
        r = kernels[KERNEL % (lds, resume)]
        print(source, "LDS_TABLES", lds, r)
        assert r["VGPRs"] <= 128 and r["AGPRs"] == 0, r
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, r
        assert r["Occupancy"] == 4, r


# ---- frames ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spheres():
    return scenes.cornell_box_spheres(1.0, 8, 4, "glass")


def patchwork(num_materials=45, num_lights=20):
    """Cornell walls and a floor patchwork, a matte material per patch, some patches emit: more materials (> 32) and lights (> 16) than
    k_shade stages in LDS, no glossy lobe — the instantiations with LDS_TABLES = false."""
    b = scenes.SceneBuilder()
    scenes.cornell_walls(b)
    rng = np.random.default_rng(3)
    side = int(np.ceil(np.sqrt(num_materials)))
    for i in range(num_materials):
        r, g, bl = rng.uniform(0.1, 0.9, 3)
        emit = b.spectrum_d65(0.5 + 0.1 * i, scenes.D65_RGB) if i < num_lights else -1
        m = b.matte(b.spectrum_srgb_nonlinear(float(r), float(g), float(bl)), emittance=emit)
        x, z = -1.2 + 2.4 * (i % side) / side, -1.8 + 3.0 * (i // side) / side
        w, y = 2.2 / side, 0.02 + 0.3 * (i % 3)
        b.add_quad([(x, y, z + w), (x + w, y, z + w), (x + w, y, z), (x, y, z)], (0, 1, 0), (1, 0, 0), m)
    return b.build(scenes.cornell_camera(1.0), name="patchwork")


@pytest.mark.gpu
def test_every_lane_of_a_workgroup_starts(spheres):
    """48 x 36, one pass, a slot per pixel: in the first launch every slot wants a sample, so every full workgroup starts 256 (trip 1 on
    every lane) and the last, of 1 728 - 6 x 256 = 192 slots' worth, fewer; the pass after the last is the queue's end on every lane."""
    for stripes in (1, 64, 0):
        compare(spheres, ob.settings(48, 36, seed=41), ((0, 1),), "48x36, 1 pass, stripes %d" % stripes, 48 * 36, stripes=stripes)


@pytest.mark.gpu
def test_workgroups_that_start_nothing(spheres):
    """36 x 20, 3 passes, 64 stripes: 46 080 slots for 2 160 samples — after the first launches most workgroups start nothing (n = 0, the
    uniform exit before trip 1) while their paths run on, and a slot whose path ends finds its queue empty and goes idle in that launch."""
    compare(spheres, ob.settings(36, 20, seed=42), ((0, 3),), "36x20, 3 passes, stripes 64", 36 * 20, stripes=64)


@pytest.mark.gpu
@pytest.mark.parametrize("passes", (63, 64, 65))
def test_counts_that_straddle_a_wave(spheres, passes):
    """A wave's queue holds runs of one pixel's passes: 63, 64 and 65 put the end of a run, and with it the number of starts of a wave
    and the compaction's wave bases, one short of, on and one past a wave of lanes.  65 = a window of 64 and a window of one pass: the
    last pass of a window ends paths in trip 0 whose slots go idle in the same launch."""
    for stripes in (1, 0):
        compare(spheres, ob.settings(36, 20, seed=43), ((0, passes),), "36x20, %d passes, stripes %d" % (passes, stripes), 36 * 20, stripes=stripes)


@pytest.mark.gpu
def test_paths_that_end_in_trip_1():
    """The terrain under an open sky, no environment light: camera rays that miss end their path in the visit of the fused start."""
    sc = scenes.lattice_terrain(8)
    st = ob.settings(37, 19, seed=3)
    ctx = begun(sc, st)
    rec, miss = check_launch(ctx, 37 * 19, 0, 5, 5, True, "open terrain")
    ctx.close()
    assert miss.any() and (~miss).any(), (int(miss.sum()), len(miss))
    for stripes, passes in ((1, 5), (64, 3), (0, 65)):
        compare(sc, st, ((0, passes),), "open terrain, %d passes, stripes %d" % (passes, stripes), 37 * 19, stripes=stripes)


@pytest.mark.gpu
def test_twin_without_lds_tables():
    sc = patchwork()
    assert len(sc.materials) > 32 and (sc.materials["emittance"] >= 0).sum() > 16
    for stripes, passes in ((1, 6), (64, 3), (0, 65)):
        compare(sc, ob.settings(48, 36, seed=44), ((0, passes),), "patchwork, %d passes, stripes %d" % (passes, stripes), 48 * 36, stripes=stripes)


@pytest.mark.gpu
def test_seeded_twin():
    """An instanced scene runs the pass without the stream plane (the fused start seeds its own stream); compare() checks that no plane
    was bound and that every sample started from the pass."""
    sc = scenes.cornell_instanced(1.0, 10, 5)
    assert len(sc.instances) > 0
    for stripes, passes in ((1, 6), (64, 3), (0, 65)):
        compare(sc, ob.settings(48, 36, seed=45), ((0, passes),), "instanced, %d passes, stripes %d" % (passes, stripes), 48 * 36, stripes=stripes)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [abi.FLAG_TIME_KERNELS, 0], ids=["event-timed", "hipGraph"])
def test_launch_loops(flags):
    """640 x 480: 614 400 slots at two stripes — the event-timed loop, and the loop that captures blocks of iterations into a hipGraph."""
    sc = scenes.cornell_box_spheres(4.0 / 3.0, 16, 8, "matte")
    compare(sc, ob.settings(640, 480, seed=78), ((0, 8),), "640x480, flags %d" % flags, 640 * 480, stripes=2, flags=flags)
