"""CPU: the C-ABI library loads without a GPU, exports every symbol include/slrhip.h declares, fails loudly
where a device is needed, and its host-only entry points (seeding contract, image export) match the reference."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from helpers import load_golden
from slr_amd import abi, binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return binding.load_library()


def declared_functions():
    names = set()
    for header in ("slrhip.h", "slrhip_debug.h"):          # the drop-in boundary and the diagnostic exports the parity tests use
        text = open(os.path.join(ROOT, "include", header)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names |= set(re.findall(r"\b(slrhip_[a-z_0-9]+)\s*\(", text))
    return sorted(names)


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert len(names) >= 16
    for n in names:
        assert hasattr(lib, n), "libslrhip.so does not export " + n
    assert sorted(binding.EXPORTS) == names


@pytest.mark.parametrize("num_pixels, num_slots, num_passes, run_length",
                         [(64 * 48, 64 * 48 * 8 // 256 * 256, 40, 8),      # the usual case: many runs per queue
                          (1000, 256, 12, 4),                              # few queues, a pixel count that is no multiple of anything
                          (37, 1024, 3, 1),                                # more slots than samples: most queues are empty
                          (640 * 360, 640 * 360 * 4, 64, 64),              # one run per pixel, four slots per pixel
                          (513, 64, 6, 2)])                                # a single queue
def test_work_queues_hand_out_every_sample_exactly_once(lib, num_pixels, num_slots, num_passes, run_length):
    """The sample scheduling of the render path (pt_kernels.h WorkItem), evaluated on the host by the function the kernels call:
    the (pixel, pass) samples of a window are dealt to per-wave queues in runs of `run_length` passes of one pixel.  Every sample
    must come up exactly once, the queues must be of equal length to within one run, and a queue walks over the image (its runs
    are not all the same pixel), which is what balances the work of the queues."""
    f = lib.slrhip_debug_work_distribution
    f.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p]
    counts = np.zeros(num_pixels * num_passes, np.uint32)
    lengths = np.zeros(num_slots // 64, np.uint32)
    assert f(num_pixels, num_slots, num_passes, run_length, counts.ctypes.data, lengths.ctypes.data) == 0
    assert (counts == 1).all()
    assert int(lengths.sum()) == num_pixels * num_passes
    assert int(lengths.max()) - int(lengths.min()) <= run_length
    assert f(num_pixels, num_slots, num_passes, num_passes + 1, counts.ctypes.data, lengths.ctypes.data) != 0      # the run length must divide the passes


GIB = 1 << 30
MIB = 1 << 20


def render_plan(lib, width, height, shard=(0, 1), stripes=0, mode=abi.MODE_RGB, passes=1, budget=16 * GIB, want_pixels=False):
    """slrhip_debug_render_plan: (numPixels, stripes, numSlots, window), [(passes, run length) per window], pixel list or None."""
    f = lib.slrhip_debug_render_plan
    f.argtypes = [C.c_int32, C.c_int32] + [C.c_uint32] * 3 + [C.c_int32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                                              C.c_void_p, C.c_void_p, C.c_uint32]
    plan = np.zeros(4, np.uint32)
    max_windows = max(passes, 1)
    windows = np.zeros(2 * max_windows, np.uint32)
    num_windows = C.c_uint32(0)
    pixels = np.full(width * height, 0xDEADBEEF, np.uint32) if want_pixels else None
    rc = f(width, height, shard[0], shard[1], stripes, mode, passes, budget, plan.ctypes.data, windows.ctypes.data, max_windows,
           C.byref(num_windows), pixels.ctypes.data if want_pixels else None, pixels.size if want_pixels else 0)
    if rc != 0:
        raise binding.SlrHipError("(%d): %s" % (rc, lib.slrhip_last_error_string().decode()))
    assert num_windows.value <= max_windows
    return tuple(int(v) for v in plan), [tuple(int(v) for v in w) for w in windows[:2 * num_windows.value].reshape(-1, 2)], \
        (pixels[:int(plan[0])] if want_pixels else None)


@pytest.mark.parametrize("width, height, shard, mode, stripes, slots",
                         [(1280, 720, (0, 1), abi.MODE_RGB, 32, 29491200),
                          (1280, 720, (0, 1), abi.MODE_SPECTRAL, 8, 7372800),
                          (1280, 720, (5, 8), abi.MODE_RGB, 64, 7372800),          # 115 200 pixels: capped at the 64 stripes of the pool's mask
                          (64, 64, (0, 1), abi.MODE_RGB, 64, 262144),
                          (64, 64, (0, 1), abi.MODE_SPECTRAL, 64, 262144)])
def test_render_plan_automatic_slot_count(lib, width, height, shard, mode, stripes, slots):
    """The automatic stripe count (slrhip_config::stripes = 0): the smallest power of two that reaches 22 118 400 slots in RGB mode,
    7 372 800 in spectral mode, at most 64; slots = pixels x stripes rounded up to 256.  Values derived by hand from that rule."""
    (num_pixels, got_stripes, got_slots, _), _, _ = render_plan(lib, width, height, shard, 0, mode)
    assert num_pixels == width * height // shard[1]
    assert (got_stripes, got_slots) == (stripes, slots)


@pytest.mark.parametrize("width, height, mode, passes, budget, window, windows",
                         [(1280, 720, abi.MODE_RGB, 1024, 16 * GIB, 1024, [(1024, 64)]),
                          (1280, 720, abi.MODE_SPECTRAL, 1024, 16 * GIB, 256, [(256, 64)] * 4),
                          (1280, 720, abi.MODE_RGB, 100, 16 * GIB, 64, [(64, 64), (36, 4)]),
                          (1280, 720, abi.MODE_RGB, 2048, 16 * GIB, 1152, [(1152, 64), (896, 64)]),
                          (64, 64, abi.MODE_RGB, 32, MIB, 16, [(16, 16)] * 2),          # the windows test_stripes_do_not_change_the_image forces
                          (64, 64, abi.MODE_SPECTRAL, 32, MIB, 4, [(4, 4)] * 8)])
def test_render_plan_result_windows(lib, width, height, mode, passes, budget, window, windows):
    """The split of a render call into result windows (16 B per pixel and pass, 64 B in spectral mode): as many passes as fit the
    budget, whole runs of 64 once there are 64, and per window the largest power-of-two fraction of 64 that divides it as its run
    length.  Values derived by hand from slrhip_render's arithmetic."""
    plan, got, _ = render_plan(lib, width, height, mode=mode, passes=passes, budget=budget)
    assert plan[0] == width * height and plan[3] == window
    assert got == windows


def _tile_major_pixels(width, height, index, count):
    """The shard's pixel list as slrhip.h states it: the 8x8 tiles t (row-major over the frame) with t % count == index, each tile
    row-major, cut at the frame's edge."""
    tiles_x, tiles_y = (width + 7) // 8, (height + 7) // 8
    out = []
    for t in range(index, tiles_x * tiles_y, count):
        tx, ty = t % tiles_x, t // tiles_x
        out += [(x, y) for y in range(8 * ty, min(8 * ty + 8, height)) for x in range(8 * tx, min(8 * tx + 8, width))]
    return out


@pytest.mark.parametrize("shard_count", [1, 3, 8])
@pytest.mark.parametrize("width, height", [(1, 1), (3, 5), (9, 8), (37, 21), (64, 64), (1280, 720)])
def test_render_plan_shards_partition_the_frame(lib, width, height, shard_count):
    """The pixel lists of the shards of a frame are disjoint and cover every pixel once, each is 8x8-tile-major, a shard without
    a tile has no pixel and no slot, and the arithmetic pixel count agrees with the list."""
    seen = np.zeros((height, width), np.uint32)
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    for index in range(shard_count):
        (num_pixels, stripes, slots, window), windows, pixels = render_plan(lib, width, height, (index, shard_count), passes=8, want_pixels=True)
        assert len(pixels) == num_pixels
        if index >= tiles:
            assert (num_pixels, slots, window, windows) == (0, 0, 0, [])
            continue
        x, y = pixels & 0xFFFF, pixels >> 16
        if width * height <= 64 * 64:
            assert list(zip(x.tolist(), y.tolist())) == _tile_major_pixels(width, height, index, shard_count)
        else:          # the same statement without the Python loop: the tile sequence is the shard's, and inside a tile y, x ascend
            tile = (y // 8) * ((width + 7) // 8) + x // 8
            order = tile.astype(np.int64) * 64 + (y % 8) * 8 + x % 8
            assert (np.diff(order) > 0).all() and (tile % shard_count == index).all()
        np.add.at(seen, (y, x), 1)
        assert slots % 256 == 0 and slots >= num_pixels * stripes > slots - 256
    assert (seen == 1).all()


@pytest.mark.parametrize("mode", [abi.MODE_RGB, abi.MODE_SPECTRAL])
@pytest.mark.parametrize("width, height, shard, passes, budget",
                         [(1, 1, (0, 1), 7, 16 * GIB), (3, 5, (0, 3), 1000, 4096), (9, 8, (0, 3), 130, MIB), (37, 21, (7, 8), 97, 64 * 1024),
                          (1280, 720, (0, 1), 5000, 16 * GIB), (1280, 720, (2, 8), 333, 100 * MIB), (1280, 720, (0, 1), 3, MIB)])
def test_render_plan_windows_cover_the_call(lib, mode, width, height, shard, passes, budget):
    """The windows of a call sum to its pass count, all but the last have the window length, each window's run length divides it
    and is a power of two <= 64, each window fits the budget unless that would mean less than one pass, and a fixed stripe count
    is honoured."""
    (num_pixels, stripes, slots, window), windows, _ = render_plan(lib, width, height, shard, 5, mode, passes, budget)
    assert stripes == 5 and slots == (num_pixels * 5 + 255) // 256 * 256
    entry = 64 if mode == abi.MODE_SPECTRAL else 16
    assert sum(n for n, _ in windows) == passes
    assert all(n == window for n, _ in windows[:-1]) and 0 < windows[-1][0] <= window
    for n, run in windows:
        assert n % run == 0 and run in (1, 2, 4, 8, 16, 32, 64)
        assert n * num_pixels * entry <= budget or n == 1
        assert n * num_pixels < 1 << 32
    assert window < 64 or window % 64 == 0


def test_render_plan_refuses_before_it_builds_anything(lib):
    """The refusals of slrhip_render_begin, with their texts; a 65535 x 65535 frame (4.29e9 pixels) is refused for its slot count
    without its pixel list being built: the plan counts the pixels row of tiles by row of tiles, so the call returns at once (the
    list alone would be 17 GB)."""
    import time
    for args, message in [((0, 5), "image size out of range"), ((65536, 8), "image size out of range"),
                          ((8, 8, (1, 1)), "bad shard"), ((8, 8, (0, 0)), "bad shard")]:
        with pytest.raises(binding.SlrHipError, match=r"^\(1\): slrhip_render_begin: %s$" % message):
            render_plan(lib, *args)
    t0 = time.monotonic()
    with pytest.raises(binding.SlrHipError, match=r"^\(1\): slrhip_render_begin: too many path slots$"):
        render_plan(lib, 65535, 65535)
    assert time.monotonic() - t0 < 1.0


def test_version(lib):
    text = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    assert lib.slrhip_version() == int(re.search(r"#define SLRHIP_VERSION (\d+)", text).group(1)) == 7


def test_create_fails_loudly_without_gpu(lib):
    # asked in a child process: torch ships its own copy of the HIP runtime, and once that copy has opened the device in this
    # process the runtime libslrhip.so uses finds none, which would fail every GPU test that runs after this one
    probe = subprocess.check_output([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], text=True, timeout=600)
    if probe.split()[-1] == "True":
        pytest.skip("a GPU is present")
    with pytest.raises(binding.SlrHipError) as e:
        binding.Context(device=0)
    assert "no HIP device" in str(e.value)


def test_invalid_arguments_are_rejected(lib):
    assert lib.slrhip_create(None, None) == 1
    assert lib.slrhip_upload_scene(None, None) == 1
    assert lib.slrhip_render(None, 0, 1, None) == 1
    assert b"null" in lib.slrhip_last_error_string()


def test_sample_seed_matches_python_restatement(lib):
    rng = np.random.default_rng(3)
    for _ in range(200):
        seed = int(rng.integers(-2**31, 2**31))
        x, y, s = int(rng.integers(0, 65536)), int(rng.integers(0, 65536)), int(rng.integers(0, 1 << 20))
        assert lib.slrhip_sample_seed(seed, x, y, s) == abi.sample_seed(seed, x, y, s)


@pytest.mark.parametrize("name", ["tonemap_bmp", "tonemap_bmp_spectral"])
def test_tonemap_and_bmp_match_reference_saveimage(lib, name):
    """slrhip_tonemap_bgr8 + slrhip_save_bmp == ImageSensor::saveImage + saveBMP, byte for byte
    (golden BMP written by the compiled reference — RGB build, and spectral build: 16 storage bins through
    DiscretizedSpectrum::getRGB; pad bytes excluded: the reference leaves them uninitialised)."""
    g = load_golden(name)
    fb = np.ascontiguousarray(g["framebuffer"])
    h, w, comps = fb.shape
    byte_width = 3 * w + w % 4
    out = np.zeros(byte_width * h, np.uint8)
    scale = float(g["scale"]) * float(g["sensitivity"])          # saveImage: scale *= sensitivity (ImageSensor.cpp:147)
    rc = lib.slrhip_tonemap_bgr8(fb.ctypes.data, w, h, comps, C.c_float(scale), out.ctypes.data, out.size)
    assert rc == 0
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "o.bmp")
        assert lib.slrhip_save_bmp(path.encode(), out.ctypes.data, w, h) == 0
        mine = np.frombuffer(open(path, "rb").read(), np.uint8)
    ref = g["bmp"]
    assert mine.size == ref.size
    assert (mine[:54] == ref[:54]).all()                          # headers
    a, b = mine[54:].reshape(h, byte_width)[:, :3 * w], ref[54:].reshape(h, byte_width)[:, :3 * w]
    assert (a == b).all(), "%d of %d pixel bytes differ" % ((a != b).sum(), a.size)


def test_cpp_spectrum_construction_matches_the_reference_and_the_python_host(lib):
    """slrhip_upsample / slrhip_resolve_upsampled (the C++ host's construction of spectral-mode spectra) against the compiled
    reference's UpsampledContinuousSpectrum constructor (tests/golden/upsample_kat.npz: (u, v, scale) for 768 inputs over both
    spectrum types and all four colour spaces, SpectrumTypes.h:180-237), and against slr_amd/spectra.py, whose payloads the
    GPU parity tests render with: every float bit-equal."""
    from helpers import assert_bit_equal
    from slr_amd import spectra
    g = load_golden("upsample_kat")["rows"]
    for row in g:
        out = np.zeros(3, np.float32)
        assert lib.slrhip_upsample(int(row[0]), int(row[1]), C.c_float(row[2]), C.c_float(row[3]), C.c_float(row[4]), out.ctypes.data) == 0
        assert_bit_equal(out, row[5:8], "slrhip_upsample %s" % row[:5])
        assert_bit_equal(np.array(spectra.upsample(int(row[0]), int(row[1]), row[2], row[3], row[4]), np.float32), row[5:8], "spectra.upsample")
    assert lib.slrhip_upsample(2, 0, C.c_float(0.5), C.c_float(0.5), C.c_float(0.5), np.zeros(3, np.float32).ctypes.data) == 1   # IOR from sRGB: the reference asserts
    # the (u, v)-only half of evaluate(): cell, data points, weights and the interleaved payload
    holder = type("T", (), {"_tables": None})()          # keeps the table arrays alive
    sc_tables = abi.Scene.upsampling_tables(holder)
    rng = np.random.default_rng(5)
    uvs = np.concatenate([g[:, 5:7], rng.uniform(-1, 15, (512, 2)).astype(np.float32)])
    kinds = set()
    for u, v in uvs:
        n = C.c_uint32(0)
        payload = np.full(4 + 4 * 95, -1.0, np.float32)
        assert lib.slrhip_resolve_upsampled(C.byref(sc_tables), C.c_float(u), C.c_float(v), C.byref(n), payload.ctypes.data) == 0
        pn, pw, pidx = spectra.resolve_upsampled(u, v)
        assert n.value == pn
        kinds.add(pn)
        assert_bit_equal(payload[:4], pw, "weights")
        spec = spectra.tables()["point_spectrum"]
        want = np.stack([spec[pidx[k]] if k < pn else np.zeros(95, np.float32) for k in range(4)], axis=1)
        assert_bit_equal(payload[4:].reshape(95, 4), want, "payload")
    assert kinds == {0, 3, 4}


def _numpy_spectrum_to_rgb(sp_type, values, lo=None, hi=None, lambdas=None, integral=None, to_rgb=None):
    """A second, independent restatement (numpy float32, one operation per line) of the RGB build's Spectrum::create for a sampled
    spectrum (libSLRSceneGraph/API.cpp:1149-1278): the walk over the union of the CMF's 1-nm grid and the spectrum's samples."""
    from slr_amd import spectra
    F = np.float32
    cmf = spectra.tables()["cmf"]
    values = np.asarray(values, F)
    n = len(values)
    low, ncmf = F(360.0), 471
    cmf_bin = F(F(830.0) - low) / F(ncmf - 1)
    bin_w = None if lambdas is not None else F(F(hi) - F(lo)) / F(n - 1)
    cur_cmf, base = 0, 0
    cur = low
    prev = [F(0), F(0), F(0)]
    prev_v, half = F(0), F(0)
    acc = [[F(0), F(0)] for _ in range(3)]          # Kahan pairs

    def kahan(p, v):
        c_in = F(v - p[1]); t = F(p[0] + c_in); p[1] = F(F(t - p[0]) - c_in); p[0] = t

    def sample_pos(i):
        return F(lambdas[i]) if lambdas is not None else F(F(lo) + F(F(i) * bin_w))
    while True:
        if cur == F(low + F(F(cur_cmf) * cmf_bin)):
            bar = [cmf[k][cur_cmf] for k in range(3)]
            cur_cmf += 1
        elif cur < low:
            bar = [F(0), F(0), F(0)]          # the reference's detour below 360 nm is undefined behaviour: see slrhip_spectrum_to_rgb
        else:
            idx = min(int(F(F(cur - low) / cmf_bin)), ncmf - 2)
            t = F(F(cur - F(low + F(F(idx) * cmf_bin))) / cmf_bin)
            bar = [F(F(F(F(1) - t) * cmf[k][idx]) + F(t * cmf[k][idx + 1])) for k in range(3)]
        first, last = (F(lambdas[0]), F(lambdas[n - 1])) if lambdas is not None else (F(lo), F(hi))
        if cur < first:
            v = values[0]
        elif cur > last:
            v = values[n - 1]
        elif base < n and cur == sample_pos(base):
            v = values[base]
            base += 1
        else:
            if lambdas is not None:
                lb = int(np.searchsorted(np.asarray(lambdas, F), cur, side="left"))
                idx = min(max(lb - 1, 0), n - 2)
                t = F(F(cur - F(lambdas[idx])) / F(F(lambdas[idx + 1]) - F(lambdas[idx])))
            else:
                idx = min(int(F(F(cur - F(lo)) / bin_w)), n - 2)
                t = F(F(cur - F(F(lo) + F(F(idx) * bin_w))) / bin_w)
            v = F(F(F(F(1) - t) * values[idx]) + F(t * values[idx + 1]))
        avg = F(F(prev_v + v) * F(0.5))
        for k in range(3):
            kahan(acc[k], F(F(avg * F(prev[k] + bar[k])) * half))
        prev, prev_v = bar, v
        nxt_sample = sample_pos(base) if base < n else F(np.inf)
        nxt = min(F(low + F(F(cur_cmf) * cmf_bin)), nxt_sample)
        half = F(F(nxt - cur) * F(0.5))
        cur = nxt
        if cur_cmf == ncmf:
            break
    xyz = np.array([F(acc[k][0] / integral) for k in range(3)], F)
    return to_rgb(sp_type, xyz)


def test_rgb_build_values_of_named_spectra(lib):
    """SURVEY row a27, RGB half: slrhip_spectrum_to_rgb (the C++ host's Spectrum::create for sampled spectra in the RGB build).
    Pinned pieces (tests/golden/rgb_conversion_kat.npz, from the compiled libSLR): the global integralCMF and the XYZ -> sRGB /
    sRGB_E matrices with the clamp.  The integration loop itself lives in libSLRSceneGraph/API.cpp:1149-1278, which does not
    build here (assimp, OpenEXR): it has NO reference-held check — "parity unpinned" for that one step — so it is checked
    against an independent numpy restatement instead, bit for bit, on D65, four refractive-index tables and random spectra."""
    from helpers import assert_bit_equal
    from slr_amd import spectra
    g = load_golden("rgb_conversion_kat")
    F = np.float32
    integral = F(g["integral_cmf"][0])
    # integralCMF: Kahan sum of (ybar[i-1] + ybar[i]) * 1 * 0.5 with double literals (Spectrum.cpp:222-229)
    ybar = spectra.tables()["cmf"][1]
    s, c = F(0), F(0)
    for i in range(1, 471):
        v = F((np.float64(F(ybar[i - 1] + ybar[i])) * 1) * 0.5)
        c_in = F(v - c); t = F(s + c_in); c = F(F(t - s) - c_in); s = t
    assert s == integral

    m_srgb = [(3.2404542, -1.5371385, -0.4985314), (-0.9692660, 1.8760108, 0.0415560), (0.0556434, -0.2040259, 1.0572252)]
    m_e = [(2.6897, -1.2759, -0.4138), (-1.0221, 1.9783, 0.0438), (0.0612, -0.2245, 1.1633)]

    def to_rgb(sp_type, xyz, clamp=True):
        m = m_srgb if sp_type == spectra.ILLUMINANT else m_e
        rgb = np.array([F(r[0] * float(xyz[0]) + r[1] * float(xyz[1]) + r[2] * float(xyz[2])) for r in m], F)
        return np.maximum(rgb, F(0)) if clamp else rgb
    for tag, tp in (("illuminant", spectra.ILLUMINANT), ("reflectance", spectra.REFLECTANCE)):
        mine = np.stack([to_rgb(tp, x, clamp=False) for x in g["xyz"]])
        assert_bit_equal(mine, g["rgb_" + tag], "XYZ -> RGB " + tag)

    t = spectra.tables()
    rng = np.random.default_rng(8)
    cases = [("D65", spectra.ILLUMINANT, t["d65"], 300.0, 830.0, None)]
    for name in ("Aluminium", "Glass_BK7", "Air", "Titanium"):
        lo, hi, regular, _ = t["ior_%s_meta" % name]
        cases.append((name, spectra.IOR, t["ior_%s_etas" % name], float(lo), float(hi), None if regular else t["ior_%s_lambdas" % name]))
    cases.append(("random regular, narrower than the CMFs", spectra.REFLECTANCE, rng.random(37).astype(F), 400.0, 700.0, None))
    cases.append(("random regular, wider", spectra.REFLECTANCE, rng.random(64).astype(F), 300.0, 900.0, None))
    lam = np.sort(rng.uniform(350.0, 850.0, 23)).astype(F)
    cases.append(("random irregular", spectra.IOR, rng.random(23).astype(F) + F(1), 0.0, 0.0, lam))
    for name, tp, vals, lo, hi, lambdas in cases:
        got = np.array(spectra.spectrum_to_rgb(tp, vals, lo, hi, lambdas), F)
        want = _numpy_spectrum_to_rgb(tp, vals, lo, hi, lambdas, integral, to_rgb)
        assert_bit_equal(got, want, name)
        assert np.isfinite(got).all()
    d65 = np.array(spectra.named_rgb("D65"), F)
    assert np.allclose(d65, 98.89, atol=0.02)             # D65 is the white of sRGB: equal components, Y ~ 98.9 on this normalisation
