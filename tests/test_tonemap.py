"""The image export on the device (slrhip_tonemap / Context.tonemap / Context.frame_image / `python -m slr_amd.host --device-tonemap`):
the per-pixel pipeline of include/slrhip.h, compared EXACTLY with the host function slrhip_tonemap_bgr8.

exp and pow are the only places where the device may differ from the host in a last bit, so exact equality is required on inputs
where no such difference can move a byte.  A numpy restatement of the definition (float32 where the definition is float32, float64
where it is double, exp and pow from numpy) gives every byte's un-truncated value t = 256 * fminf(gamma, 0.999f).  A last-bit
difference in exp or pow moves t by about 256 * 2^-24 times a small factor (at the darkest luminance used, 2^-10, the cancellation in
1 - exp(-Y) amplifies it to a relative 2^-14 of a t of about 3: 2e-4), far below 2^-8.  The safe set: an ordinary pixel is kept only
if every channel's t is farther than 2^-8 from every integer it could cross (t >= 0 always, so 0 cannot be crossed); a pixel that fails
is replaced by a copy of the nearest kept one.

Inputs (np.random.default_rng, no render): log-uniform pixel values such that the scaled luminance spans 2^-10 .. 2^6, three
components drawn around it (a twelfth of the RGB pixels get one negative channel); for 16 components smooth random spectra times the
same range, a tenth of the pixels with a negative bin.  Mixed in after the filter, where the image has room: pixels whose bytes the
definition fixes: exactly zero and all-negative (0 0 0), +inf everywhere and a NaN in one component (255 255 255).

Input condition, asserted on the CPU before any GPU result is looked at (test_input_condition, and again by every GPU case): at most
5 % of the ordinary pixels are replaced (expected: 3 channels x 2 x 2^-8 = 2.3 % of those not saturated), dark channels lie on both
sides of the 0.0031308 gamma knee, and slrhip_tonemap_bgr8 equals the restatement in every byte.  Shares replaced, measured on the CPU
(256 candidates at least per case): between 0.4 % and 4.3 % over the six shapes x two component counts x two scales."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from slr_amd import Context, abi, binding, host, spectra

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 2.0 ** -8
KNEE = 0.0031308
SHAPES = [(1, 1), (36, 5), (37, 21), (38, 5), (39, 5), (130, 3)]
SCALES = [1.0, 0.37]
INVALID = 1                                                         # SLRHIP_ERR_INVALID_ARGUMENT


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def cmf16():
    t = np.asarray(spectra.tables()["cmf16"], F)
    return t[0:16].copy(), t[16:32].copy(), t[32:48].copy(), F(t[48])


def restate(pixels, scale):
    """t [N, 3] (R, G, B; float32) of pixels [N, C] float32: the un-truncated byte values of include/slrhip.h's definition."""
    pixels = np.asarray(pixels)
    assert pixels.dtype == F and pixels.ndim == 2
    s = F(scale)
    with np.errstate(all="ignore"):
        if pixels.shape[1] == 3:
            rgb = pixels * s
        else:
            xbar, ybar, zbar, integral = cmf16()
            X = Y = Z = np.zeros(len(pixels), F)
            for b in range(16):
                v = pixels[:, b] * s
                X, Y, Z = X + xbar[b] * v, Y + ybar[b] * v, Z + zbar[b] * v
            X, Y, Z = X / integral, Y / integral, Z / integral
            assert X.dtype == Y.dtype == Z.dtype == F
            X, Y, Z = X.astype(np.float64), Y.astype(np.float64), Z.astype(np.float64)
            rgb = np.stack([3.2404542 * X - 1.5371385 * Y - 0.4985314 * Z, -0.9692660 * X + 1.8760108 * Y + 0.0415560 * Z,
                            0.0556434 * X - 0.2040259 * Y + 1.0572252 * Z], axis=1).astype(F)
        assert rgb.dtype == F
        rgb = np.where(rgb < 0, F(0), rgb)
        d = rgb.astype(np.float64)
        lum = (0.222485 * d[:, 0] + 0.716905 * d[:, 1] + 0.060610 * d[:, 2]).astype(F)
        e = np.exp(-lum.astype(np.float64)).astype(F)
        scale_y = np.where(lum != 0, (F(1) - e) / lum, F(0))
        v = np.fmin(scale_y[:, None] * rgb, F(1))
        assert scale_y.dtype == F and v.dtype == F
        vd = v.astype(np.float64)
        gamma = np.where(vd <= KNEE, 12.92 * vd, 1.055 * np.power(vd, 1.0 / 2.4) - 0.055).astype(F)
        t = F(256) * np.fmin(gamma, F(0.999))
    assert t.dtype == F and not np.isnan(t).any()
    return t, v


def safe(t):
    """Per pixel: every channel's t is farther than MARGIN from every integer it could cross (1 .. 255; t >= 0)."""
    t = t.astype(np.float64)
    return (np.abs(t - np.maximum(np.rint(t), 1.0)) > MARGIN).all(axis=1)


def bmp_bytes(t, width, height):
    """The BGR8_BMP image of the restated t [H * W, 3]."""
    rows = np.zeros((height, 3 * width + width % 4), np.uint8)
    rows[:, :3 * width] = t.astype(np.uint8).reshape(height, width, 3)[::-1, :, ::-1].reshape(height, 3 * width)
    return rows.reshape(-1)


def rgba_of_bmp(bmp, width, height):
    rows = bmp.reshape(height, 3 * width + width % 4)[::-1, :3 * width].reshape(height, width, 3)
    return np.concatenate([rows[:, :, ::-1], np.full((height, width, 1), 255, np.uint8)], axis=2)


def host_bmp(pixels, width, height, scale):
    lib = binding.load_library()
    fb = np.ascontiguousarray(pixels, F)
    out = np.full((3 * width + width % 4) * height, 0x55, np.uint8)
    assert lib.slrhip_tonemap_bgr8(fb.ctypes.data, width, height, fb.size // (width * height), C.c_float(scale), out.ctypes.data, out.size) == 0
    return out


# ---- synthetic inputs -----------------------------------------------------------------------------------------------------------
def candidates(n, comps, scale, rng):
    lum = np.exp2(rng.uniform(-10.0, 6.0, n))                       # the scaled luminance, about
    if comps == 3:
        p = lum[:, None] * np.exp2(rng.uniform(-1.5, 1.5, (n, 3)))
        neg = rng.random(n) < 1.0 / 12.0
        p[neg, rng.integers(0, 3, int(neg.sum()))] *= -1.0          # negative in one channel
    else:
        x = np.linspace(0.0, 1.0, 16)
        a, f, ph = rng.uniform(0.1, 0.9, (n, 1)), rng.uniform(0.5, 2.5, (n, 1)), rng.uniform(0, 2 * np.pi, (n, 1))
        shape = 1.0 + a * np.sin(2 * np.pi * f * x[None, :] + ph)   # smooth and positive
        neg = rng.random(n) < 0.1
        shape[neg, rng.integers(0, 16, int(neg.sum()))] *= -3.0     # a negative bin: exercises the clamp after XYZ -> sRGB
        p = lum[:, None] * shape
    return (p / scale).astype(F)


_cases = {}


def case(width, height, comps, scale):
    """The input [H, W, C] and the restated BGR8_BMP bytes of one case, computed once and shared (never modified)."""
    key = (width, height, comps, scale)
    if key in _cases:
        return _cases[key]
    n = width * height
    rng = np.random.default_rng(1000 * width + 10 * height + comps + int(100 * scale))
    cand = candidates(max(n, 256), comps, scale, rng)
    t, v = restate(cand, scale)
    keep = safe(t)
    kept = np.flatnonzero(keep)
    assert len(kept) > 0
    idx = np.arange(len(cand))
    pos = np.searchsorted(kept, idx)                                # the first kept candidate at or behind idx
    lo, hi = kept[np.clip(pos - 1, 0, len(kept) - 1)], kept[np.clip(pos, 0, len(kept) - 1)]
    nearest = np.where(np.abs(idx - lo) < np.abs(hi - idx), lo, hi)
    pixels = cand[nearest][:n].copy()
    ordinary = np.ones(n, bool)
    specials = {}
    if n >= 100:                                                    # pixels whose bytes the definition fixes, two of each kind
        where = rng.choice(n, 10, replace=False)
        nan_pixel = pixels[where[8:10]].copy()
        nan_pixel[:, comps // 2] = np.nan
        kinds = [("zero", F(0), 0), ("negative", -np.abs(pixels[where[2:4]]) if comps == 3 else -np.abs(pixels[where[2:4], :1]), 0),
                 ("negative tiny", F(-1e-30), 0), ("inf", F(np.inf), 255), ("nan", nan_pixel, 255)]
        for k, (name, value, byte) in enumerate(kinds):
            pixels[where[2 * k:2 * k + 2]] = value
            specials[name] = (where[2 * k:2 * k + 2], byte)
        ordinary[where] = False
    t_final, v_final = restate(pixels, scale)
    k = dict(pixels=pixels.reshape(height, width, comps), want=bmp_bytes(t_final, width, height), replaced=float(1.0 - keep.mean()),
             safe_final=safe(t_final), ordinary=ordinary, specials=specials, t=t_final, v=v_final)
    for a in (k["pixels"], k["want"], k["t"], k["v"]):
        a.setflags(write=False)
    _cases[key] = k
    return k


def assert_input_condition(width, height, comps, scale):
    k = case(width, height, comps, scale)
    print("%d x %d x %d, scale %g: %.2f %% of the candidates replaced" % (width, height, comps, scale, 100 * k["replaced"]))
    assert k["replaced"] <= 0.05, k["replaced"]
    assert k["safe_final"][k["ordinary"]].all()
    t = k["t"].reshape(height * width, 3)
    for name, (where, byte) in k["specials"].items():
        assert (t[where].astype(np.uint8) == byte).all(), name
        assert k["safe_final"][where].all(), name
    got = host_bmp(k["pixels"], width, height, scale)
    assert np.array_equal(got, k["want"]), "%d bytes of slrhip_tonemap_bgr8 differ from the restatement" % (got != k["want"]).sum()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_tonemap_bytes():
    """(Fails on the parent commit: the symbol does not exist there.)"""
    lib = binding.load_library()
    size = lib.slrhip_tonemap_bytes
    assert "slrhip_tonemap" in binding.EXPORTS and "slrhip_tonemap_bytes" in binding.EXPORTS
    assert size(37, 21, abi.IMAGE_BGR8_BMP) == 21 * (3 * 37 + 1)
    for w, row in ((36, 108), (37, 112), (38, 116), (39, 120)):
        assert size(w, 1, abi.IMAGE_BGR8_BMP) == row and size(w, 7, abi.IMAGE_BGR8_BMP) == 7 * row
    for w, h in ((1, 1), (37, 21), (1280, 720), (65535, 32768), (1, (1 << 31) - 1), ((1 << 31) - 1, 1)):
        assert size(w, h, abi.IMAGE_RGBA8) == 4 * w * h
        assert size(w, h, abi.IMAGE_BGR8_BMP) == (3 * w + w % 4) * h
    for w, h, f in ((0, 4, 0), (4, 0, 0), (0, 0, 1), (4, 4, 2), (4, 4, 0xFFFFFFFF), (65536, 32768, 0), (65536, 32768, 1), (1 << 31, 1, 1),
                    (0xFFFFFFFF, 0xFFFFFFFF, 0)):
        assert size(w, h, f) == 0, (w, h, f)


def test_refusals_that_need_no_device():
    lib = binding.load_library()
    d = abi.TonemapDesc(4, 4, 3, abi.IMAGE_RGBA8, 16, 4096, 64, 1.0, 0)
    assert lib.slrhip_tonemap(None, C.byref(d), None) == INVALID and lib.slrhip_tonemap(None, None, None) == INVALID
    assert b"slrhip_tonemap" in lib.slrhip_last_error_string()


def test_struct_layout():
    """slrhip_tonemap_desc under LP64: four uint32, two pointers, a size_t, a float and a uint32: 48 bytes."""
    offsets = {n: getattr(abi.TonemapDesc, n).offset for n, _ in abi.TonemapDesc._fields_}
    assert offsets == dict(width=0, height=4, components=8, format=12, color=16, output=24, output_bytes=32, scale=40, reserved=44)
    assert C.sizeof(abi.TonemapDesc) == 48
    text = open(os.path.join(ROOT, "include", "slrhip.h")).read()
    body = text[text.index("typedef struct slrhip_tonemap_desc {"):text.index("} slrhip_tonemap_desc;")]
    order = [body.index(" " + n) for n in ("width", "height", "components;", "format;", "color;", "output;", "output_bytes;", "scale;", "reserved;")]
    assert order == sorted(order)
    assert (abi.IMAGE_BGR8_BMP, abi.IMAGE_RGBA8) == (0, 1) and "#define SLRHIP_IMAGE_BGR8_BMP 0u" in text and "#define SLRHIP_IMAGE_RGBA8    1u" in text


def test_host_program_parses_the_flag():
    ap = host.build_parser()
    assert ap.parse_args(["scene.txt"]).device_tonemap is False
    a = ap.parse_args(["--device-tonemap", "scene.txt", "--denoise", "2"])
    assert (a.device_tonemap, a.denoise, a.scene) == (True, 2, "scene.txt")


@pytest.mark.parametrize("comps", [3, 16])
def test_input_condition(comps):
    for width, height in SHAPES:
        for scale in SCALES:
            assert_input_condition(width, height, comps, scale)
    # the dark end lies on both sides of the gamma knee, in kept ordinary pixels
    k = case(37, 21, comps, 1.0)
    v = k["v"][k["ordinary"]]
    below, above = int(((v > 0) & (v <= KNEE)).sum()), int(((v > KNEE) & (v < 10 * KNEE)).sum())
    print("channels below / just above the knee:", below, above)
    assert below >= 20 and above >= 20
    assert (k["t"] > 255.5).any() and (k["t"][k["ordinary"]] == 0).any()                  # saturated channels; channels clamped at 0


def test_restatement_on_known_values():
    """Black is 0, a huge value saturates at (uint8)(256 * 0.999f) = 255, and v = 1 gives gamma 1.0 -> 255."""
    t, _ = restate(np.array([[0, 0, 0], [1e6, 1e6, 1e6], [0.5, 0.5, 0.5]], F), 1.0)
    assert (t[0] == 0).all() and (t[1].astype(np.uint8) == 255).all()
    y = 0.5 * (0.222485 + 0.716905 + 0.060610)
    want = 256 * (1.055 * (1 - np.exp(-y)) ** (1 / 2.4) - 0.055)
    assert abs(float(t[2, 0]) - want) < 1e-3


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


GUARD = 64


def device_image(ctx, dev, pixels, scale, fmt):
    """The image of pixels [H, W, C] in a 0xAA-filled buffer with GUARD bytes behind it: (image bytes, guard bytes)."""
    h, w, comps = pixels.shape
    size = ctx.lib.slrhip_tonemap_bytes(w, h, fmt)
    out = dev.put(np.full(size + GUARD, 0xAA, np.uint8))
    ctx.tonemap_into(w, h, comps, dev.put(pixels), out, size, scale, fmt)
    ctx.synchronize()
    got = dev.get(out, size + GUARD, np.uint8)
    return got[:size], got[size:]


@pytest.mark.gpu
@pytest.mark.parametrize("comps", [3, 16])
@pytest.mark.parametrize("width, height", SHAPES)
def test_bmp_layout_equals_the_host_function(ctx, width, height, comps):
    with binding.DeviceBlocks() as dev:
        for scale in SCALES:
            assert_input_condition(width, height, comps, scale)
            k = case(width, height, comps, scale)
            want = host_bmp(k["pixels"], width, height, scale)
            got, guard = device_image(ctx, dev, k["pixels"], scale, abi.IMAGE_BGR8_BMP)
            assert len(got) == (3 * width + width % 4) * height
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, "%d x %d x %d, scale %g: %d bytes differ, first at %d: %d vs %d" % (width, height, comps, scale, len(bad), bad[0], got[bad[0]], want[bad[0]])
            assert (guard == 0xAA).all(), "bytes behind the image were written"


@pytest.mark.gpu
@pytest.mark.parametrize("comps", [3, 16])
@pytest.mark.parametrize("width, height", SHAPES)
def test_rgba8_is_the_bmp_reordered(ctx, width, height, comps):
    with binding.DeviceBlocks() as dev:
        for scale in SCALES:
            k = case(width, height, comps, scale)
            got, guard = device_image(ctx, dev, k["pixels"], scale, abi.IMAGE_RGBA8)
            assert len(got) == 4 * width * height
            got = got.reshape(height, width, 4)
            assert (got[:, :, 3] == 255).all()
            assert np.array_equal(got, rgba_of_bmp(host_bmp(k["pixels"], width, height, scale), width, height))
            assert (guard == 0xAA).all(), "bytes behind the image were written"


@pytest.mark.gpu
def test_argument_errors(ctx):
    w, h, comps, scale = 37, 21, 3, 1.0
    k = case(w, h, comps, scale)
    with binding.DeviceBlocks() as dev:
        color = dev.put(k["pixels"])
        frame = 4 * w * h * comps
        size = ctx.lib.slrhip_tonemap_bytes(w, h, abi.IMAGE_BGR8_BMP)
        room = 4 * w * h + GUARD                                     # enough for either format
        out = dev.put(np.full(room, 0xAA, np.uint8))
        big = dev.put(np.full(2 * frame, 0xAA, np.uint8))            # room for overlapping ranges: the colour is copied into it below
        binding._hip_check(dev.hip.hipMemcpy(big + frame, k["pixels"].ctypes.data, frame, 1), "hipMemcpy")

        def desc(**over):
            f = dict(width=w, height=h, components=comps, format=abi.IMAGE_BGR8_BMP, color=color, output=out, output_bytes=size, scale=scale, reserved=0)
            f.update(over)
            return abi.TonemapDesc(**f)
        lib = ctx.lib
        bad = [dict(color=None), dict(output=None), dict(color=color + 2), dict(output=out + 1), dict(output=out + 2), dict(width=0), dict(height=0),
               dict(width=65536, height=32768), dict(components=4), dict(components=0), dict(components=15), dict(format=2), dict(format=0xFFFFFFFF),
               dict(reserved=1), dict(output_bytes=size - 1), dict(output_bytes=0), dict(format=abi.IMAGE_RGBA8, output_bytes=4 * w * h - 1),
               dict(output=color), dict(color=big + frame, output=big + frame), dict(color=big + frame, output=big + frame - size + 4),
               dict(color=big + frame, output=big + 2 * frame - 4, output_bytes=1 << 20)]
        for over in bad:
            d = desc(**over)
            assert lib.slrhip_tonemap(ctx.handle, C.byref(d), None) == INVALID, over
            assert b"slrhip_tonemap" in lib.slrhip_last_error_string()
        assert lib.slrhip_tonemap(ctx.handle, None, None) == INVALID and lib.slrhip_tonemap(None, C.byref(desc()), None) == INVALID
        ctx.synchronize()
        assert (dev.get(out, room, np.uint8) == 0xAA).all() and (dev.get(big, frame, np.uint8) == 0xAA).all(), "a refused call wrote"
        assert np.array_equal(dev.get(color, frame, np.uint8), k["pixels"].view(np.uint8).reshape(-1)) and np.array_equal(dev.get(big + frame, frame, np.uint8), k["pixels"].view(np.uint8).reshape(-1))
        # adjacent ranges do not overlap: the image ends where the colour begins
        want = host_bmp(k["pixels"], w, h, scale)
        d = desc(color=big + frame, output=big + frame - size)
        assert lib.slrhip_tonemap(ctx.handle, C.byref(d), None) == 0
        ctx.synchronize()
        assert np.array_equal(dev.get(big + frame - size, size, np.uint8), want)
        # the good descriptor works after all the refusals; any scale is accepted
        assert lib.slrhip_tonemap(ctx.handle, C.byref(desc()), None) == 0
        ctx.synchronize()
        got = dev.get(out, room, np.uint8)
        assert np.array_equal(got[:size], want) and (got[size:] == 0xAA).all()
        for s in (0.0, float("inf"), float("nan")):                 # (bytes the definition fixes: 0 or 255)
            assert lib.slrhip_tonemap(ctx.handle, C.byref(desc(scale=s)), None) == 0
            ctx.synchronize()
            assert np.array_equal(dev.get(out, size, np.uint8), host_bmp(k["pixels"], w, h, s)), s


# torch ships its own copy of the HIP runtime, and only one copy can open the device in a process.  The checks on torch tensors and
# torch streams therefore run in ONE fresh child process that imports torch BEFORE libslrhip.so is loaded; each prints its own mark.
@pytest.fixture(scope="module")
def torch_child():
    src = ("import sys, torch\nsys.path[:0] = [%r, %r]\nimport test_tonemap as T\nT._torch_checks()\n" % (ROOT, os.path.join(ROOT, "tests")))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", src]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    return p.stdout[-6000:] + "\n" + p.stderr[-3000:]


def _torch_checks():
    for check in (_stream_check, _end_to_end_check):
        try:
            check()
            print("OK", check.__name__, flush=True)
        except Exception:
            import traceback
            traceback.print_exc()
            print("FAILED", check.__name__, flush=True)


@pytest.mark.gpu
def test_context_without_a_scene_on_another_stream(torch_child):
    assert "OK _stream_check" in torch_child, torch_child


def _stream_check():
    import torch
    w, h = 37, 21
    fresh = Context()                                               # no scene, no render_begin
    try:
        for comps in (3, 16):
            k = case(w, h, comps, 0.37)
            side = torch.cuda.Stream()
            color = torch.from_numpy(k["pixels"].copy()).cuda()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                first = fresh.tonemap(color, 0.37, abi.IMAGE_BGR8_BMP)
                second = fresh.tonemap(color, 0.37, abi.IMAGE_BGR8_BMP)
                rgba = fresh.tonemap(color, 0.37)
            side.synchronize()
            assert first.dtype == torch.uint8 and first.is_cuda and first.data_ptr() != second.data_ptr()
            assert torch.equal(first, second)
            want = host_bmp(k["pixels"], w, h, 0.37)
            assert np.array_equal(first.cpu().numpy(), want)
            assert rgba.shape == (h, w, 4) and np.array_equal(rgba.cpu().numpy(), rgba_of_bmp(want, w, h))
            with pytest.raises(ValueError):
                fresh.tonemap(color[:, ::2], 0.37)                  # not contiguous
    finally:
        fresh.close()


def compare_where_safe(got, want, fb, width, height, scale, what):
    """Rendered values are not in the safe set: BGR8_BMP images got / want must agree in every byte whose restated t clears the
    margin, and those must be at least 90 % of all colour bytes (expected: about 97.7 %)."""
    t, _ = restate(np.ascontiguousarray(fb, F).reshape(width * height, -1), scale)
    tt = t.astype(np.float64)
    clear = np.abs(tt - np.maximum(np.rint(tt), 1.0)) > MARGIN
    mask = np.zeros((height, 3 * width + width % 4), bool)
    mask[:, :3 * width] = clear.reshape(height, width, 3)[::-1, :, ::-1].reshape(height, 3 * width)
    mask[:, 3 * width:] = True                                      # the padding is compared always
    share = float(clear.mean())
    differ = int((got != want).sum())
    print("%s: %.2f %% of the colour bytes clear the margin; %d bytes differ in all" % (what, 100 * share, differ))
    assert share >= 0.90, share
    assert np.array_equal(got[mask.reshape(-1)], want[mask.reshape(-1)]), what
    assert np.array_equal(want[mask.reshape(-1)], bmp_bytes(t, width, height)[mask.reshape(-1)]), what + ": the host function vs the restatement"


@pytest.mark.gpu
def test_rendered_frame_end_to_end(torch_child):
    assert "OK _end_to_end_check" in torch_child, torch_child


def _end_to_end_check():
    import torch
    from oracle import binding as ob
    from slr_amd import scenes
    w, h, spp = 32, 32, 8
    sc = scenes.cornell_box_spheres(1.0, 16, 8, "matte")
    st = ob.settings(w, h, seed=5)
    cam = sc.camera
    sensitivity = cam.sensitivity if cam.sensitivity > 0 else float(F(1.0 / (np.pi * float(F(cam.lens_radius)) ** 2))) if cam.lens_radius > 0 else 1.0
    scale = float(F(F(st.brightness) / F(spp)) * F(sensitivity))    # as slr_amd/host.py computes it
    for mode, comps in ((abi.MODE_RGB, 3), (abi.MODE_SPECTRAL, 16)):
        c = Context(mode=mode)
        try:
            c.upload_scene(sc)
            c.render_begin(st)
            c.render(0, spp)
            frame = torch.empty((h, w, comps), dtype=torch.float32, device="cuda")
            s = torch.cuda.current_stream()
            c.resolve_into(frame.data_ptr(), frame.numel(), s.cuda_stream)
            got = c.tonemap(frame, scale, abi.IMAGE_BGR8_BMP)
            rgba = c.tonemap(frame, scale)
            torch.cuda.synchronize()
            fb = c.read_framebuffer()
            assert np.array_equal(frame.cpu().numpy(), fb)
            want = host_bmp(fb, w, h, scale)
            assert 8 < want.mean() < 247, "the frame is black or white: the comparison would say nothing"
            compare_where_safe(got.cpu().numpy(), want, fb, w, h, scale, "cornell %d components" % comps)
            assert np.array_equal(rgba.cpu().numpy(), rgba_of_bmp(got.cpu().numpy(), w, h))
            # the same through the binding's own staging, without torch
            assert np.array_equal(c.frame_image(scale), got.cpu().numpy())
        finally:
            c.close()


@pytest.mark.gpu
def test_host_program_with_device_tonemap(tmp_path, capsys):
    """python -m slr_amd.host --denoise 2 with and without --device-tonemap: the same files, equal headers and sizes, and equal pixel
    bytes wherever the restated t of the frame clears the margin."""
    from test_scene_language import cornell_script
    w, h, spp = 48, 36, 4
    script = tmp_path / "box.txt"
    script.write_text(cornell_script("matte").replace('"width": 320, "height": 240', '"width": %d, "height": %d' % (w, h)))
    plain, device = tmp_path / "plain", tmp_path / "device"
    plain.mkdir()
    device.mkdir()
    args = [str(script), "--samples", str(spp), "--denoise", "2"]
    assert host.main(args + ["--out", str(plain)]) == 0
    assert host.main(args + ["--out", str(device), "--device-tonemap"]) == 0
    capsys.readouterr()
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(device)) == ["000.bmp", "001.bmp", "002.bmp", "002_denoised.bmp"]
    # the frames the program tone-mapped, rendered again through the binding call for call
    from slr_amd import scene_language
    scene, settings, _ = scene_language.load_scene(str(script))
    st = abi.RenderSettings(w, h, float(settings["timeStart"]), float(settings["timeEnd"]), float(settings["brightness"]), int(settings["rngSeed"]))
    cam = scene.camera
    sensitivity = cam.sensitivity if cam.sensitivity > 0 else float(F(1.0 / (np.pi * float(F(cam.lens_radius)) ** 2))) if cam.lens_radius > 0 else 1.0
    frames = {}
    c = Context()
    try:
        c.upload_scene(scene)
        c.render_begin(st)
        c.statistics_begin()
        done = 0
        for img, upto in enumerate((1, 2, 4)):
            c.render(done, upto - done)
            done = upto
            frames["%03u.bmp" % img] = (c.read_framebuffer(), float(F(F(st.brightness) / F(upto)) * F(sensitivity)))
        c.render_features(host.DENOISE_CHANNELS, spp)
        frames["002_denoised.bmp"] = (c.denoised(iterations=2), float(F(st.brightness) * F(sensitivity)))
    finally:
        c.close()
    for name in names:
        a, b = np.frombuffer((plain / name).read_bytes(), np.uint8), np.frombuffer((device / name).read_bytes(), np.uint8)
        assert len(a) == len(b) == 54 + (3 * w + w % 4) * h and np.array_equal(a[:54], b[:54]), name
        fb, scale = frames[name]
        assert np.array_equal(a[54:], host_bmp(fb, w, h, scale)), name + ": the plain run is not the host tone map of this frame"
        compare_where_safe(b[54:], a[54:], fb, w, h, scale, name)
