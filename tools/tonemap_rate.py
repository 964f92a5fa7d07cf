"""What the image export on the device (slrhip_tonemap) costs on the headline Cornell frame (1280x720), for 3 components (an RGB
context) and 16 (a spectral one), next to what a host paid for the same image before it existed.

The input is a real render's: --spp passes, the frame of sums resolved into device memory once, scale = brightness / spp x
sensitivity as slr_amd/host.py computes it.  A: the device call (SLRHIP_IMAGE_BGR8_BMP, and SLRHIP_IMAGE_RGBA8) bracketed by two HIP
events on one stream (torch.cuda.Event), after --warmup calls: the median, the fastest and the slowest of --reps calls.  Against that:
the bytes the kernel must move, 4 C read and 3 (or 4) written per pixel, over the HBM peak DESIGN.md states its fractions against.
B: the wall time of Context.read_framebuffer() followed by slrhip_tonemap_bgr8 on the host, the only path there was, same counts;
and of Context.frame_image(), the path `--device-tonemap` takes (resolve, tone-map, copy the 8-bit rows back, with its allocations).
The two images are compared: bytes that differ (only where exp or pow differ in a last bit: include/slrhip.h).  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch  # before libslrhip.so is loaded: the library binds to torch's copy of the HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from slr_amd import Context, abi, scenes  # noqa: E402

HBM_BYTES_PER_SECOND = 8.0e12          # the peak DESIGN.md 7.2 states its fractions against


def spread(values):
    return dict(median_ms=float(np.median(values)), min_ms=float(min(values)), max_ms=float(max(values)))


def measure(mode, w, h, spp, warmup, reps):
    ctx = Context(mode=mode)
    sc = scenes.cornell_box_spheres(w / h, 48, 24, "matte")
    ctx.upload_scene(sc)
    st = abi.RenderSettings(w, h, 0.0, 0.0, 1.0, abi.DEFAULT_SEED)
    ctx.render_begin(st)
    ctx.render(0, spp)
    comps = ctx.components
    cam = sc.camera
    sensitivity = cam.sensitivity if cam.sensitivity > 0 else float(np.float32(1.0 / (np.pi * float(np.float32(cam.lens_radius)) ** 2))) if cam.lens_radius > 0 else 1.0
    scale = float(np.float32(np.float32(st.brightness) / np.float32(spp)) * np.float32(sensitivity))
    dev = "cuda:%d" % ctx.device
    stream = torch.cuda.current_stream(ctx.device)
    color = torch.empty(h * w * comps, dtype=torch.float32, device=dev)
    ctx.resolve_into(color.data_ptr(), color.numel(), stream.cuda_stream)
    out = dict(components=comps, scale=scale)
    images = {}
    for name, fmt in (("bgr8_bmp", abi.IMAGE_BGR8_BMP), ("rgba8", abi.IMAGE_RGBA8)):
        size = ctx.lib.slrhip_tonemap_bytes(w, h, fmt)
        image = torch.empty(size, dtype=torch.uint8, device=dev)
        ms = []
        for i in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            ctx.tonemap_into(w, h, comps, color.data_ptr(), image.data_ptr(), size, scale, fmt, stream)
            b.record(stream)
            b.synchronize()
            if i >= warmup:
                ms.append(a.elapsed_time(b))
        need = w * h * 4 * comps + size
        t = spread(ms)
        out[name] = dict(call=t, bytes_moved=need, bytes_per_pixel=need / (w * h), floor_ms=need / HBM_BYTES_PER_SECOND * 1e3,
                         bytes_per_second=need / (t["median_ms"] * 1e-3), fraction_of_hbm_rate=need / HBM_BYTES_PER_SECOND / (t["median_ms"] * 1e-3))
        images[name] = image.cpu().numpy()

    lib = ctx.lib
    bmp = np.zeros((3 * w + w % 4) * h, np.uint8)
    read_ms, host_ms, device_path_ms = [], [], []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        fb = ctx.read_framebuffer()
        t1 = time.perf_counter()
        assert lib.slrhip_tonemap_bgr8(fb.ctypes.data, w, h, comps, C.c_float(scale), bmp.ctypes.data, bmp.size) == 0
        t2 = time.perf_counter()
        got = ctx.frame_image(scale)
        t3 = time.perf_counter()
        if i >= warmup:
            read_ms.append((t1 - t0) * 1e3)
            host_ms.append((t2 - t1) * 1e3)
            device_path_ms.append((t3 - t2) * 1e3)
    out["host_path"] = dict(read_framebuffer=spread(read_ms), slrhip_tonemap_bgr8=spread(host_ms),
                            total_median_ms=float(np.median(np.array(read_ms) + np.array(host_ms))), float_bytes_read_back=int(fb.nbytes))
    out["device_path_frame_image"] = dict(wall=spread(device_path_ms), bytes_read_back=int(got.nbytes))
    out["bytes_differing_from_host"] = int((images["bgr8_bmp"] != bmp).sum())
    out["frame_image_equals_device_call"] = bool(np.array_equal(got, images["bgr8_bmp"]))
    out["mean_byte"] = float(bmp.mean())
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    out = dict(width=args.width, height=args.height, spp=args.spp, warmup=args.warmup, reps=args.reps, hbm_bytes_per_second=HBM_BYTES_PER_SECOND)
    out["rgb"] = measure(abi.MODE_RGB, args.width, args.height, args.spp, args.warmup, args.reps)
    out["spectral"] = measure(abi.MODE_SPECTRAL, args.width, args.height, args.spp, args.warmup, args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
