// slrhip_image.hip — the entry points that are pure functions of the caller's device buffers and read nothing of the render state:
// the denoiser, the image export, albedo demodulation, temporal reprojection.  The argument checks are render_plan.cpp's; here are the launches.
#include "slrhip_ctx.h"

using namespace slrhip;

extern "C" {

// The denoiser: the argument checks (render_plan.cpp), the scratch, the launch list (pt_denoise.hip).  It reads nothing of the render state.
int slrhip_denoise(slrhip_ctx* ctx, const slrhip_denoise_desc* d, void* streamPtr) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_denoise: null argument");
    if (const char* what = denoiseRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_denoise: ") + what);
    const DenoiseScratch scratch = denoiseScratch(d->width, d->height, d->components);
    HIP_TRY(hipSetDevice(ctx->device));
    if (const hipError_t e = ctx->denoiseScratch.alloc(scratch.bytes)) {
        (void)hipGetLastError();                           // the context stays usable: the next call allocates again
        return fail(SLRHIP_ERR_OUT_OF_MEMORY, std::string("slrhip_denoise: allocating the scratch: ") + hipGetErrorString(e));
    }
    uint8_t* base = ctx->denoiseScratch.ptr;
    DenoiseParams dp{};
    dp.width = d->width; dp.height = d->height; dp.components = d->components; dp.iterations = d->iterations;
    dp.color = d->color; dp.variance = d->variance; dp.normal = d->normal; dp.distance = d->distance; dp.coverage = d->coverage;
    dp.output = d->output; dp.outputVariance = d->output_variance;
    dp.sigmaLuminance = d->sigma_luminance; dp.sigmaDistance = d->sigma_distance; dp.normalPowerLog2 = d->normal_power_log2;
    dp.guides = reinterpret_cast<float4*>(base + scratch.guides);
    for (int k = 0; k < 2; ++k) {
        dp.planes[k] = reinterpret_cast<float4*>(base + scratch.planes[k]);
        dp.yv[k] = reinterpret_cast<float2*>(base + scratch.yv[k]);
    }
    launchDenoise(dp, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

// The image export: the argument checks (render_plan.cpp), one launch (pt_tonemap.hip).  It reads nothing of the render state.
int slrhip_tonemap(slrhip_ctx* ctx, const slrhip_tonemap_desc* d, void* streamPtr) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_tonemap: null argument");
    if (const char* what = tonemapRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_tonemap: ") + what);
    HIP_TRY(hipSetDevice(ctx->device));
    launchTonemap(*d, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

// Albedo demodulation: the argument checks (render_plan.cpp), one launch (pt_albedo.hip).  It reads nothing of the render state.
int slrhip_modulate(slrhip_ctx* ctx, const slrhip_modulate_desc* d, void* streamPtr) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_modulate: null argument");
    if (const char* what = modulateRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_modulate: ") + what);
    HIP_TRY(hipSetDevice(ctx->device));
    launchModulate(*d, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

// Temporal reprojection: the argument checks (render_plan.cpp), one launch (pt_reproject.hip).  It reads nothing of the render state.
int slrhip_reproject(slrhip_ctx* ctx, const slrhip_reproject_desc* d, void* streamPtr) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_reproject: null argument");
    if (const char* what = reprojectRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_reproject: ") + what);
    HIP_TRY(hipSetDevice(ctx->device));
    launchReproject(*d, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

} // extern "C"
