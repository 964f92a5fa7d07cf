// slrhip_environment.hip — the environment light from device memory: slrhip_set_environment swaps the environment sphere of the
// uploaded scene without a scene upload, and slrhip_debug_environment reads an environment's arrays back.  The argument checks are
// render_plan.cpp's (environmentRefusal), the kernels pt_envmap.hip's, the arithmetic pt_envmap.h's; here are the arrays and the launch.
#include "../../include/slrhip_debug.h"
#include "pt_envmap.h"
#include "slrhip_ctx.h"

using namespace slrhip;

namespace {

// An array of the new environment: the context's own if it is large enough, else a fresh block that replaces it once every block of
// the call exists (the old environment renders on if one of them cannot be had).
template <typename T>
struct Grown {
    slrhip_ctx::DevArray<T>& own;
    slrhip_ctx::DevArray<T> fresh;
    size_t count;
    Grown(slrhip_ctx::DevArray<T>& a, size_t n) : own(a), count(n) {}
    hipError_t reserve() { return own.ptr && count <= own.capacity ? hipSuccess : fresh.alloc(count); }
    void commit() {
        if (fresh.ptr) { std::swap(own.ptr, fresh.ptr); std::swap(own.base, fresh.base); std::swap(own.capacity, fresh.capacity); }
        own.count = count;                             // (`fresh` frees the old block on its way out; hipFree waits for the device)
    }
};

} // namespace

extern "C" {

int slrhip_set_environment(slrhip_ctx* ctx, const slrhip_environment_desc* d, void* streamPtr) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_environment: null argument");
    if (const char* what = environmentRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_set_environment: ") + what);
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_set_environment: no scene uploaded");
    const bool spectral = ctx->config.mode == SLRHIP_MODE_SPECTRAL;
    if (spectral && ctx->scene.gridWidth == 0)
        return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_set_environment: an environment map in spectral mode needs the scene uploaded with slrhip_scene_desc::upsampling");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    const uint32_t mw = d->width / 4u, mh = d->height / 4u;
    const size_t cells = (size_t)mw * mh;

    Grown<float> texels(ctx->envTexels, (size_t)d->width * d->height * 3u), importance(ctx->envImportance, cells);
    Grown<float> topPDF(ctx->envTopPDF, mh), topCDF(ctx->envTopCDF, mh + 1u), rowPDF(ctx->envRowPDF, cells), rowCDF(ctx->envRowCDF, cells + mh);
    Grown<double> sinRow(ctx->envSinRow, mh);
    hipError_t e = hipSuccess;
    for (Grown<float>* g : {&texels, &importance, &topPDF, &topCDF, &rowPDF, &rowCDF})
        if (e == hipSuccess) e = g->reserve();
    if (e == hipSuccess) e = sinRow.reserve();
    if (e != hipSuccess) {
        (void)hipGetLastError();                       // nothing of the context has changed: the previous environment renders on
        return fail(SLRHIP_ERR_OUT_OF_MEMORY, std::string("slrhip_set_environment: allocating the environment's arrays: ") + hipGetErrorString(e));
    }
    for (Grown<float>* g : {&texels, &importance, &topPDF, &topCDF, &rowPDF, &rowCDF}) g->commit();
    sinRow.commit();

    std::vector<double> sines(mh);
    for (uint32_t y = 0; y < mh; ++y) sines[y] = envSinRow(y, mh);
    HIP_TRY(hipMemcpyAsync(ctx->envSinRow.ptr, sines.data(), sizeof(double) * mh, hipMemcpyHostToDevice, stream));   // pageable: staged before the call returns

    EnvBuild b{};
    b.width = d->width; b.height = d->height; b.mapWidth = mw; b.mapHeight = mh;
    b.spectral = spectral;
    b.storeHalf = (d->flags & SLRHIP_ENV_STORE_HALF) != 0;
    b.toUvs = spectral && (d->flags & SLRHIP_ENV_TEXELS_RGB) != 0;
    b.src = d->texels; b.texels = ctx->envTexels.ptr; b.importance = ctx->envImportance.ptr; b.sinRow = ctx->envSinRow.ptr;
    b.topPDF = ctx->envTopPDF.ptr; b.topCDF = ctx->envTopCDF.ptr; b.rowPDF = ctx->envRowPDF.ptr; b.rowCDF = ctx->envRowCDF.ptr;
    launchEnvBuild(b, stream);
    HIP_TRY(hipGetLastError());

    DevScene& sc = ctx->scene;                         // passed to every launch by value: the next render's launches see the new light
    sc.hasEnv = 1; sc.envScale = d->scale;
    sc.envWidth = d->width; sc.envHeight = d->height; sc.envMapWidth = mw; sc.envMapHeight = mh;
    sc.envTexels = ctx->envTexels.ptr;
    sc.envTopPDF = ctx->envTopPDF.ptr; sc.envTopCDF = ctx->envTopCDF.ptr; sc.envRowPDF = ctx->envRowPDF.ptr; sc.envRowCDF = ctx->envRowCDF.ptr;
    ctx->envOwnMap = true;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_set_environment, without a context.
int slrhip_debug_environment_check(const slrhip_environment_desc* d) {
    if (!d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_environment: null argument");
    if (const char* what = environmentRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_set_environment: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): one array of the scene's environment, to host memory.
int slrhip_debug_environment(slrhip_ctx* ctx, uint32_t what, float* hostDst, size_t numFloats) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_environment: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_environment: no scene uploaded");
    const DevScene& sc = ctx->scene;
    if (!sc.hasEnv) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_environment: the scene has no environment");
    const size_t mw = sc.envMapWidth, mh = sc.envMapHeight;
    const float* src = nullptr;
    size_t need = 0;
    switch (what) {
    case 0: src = sc.envTexels; need = (size_t)sc.envWidth * sc.envHeight * 3u; break;
    case 1:
        if (!ctx->envOwnMap) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_environment: the environment came from slrhip_upload_scene, which keeps no importance map");
        src = ctx->envImportance.ptr; need = mw * mh; break;
    case 2: src = sc.envTopPDF; need = mh; break;
    case 3: src = sc.envTopCDF; need = mh + 1u; break;
    case 4: src = sc.envRowPDF; need = mw * mh; break;
    case 5: src = sc.envRowCDF; need = (mw + 1u) * mh; break;
    default: return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_environment: unknown `what`");
    }
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_environment: host_dst too small");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, src, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // extern "C"
