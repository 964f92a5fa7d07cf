// slrhip_instances.hip — moving what is placed in the uploaded scene without a scene upload: slrhip_set_instance_transforms gives
// instances new matrices and refits the top-level tree on the device, slrhip_set_camera replaces the camera, and
// slrhip_debug_top_level reads the top level back.  The argument checks are render_plan.cpp's (instanceUpdateRefusal), the kernels
// pt_instances.hip's, the box arithmetic pt_instance.h's, the camera constants scene_prep.cpp's; here are the launch and the read-out.
#include "../../include/slrhip_debug.h"
#include "pt_instance.h"
#include "slrhip_ctx.h"

using namespace slrhip;

extern "C" {

int slrhip_set_instance_transforms(slrhip_ctx* ctx, const slrhip_instance_transform* deviceSrc, uint32_t first, uint32_t count, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_instance_transforms: null context");
    const char* what = nullptr;
    if (const int rc = instanceUpdateRefusal(ctx->haveScene, ctx->haveScene ? ctx->scene.numInstances : 0u, deviceSrc, first, count, &what))
        return fail(rc, std::string("slrhip_set_instance_transforms: ") + what);
    const uint32_t numLevels = (uint32_t)ctx->topLevelFirst.size() - 1u;
    if (ctx->topLevelFirst.size() < 2 || numLevels > kMaxTopLevels)
        return fail(SLRHIP_ERR_HIP, "slrhip_set_instance_transforms: the top-level tree has no level table (internal error)");
    HIP_TRY(hipSetDevice(ctx->device));
    InstanceUpdate u{};
    u.src = reinterpret_cast<const float4*>(deviceSrc);
    u.first = first; u.count = count;
    u.numInstances = ctx->scene.numInstances; u.numMeshes = (uint32_t)(ctx->meshBoxes.count / 2u);
    u.topNodes = ctx->topLevelFirst.back(); u.numLevels = numLevels;
    u.instances = reinterpret_cast<float4*>(ctx->instances.ptr);
    u.meshBoxes = ctx->meshBoxes.ptr; u.instBoxes = ctx->instBoxes.ptr;
    u.nodes = reinterpret_cast<float4*>(ctx->nodes.ptr);
    u.status = ctx->instanceStatus.ptr;
    std::copy(ctx->topLevelFirst.begin(), ctx->topLevelFirst.end(), u.levelFirst);
    // every array is updated in place: no pointer of ctx->scene changes, and the next launches read the new placement
    launchInstanceUpdate(u, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_instances_status(slrhip_ctx* ctx, uint32_t* bits, void* streamPtr) {
    if (!ctx || !bits) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_instances_status: null argument");
    *bits = 0;
    if (!ctx->instanceStatus.ptr) return SLRHIP_OK;      // no instanced scene was ever uploaded: no update can have run
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemcpyAsync(bits, ctx->instanceStatus.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(ctx->instanceStatus.ptr, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    return SLRHIP_OK;
}

int slrhip_set_camera(slrhip_ctx* ctx, const slrhip_camera* camera) {
    if (!ctx || !camera) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_camera: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_set_camera: no scene uploaded");
    ctx->scene.camera = prepareCamera(*camera);          // passed to every launch by value: the next launches see the new camera
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_set_instance_transforms, without a context.
int slrhip_debug_instance_update_check(int32_t haveScene, uint32_t numInstances, const void* deviceSrc, uint32_t first, uint32_t count) {
    const char* what = nullptr;
    if (const int rc = instanceUpdateRefusal(haveScene != 0, numInstances, deviceSrc, first, count, &what))
        return fail(rc, std::string("slrhip_set_instance_transforms: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the top level of an instanced scene, to host memory.
int slrhip_debug_top_level(slrhip_ctx* ctx, uint32_t what, void* hostDst, size_t numWords) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_top_level: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_top_level: no scene uploaded");
    const DevScene& sc = ctx->scene;
    if (sc.numInstances == 0 || ctx->topLevelFirst.size() < 2) return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_debug_top_level: the scene has no instances");
    const uint32_t levels = (uint32_t)ctx->topLevelFirst.size() - 1u, topNodes = ctx->topLevelFirst.back();
    const void* src = nullptr;
    size_t need = 0;
    switch (what) {
    case 0: src = ctx->nodes.ptr; need = (size_t)topNodes * 32u; break;
    case 1: need = 32; break;
    case 2: src = ctx->instances.ptr; need = (size_t)sc.numInstances * 36u; break;
    case 3: src = ctx->instBoxes.ptr; need = (size_t)sc.numInstances * 8u; break;
    case 4: src = ctx->nodes.ptr; need = (size_t)sc.numNodes * 32u; break;
    case 5: src = ctx->meshBoxes.ptr; need = ctx->meshBoxes.count * 4u; break;
    default: return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_top_level: unknown `what`");
    }
    if (numWords < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_top_level: host_dst too small");
    if (what == 1) {
        uint32_t* out = static_cast<uint32_t*>(hostDst);
        std::fill(out, out + 32, 0u);
        out[0] = levels; out[1] = topNodes; out[2] = sc.numNodes; out[3] = sc.numInstances; out[4] = (uint32_t)(ctx->meshBoxes.count / 2u);
        out[5] = kRefitGroupNodes;
        std::copy(ctx->topLevelFirst.begin(), ctx->topLevelFirst.end(), out + 8);
        return SLRHIP_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, src, need * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // extern "C"
