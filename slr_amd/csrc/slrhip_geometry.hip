// slrhip_geometry.hip — moving the vertices of the uploaded scene (flat, or with instances in a context created with
// SLRHIP_FLAG_DYNAMIC_INSTANCED as well) without a scene upload: slrhip_set_vertices replaces a range of
// the kept vertex array and rebuilds, on the device and in place, every record and every box that depends on vertices;
// slrhip_geometry_status reads its status word; slrhip_debug_geometry reads back what it keeps.  The argument checks are
// render_plan.cpp's (geometryUpdateRefusal2), the kernels pt_geometry.hip's, the arithmetic pt_triangle.h's, the child rule of the refit
// pt_refit.h's, the quantizer pt_quantize.h's; here are the launch and the read-outs.
#include "../../include/slrhip_debug.h"
#include "pt_geometry.h"
#include "slrhip_ctx.h"

using namespace slrhip;

namespace {

// The lights segment of the staged shade tables (packShadeTables: RGB materials | lights | ..; spectral materials | spectra | pool |
// lights | ..), or nullptr when the tables are not staged or the segment is not the light records' size (never).
float4* stagedLights(slrhip_ctx* ctx) {
    const DevScene& sc = ctx->scene;
    if (!sc.shadeTables || sc.numLights == 0) return nullptr;
    const uint32_t seg = ctx->config.mode == SLRHIP_MODE_SPECTRAL ? 3u : 1u;
    const uint32_t begin = sc.tableEnd[seg - 1u], end = sc.tableEnd[seg];
    if (end < begin || (size_t)(end - begin) != (size_t)sc.numLights * 9u || end > ctx->shadeTables.count) return nullptr;
    return ctx->shadeTables.ptr + begin;
}

int refusal(slrhip_ctx* ctx, const void* deviceSrc, uint32_t first, uint32_t count, const char** what) {
    const bool have = ctx->haveScene;
    return geometryUpdateRefusal2(have, (ctx->config.flags & SLRHIP_FLAG_DYNAMIC_GEOMETRY) != 0, (ctx->config.flags & SLRHIP_FLAG_DYNAMIC_INSTANCED) != 0,
                                  have ? ctx->treeBuilder : 0u, have ? ctx->scene.numInstances : 0u, have && ctx->geometryKept ? ctx->geoNumVertices : 0u, deviceSrc,
                                  first, count, what);
}

} // namespace

extern "C" {

int slrhip_set_vertices(slrhip_ctx* ctx, const slrhip_vertex* deviceSrc, uint32_t first, uint32_t count, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_vertices: null context");
    const char* what = nullptr;
    if (const int rc = refusal(ctx, deviceSrc, first, count, &what)) return fail(rc, std::string("slrhip_set_vertices: ") + what);
    const uint32_t numLevels = (uint32_t)ctx->geoLevelFirst.size() - 1u;
    const bool instanced = ctx->haveScene && ctx->scene.numInstances != 0;
    if (!ctx->geometryKept || ctx->geoInstanced != instanced || ctx->geoLevelFirst.size() < 2 || numLevels > kMaxTreeLevels ||
        ctx->geoLevelFirst.back() != (instanced ? ctx->topLevelFirst.back() : ctx->scene.numNodes))
        return fail(SLRHIP_ERR_HIP, "slrhip_set_vertices: the tree has no level table (internal error)");
    const uint32_t numMeshLevels = instanced ? (uint32_t)ctx->geoMeshLevelFirst.size() - 1u : 0u;
    if (instanced && (ctx->geoMeshLevelFirst.size() < 2 || numMeshLevels > kMaxTreeLevels || ctx->geoMeshLevelFirst.back() != ctx->geoMeshLevelNodes.count ||
                      ctx->geoMeshRoots.count * 2u != ctx->meshBoxes.count || ctx->geoMeshRoots.count > ctx->scene.numInstances))
        return fail(SLRHIP_ERR_HIP, "slrhip_set_vertices: the mesh trees have no level list (internal error)");
    HIP_TRY(hipSetDevice(ctx->device));
    const DevScene& sc = ctx->scene;
    GeometryUpdate u{};
    u.src = reinterpret_cast<const float*>(deviceSrc);
    u.first = first; u.count = count;
    u.numVertices = ctx->geoNumVertices; u.numTriangles = ctx->geoNumTriangles; u.numLeafTris = (uint32_t)ctx->bvhLeafRefs;
    u.numNodes = sc.numNodes; u.numLights = ctx->geoNumLights; u.numLevels = numLevels;
    u.vertices = reinterpret_cast<float*>(ctx->geoVertices.ptr);
    u.triangles = ctx->geoTriangles.ptr;
    u.leafTris = reinterpret_cast<float4*>(ctx->leafTris.ptr);
    u.leafBoxes = ctx->geoLeafBoxes.ptr;
    u.shadeTris = reinterpret_cast<float4*>(ctx->shadeTris.ptr);
    u.lightTris = reinterpret_cast<float4*>(ctx->lightTris.ptr);
    u.stagedLights = stagedLights(ctx);
    u.triUV = ctx->geoHasTriUV ? ctx->triUV.ptr : nullptr;
    u.alphaTris = ctx->alphaTris.ptr; u.numAlphaRecords = ctx->geoNumAlphaRecords;
    u.nodes = reinterpret_cast<float4*>(ctx->nodes.ptr);
    u.nodesQ = sc.nodesQ ? reinterpret_cast<float4*>(ctx->nodesQ.ptr) : nullptr;
    u.status = ctx->geometryStatus.ptr;
    std::copy(ctx->geoLevelFirst.begin(), ctx->geoLevelFirst.end(), u.levelFirst);
    if (instanced) {
        u.numInstances = sc.numInstances; u.numMeshes = (uint32_t)ctx->geoMeshRoots.count; u.numMeshLevels = numMeshLevels;
        u.meshLevelNodes = ctx->geoMeshLevelNodes.ptr; u.meshRoots = ctx->geoMeshRoots.ptr;
        u.instances = reinterpret_cast<const float4*>(ctx->instances.ptr);
        u.meshBoxes = ctx->meshBoxes.ptr; u.instBoxes = ctx->instBoxes.ptr;
        std::copy(ctx->geoMeshLevelFirst.begin(), ctx->geoMeshLevelFirst.end(), u.meshLevelFirst);
        if (ctx->topSeatReady && ctx->topPrimitives > sc.numInstances) {     // slrhip_rebuild_top_level's packet boxes follow the vertices
            u.numTopPackets = ctx->topPrimitives - sc.numInstances;
            u.topPacketRefs = ctx->topRefs.ptr + sc.numInstances; u.topPacketBoxes = ctx->topPacketBoxes.ptr;
        }
    }
    // every array is updated in place: no pointer of ctx->scene changes, and the next launches read the new geometry
    ctx->geoLastLaunches = launchGeometryUpdate(u, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_geometry_status(slrhip_ctx* ctx, uint32_t* bits, void* streamPtr) {
    if (!ctx || !bits) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_geometry_status: null argument");
    *bits = 0;
    if (!ctx->geometryStatus.ptr) return SLRHIP_OK;      // nothing was ever kept: no update can have run
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemcpyAsync(bits, ctx->geometryStatus.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(ctx->geometryStatus.ptr, 0, sizeof(uint32_t), s));
    HIP_TRY(hipStreamSynchronize(s));
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_set_vertices, without a context.
int slrhip_debug_geometry_update_check(int32_t haveScene, int32_t dynamic, uint32_t treeBuilder, uint32_t numInstances, uint32_t numVertices,
                                       const void* deviceSrc, uint32_t first, uint32_t count) {
    const char* what = nullptr;
    if (const int rc = geometryUpdateRefusal(haveScene != 0, dynamic != 0, treeBuilder, numInstances, numVertices, deviceSrc, first, count, &what))
        return fail(rc, std::string("slrhip_set_vertices: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the same for a context that may keep a scene with instances — the check slrhip_set_vertices calls.
int slrhip_debug_geometry_update_check2(int32_t haveScene, int32_t dynamic, int32_t instancedKept, uint32_t treeBuilder, uint32_t numInstances,
                                        uint32_t numVertices, const void* deviceSrc, uint32_t first, uint32_t count) {
    const char* what = nullptr;
    if (const int rc = geometryUpdateRefusal2(haveScene != 0, dynamic != 0, instancedKept != 0, treeBuilder, numInstances, numVertices, deviceSrc, first, count,
                                              &what))
        return fail(rc, std::string("slrhip_set_vertices: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): what slrhip_set_vertices keeps and rewrites beyond the tree, to host memory.
int slrhip_debug_geometry(slrhip_ctx* ctx, uint32_t what, void* hostDst, size_t numWords) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_geometry: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_geometry: no scene uploaded");
    if (!(ctx->config.flags & SLRHIP_FLAG_DYNAMIC_GEOMETRY))
        return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_debug_geometry: the context was created without SLRHIP_FLAG_DYNAMIC_GEOMETRY");
    if (!ctx->geometryKept) return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_debug_geometry: slrhip_set_vertices does not cover this scene (spatial splits, or instances without SLRHIP_FLAG_DYNAMIC_INSTANCED)");
    const void* src = nullptr;
    size_t need = 0;
    switch (what) {
    case 0: need = 32; break;
    case 1: src = ctx->geoVertices.ptr; need = (size_t)ctx->geoNumVertices * 11u; break;
    case 2: src = ctx->lightTris.ptr; need = (size_t)ctx->geoNumLights * 36u; break;
    case 3:
        src = stagedLights(ctx); need = (size_t)ctx->geoNumLights * 36u;
        if (!src) return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_debug_geometry: the shade tables are not staged");
        break;
    case 4: src = ctx->triUV.ptr; need = ctx->geoHasTriUV ? (size_t)ctx->geoNumTriangles * 8u : 0u; break;
    case 5: src = ctx->alphaTris.ptr; need = (size_t)ctx->geoNumAlphaRecords * 8u; break;
    case 6: need = 48; break;
    case 7: src = ctx->geoMeshLevelNodes.ptr; need = ctx->geoInstanced ? ctx->geoMeshLevelNodes.count : 0u; break;
    case 8: src = ctx->geoLeafBoxes.ptr; need = (size_t)ctx->bvhLeafRefs * 8u; break;
    case 9: src = ctx->geoMeshRoots.ptr; need = ctx->geoInstanced ? ctx->geoMeshRoots.count : 0u; break;
    case 10:
        src = ctx->topPacketBoxes.ptr;
        need = ctx->geoInstanced && ctx->topSeatReady && ctx->topPrimitives > ctx->scene.numInstances ? (size_t)(ctx->topPrimitives - ctx->scene.numInstances) * 8u : 0u;
        break;
    default: return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_geometry: unknown `what`");
    }
    if (numWords < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_geometry: host_dst too small");
    if (what == 0) {
        uint32_t* out = static_cast<uint32_t*>(hostDst);
        std::fill(out, out + 32, 0u);
        const uint32_t levels = (uint32_t)ctx->geoLevelFirst.size() - 1u;
        out[0] = levels; out[1] = ctx->scene.numNodes; out[2] = ctx->geoNumVertices; out[3] = ctx->geoNumTriangles; out[4] = ctx->geoNumLights;
        out[5] = stagedLights(ctx) ? 1u : 0u; out[6] = kRefitGroupNodes;
        std::copy(ctx->geoLevelFirst.begin(), ctx->geoLevelFirst.end(), out + 7);
        uint32_t* tail = out + 7 + levels + 1;            // levels <= kMaxTreeLevels = 21: three words fit
        tail[0] = ctx->geoHasTriUV ? ctx->geoNumTriangles * 2u : 0u; tail[1] = ctx->geoNumAlphaRecords; tail[2] = ctx->geoLastLaunches;
        return SLRHIP_OK;
    }
    if (what == 6) {
        uint32_t* out = static_cast<uint32_t*>(hostDst);
        std::fill(out, out + 48, 0u);
        out[0] = ctx->geoInstanced ? 1u : 0u; out[7] = (uint32_t)ctx->bvhLeafRefs; out[8] = ctx->geoLastLaunches;
        if (!ctx->geoInstanced) return SLRHIP_OK;
        const uint32_t meshLevels = (uint32_t)ctx->geoMeshLevelFirst.size() - 1u;
        out[1] = (uint32_t)ctx->geoLevelFirst.size() - 1u; out[2] = meshLevels; out[3] = (uint32_t)ctx->geoMeshRoots.count; out[4] = ctx->scene.numInstances;
        out[5] = ctx->geoLevelFirst.back(); out[6] = ctx->geoMeshLevelFirst.back();
        out[9] = ctx->topSeatReady && ctx->topPrimitives > ctx->scene.numInstances ? ctx->topPrimitives - ctx->scene.numInstances : 0u;
        std::copy(ctx->geoMeshLevelFirst.begin(), ctx->geoMeshLevelFirst.end(), out + 16);      // at most kMaxTreeLevels + 1 = 22 words
        return SLRHIP_OK;
    }
    if (need == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, src, need * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // extern "C"
