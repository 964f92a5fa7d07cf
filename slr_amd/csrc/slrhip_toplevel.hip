// slrhip_toplevel.hip — repairing the top-level tree after instances have moved, without a scene upload: slrhip_rebuild_top_level
// re-seats the tree's leaves in Morton order on the device and refits it, slrhip_top_level_cost is the read-out a caller decides
// with, slrhip_debug_top_level_rebuild reads the call's tables back.  The check is render_plan.cpp's (topLevelRebuildRefusal), the
// key pt_toplevel.h's, the kernels pt_toplevel.hip's and pt_instances.hip's (the refit), the plan and the cost top_level.cpp's; here
// are the first call's set-up, the launch list and the read-outs.
#include <numeric>

#include "../../include/slrhip_debug.h"
#include "pt_instance.h"
#include "pt_toplevel.h"
#include "slrhip_ctx.h"

using namespace slrhip;

static_assert(kTopSeatGroup == SLRHIP_TOP_SEAT_GROUP, "the header's limit is the kernels'");

namespace {

// the context's check, shared by the entry points; `who` prefixes the message
int refusal(const slrhip_ctx* ctx, const char* who) {
    const char* what = nullptr;
    if (const int rc = topLevelRebuildRefusal(ctx->haveScene, ctx->haveScene ? ctx->scene.numInstances : 0u, &what)) return fail(rc, std::string(who) + ": " + what);
    if (ctx->topLevelFirst.size() < 2 || ctx->topLevelFirst.size() - 1u > kMaxTopLevels)
        return fail(SLRHIP_ERR_HIP, std::string(who) + ": the top-level tree has no level table (internal error)");
    return SLRHIP_OK;
}

// The first call after an upload: the top level read back once; the slot table, the canonical references and the packets' boxes built
// on the host; everything the calls need allocated.  Synchronises.
int prepareTopSeat(slrhip_ctx* ctx) {
    const uint32_t topNodes = ctx->topLevelFirst.back(), numInstances = ctx->scene.numInstances;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<QNode> nodes(topNodes);
    HIP_TRY(hipMemcpy(nodes.data(), ctx->nodes.ptr, (size_t)topNodes * sizeof(QNode), hipMemcpyDeviceToHost));
    std::vector<uint32_t> slots(4u * (size_t)topNodes), refs(4u * (size_t)topNodes);
    uint32_t planInstances = 0;
    const uint32_t count = topLevelPlan(nodes.data(), topNodes, slots.data(), refs.data(), (uint32_t)slots.size(), &planInstances);
    if (count == 0 || planInstances != numInstances)
        return fail(SLRHIP_ERR_HIP, "slrhip_rebuild_top_level: the top-level tree does not hold every instance once (internal error)");
    slots.resize(count); refs.resize(count);
    std::vector<float4> packetBoxes(2u * (size_t)(count - numInstances));
    for (uint32_t i = 0; i < count; ++i) {
        const QNode& n = nodes[slots[i] >> 2];
        const uint32_t c = slots[i] & 3u, ref = n.child[c];
        if (((ref >> kLeafCountShift) & 0xFu) == 0u) continue;               // an instance: its box is instBoxes'
        const size_t p = (size_t)(std::lower_bound(refs.begin(), refs.end(), ref) - refs.begin()) - numInstances;
        packetBoxes[2u * p] = make_float4(n.minx[c], n.miny[c], n.minz[c], 0.0f);
        packetBoxes[2u * p + 1u] = make_float4(n.maxx[c], n.maxy[c], n.maxz[c], 0.0f);
    }
    std::vector<uint32_t> identity(count);
    std::iota(identity.begin(), identity.end(), 0u);
    HIP_TRY(ctx->topSlots.upload(slots));
    HIP_TRY(ctx->topRefs.upload(refs));
    HIP_TRY(ctx->topPacketBoxes.upload(packetBoxes));
    HIP_TRY(ctx->topIdentity.upload(identity));
    HIP_TRY(ctx->topKeys.alloc(count));
    HIP_TRY(ctx->topOrder.alloc(count));
    HIP_TRY(hipMemset(ctx->topKeys.ptr, 0, (size_t)count * sizeof(uint64_t)));
    HIP_TRY(hipMemset(ctx->topOrder.ptr, 0, (size_t)count * sizeof(uint32_t)));
    if (count > kTopSeatGroup) {
        const size_t bytes = topSeatSortBytes(count);
        if (bytes == 0) return fail(SLRHIP_ERR_HIP, "slrhip_rebuild_top_level: the device radix sort gave no size for its temporary storage");
        HIP_TRY(ctx->topSortedKeys.alloc(count));
        HIP_TRY(ctx->topSortTemp.alloc(bytes));
    }
    ctx->topSlotsHost = std::move(slots);
    ctx->topRefsHost = std::move(refs);
    ctx->topPrimitives = count;
    ctx->topLastPath = ctx->topLastLaunches = 0;
    ctx->topSeatReady = true;
    return SLRHIP_OK;
}

} // namespace

extern "C" {

int slrhip_rebuild_top_level(slrhip_ctx* ctx, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_rebuild_top_level: null context");
    if (const int rc = refusal(ctx, "slrhip_rebuild_top_level")) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->topSeatReady)
        if (const int rc = prepareTopSeat(ctx)) return rc;
    const hipStream_t stream = (hipStream_t)streamPtr;
    TopSeat s{};
    s.nodes = reinterpret_cast<float4*>(ctx->nodes.ptr);
    s.instBoxes = ctx->instBoxes.ptr; s.packetBoxes = ctx->topPacketBoxes.ptr;
    s.refs = ctx->topRefs.ptr; s.slots = ctx->topSlots.ptr;
    s.keys = ctx->topKeys.ptr; s.sortedKeys = ctx->topSortedKeys.ptr; s.identity = ctx->topIdentity.ptr; s.order = ctx->topOrder.ptr;
    s.sortTemp = ctx->topSortTemp.ptr; s.sortTempBytes = ctx->topSortTemp.count;
    s.count = ctx->topPrimitives; s.numInstances = ctx->scene.numInstances; s.topNodes = ctx->topLevelFirst.back();
    InstanceUpdate u{};                                                       // the refit's part of it
    u.numInstances = s.numInstances; u.topNodes = s.topNodes; u.numLevels = (uint32_t)ctx->topLevelFirst.size() - 1u;
    u.instBoxes = ctx->instBoxes.ptr; u.nodes = s.nodes;
    std::copy(ctx->topLevelFirst.begin(), ctx->topLevelFirst.end(), u.levelFirst);
    hipError_t err = hipSuccess;
    const uint32_t seatLaunches = launchTopSeat(s, stream, &err);
    HIP_TRY(err);
    const uint32_t refitLaunches = launchTopRefit(u, stream);
    HIP_TRY(hipGetLastError());
    ctx->topLastPath = s.count <= kTopSeatGroup ? 1u : 2u;
    ctx->topLastLaunches = seatLaunches + refitLaunches;
    return SLRHIP_OK;
}

int slrhip_top_level_cost(slrhip_ctx* ctx, double* hostCost, void* streamPtr) {
    if (!ctx || !hostCost) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_top_level_cost: null argument");
    if (const int rc = refusal(ctx, "slrhip_top_level_cost")) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t stream = (hipStream_t)streamPtr;
    const uint32_t topNodes = ctx->topLevelFirst.back();
    std::vector<QNode> nodes(topNodes);
    HIP_TRY(hipMemcpyAsync(nodes.data(), ctx->nodes.ptr, (size_t)topNodes * sizeof(QNode), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *hostCost = topLevelCost(nodes.data(), topNodes);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the check of slrhip_rebuild_top_level, without a context.
int slrhip_debug_top_level_rebuild_check(int32_t haveScene, uint32_t numInstances) {
    const char* what = nullptr;
    if (const int rc = topLevelRebuildRefusal(haveScene != 0, numInstances, &what)) return fail(rc, std::string("slrhip_rebuild_top_level: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the tables and the last call of slrhip_rebuild_top_level, to host memory.
int slrhip_debug_top_level_rebuild(slrhip_ctx* ctx, uint32_t what, void* hostDst, size_t numWords) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_top_level_rebuild: null argument");
    if (const int rc = refusal(ctx, "slrhip_debug_top_level_rebuild")) return rc;
    const uint32_t n = ctx->topSeatReady ? ctx->topPrimitives : 0u;
    const size_t need = what == 0 ? 8u : what == 3 ? 2u * (size_t)n : (size_t)n;
    if (what > 4) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_top_level_rebuild: unknown `what`");
    if (numWords < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_top_level_rebuild: host_dst too small");
    uint32_t* out = static_cast<uint32_t*>(hostDst);
    if (what == 0) {
        const uint32_t head[8] = {n, kTopSeatGroup, ctx->topLastPath, ctx->topLastLaunches, ctx->scene.numInstances, ctx->topSeatReady ? 1u : 0u, 0u, 0u};
        std::copy(head, head + 8, out);
        return SLRHIP_OK;
    }
    if (n == 0) return SLRHIP_OK;
    if (what == 1) { std::copy(ctx->topSlotsHost.begin(), ctx->topSlotsHost.end(), out); return SLRHIP_OK; }
    if (what == 2) { std::copy(ctx->topRefsHost.begin(), ctx->topRefsHost.end(), out); return SLRHIP_OK; }
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, what == 3 ? (const void*)ctx->topKeys.ptr : (const void*)ctx->topOrder.ptr, need * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // extern "C"
