// slrhip_diagnostics.hip — the entry points of include/slrhip_debug.h, and the two function-level queries with host arrays in and
// out (slrhip_trace_rays, slrhip_bsdf_queries): what the tests and tools call, never a renderer.
#include <memory>

#include "../../include/slrhip_debug.h"
#include "pt_device.h"
#include "pt_shade_variants.h"
#include "slrhip_ctx.h"

using namespace slrhip;

// slrhip_debug_dead_light_samples: deadLightSample — the very function logicSlot decides with — on the caller's triples, one a lane
static __global__ void k_dead_light_samples(uint32_t n, const float* triples, uint32_t* dead) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* t = triples + (size_t)i * 9u;
    dead[i] = deadLightSample(RGB(t[0], t[1], t[2]), RGB(t[3], t[4], t[5]), RGB(t[6], t[7], t[8])) ? 1u : 0u;
}

// The kernels' hit record is (triangle, t, b1, b2) — Moller-Trumbore's barycentrics; the ABI reports Intersection::u, ::v =
// (b0, b1) with b0 = 1 - b1 - b2 exactly as Triangle::intersect computes it (TriangleMesh.cpp:159,172-173).
static void hitsToUV(float* hits, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        float* h = hits + (size_t)i * 4;
        const float b1 = h[2], b2 = h[3];
        const float b0 = 1.0f - b1 - b2;
        uint32_t tri; std::memcpy(&tri, h, 4);
        h[2] = tri == 0xFFFFFFFFu ? 0.0f : b0;
        h[3] = tri == 0xFFFFFFFFu ? 0.0f : b1;
    }
}

extern "C" {

// Diagnostic entry point: closest-hit queries against the uploaded scene (host arrays in and out).
// rays: n x {org[3], dir[3], dist_min, dist_max}; hits: n x {triangle, dist, b0, b1}.
int slrhip_trace_rays(slrhip_ctx* ctx, const float* rays, uint32_t n, float* hits) {
    if (!ctx || !rays || !hits) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_trace_rays: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_trace_rays: no scene uploaded");
    if (n == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<float4> org(n), dir(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float* r = rays + (size_t)i * 8;
        org[i] = make_float4(r[0], r[1], r[2], r[6]);
        dir[i] = make_float4(r[3], r[4], r[5], r[7]);
    }
    DevArray<float4> dOrg, dDir, dOut;
    HIP_TRY(dOrg.upload(org));
    HIP_TRY(dDir.upload(dir));
    HIP_TRY(dOut.alloc(n));
    launchTraceBatch(ctx->scene, dOrg.ptr, dDir.ptr, dOut.ptr, n, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hits, dOut.ptr, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
    hitsToUV(hits, n);
    return SLRHIP_OK;
}

// slrhip_debug.h: the caller's samples as a result window, through the fold of the context's current state.
int slrhip_debug_fold(slrhip_ctx* ctx, const float* hostSamples, uint32_t passes) {
    if (!ctx || !hostSamples) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_fold: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_fold: call slrhip_render_begin first");
    if (passes < 1 || passes > 64) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_fold: 1 .. 64 passes");
    HIP_TRY(hipSetDevice(ctx->device));
    RenderParams rp = ctx->params;
    if (rp.numSlots == 0) { ctx->firstRenderCall = false; return SLRHIP_OK; }       // an empty shard
    if (const int rc = clearStatistics(ctx, nullptr)) return rc;
    if (ctx->firstRenderCall)                                                        // clears the sensor, as a render call of zero passes does
        if (const int rc = renderWindow(ctx, 0, 0, nullptr)) return rc;
    const uint32_t planes = rp.spectral ? 4u : 1u, comps = rp.spectral ? 16u : 3u;
    const size_t elems = (size_t)rp.numPixels * planes;
    std::vector<uint32_t> xy(rp.numPixels);
    HIP_TRY(hipMemcpy(xy.data(), ctx->pixelXY.ptr, xy.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<float4> window((size_t)passes * elems);
    for (uint32_t p = 0; p < passes; ++p)
        for (uint32_t i = 0; i < rp.numPixels; ++i) {
            const float* src = hostSamples + (((size_t)p * rp.imageHeight + (xy[i] >> 16)) * rp.imageWidth + (xy[i] & 0xFFFFu)) * comps;
            float4* dst = window.data() + windowEntry(i, p, passes) * planes;
            if (rp.spectral) for (uint32_t q = 0; q < 4; ++q) dst[q] = make_float4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
            else dst[0] = make_float4(src[0], src[1], src[2], 0.0f);
        }
    HIP_TRY(ctx->results.alloc(window.size()));
    ctx->buffers.results = ctx->results.ptr;
    HIP_TRY(hipMemcpy(ctx->results.ptr, window.data(), window.size() * sizeof(float4), hipMemcpyHostToDevice));
    rp.sppBegin = 0; rp.sppCount = passes;
    launchFold(ctx->buffers, rp, ctx->stats.on ? ctx->stats.records.ptr : nullptr, clampParams(ctx), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_modulate alone.
int slrhip_debug_modulate_check(const slrhip_modulate_desc* d) {
    if (!d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_modulate: null argument");
    if (const char* what = modulateRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_modulate: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_reproject alone.
int slrhip_debug_reproject_check(const slrhip_reproject_desc* d) {
    if (!d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_reproject: null argument");
    if (const char* what = reprojectRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_reproject: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_render_motion alone, for a context described by two numbers.
int slrhip_debug_motion_check(int32_t haveRender, uint32_t numInstances, const slrhip_motion_desc* d, uint32_t sppBegin, uint32_t sppCount) {
    const char* what = nullptr;
    if (const int rc = motionRefusal(haveRender != 0, numInstances, d, sppBegin, sppCount, &what))
        return fail(rc, std::string("slrhip_render_motion: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_render_motion_vertices alone, for a context described by four numbers.
int slrhip_debug_motion_vertices_check(int32_t haveRender, uint32_t numInstances, uint32_t configFlags, uint32_t treeBuilder,
                                       const slrhip_motion_vertices_desc* d, uint32_t sppBegin, uint32_t sppCount) {
    const char* what = nullptr;
    if (const int rc = motionVerticesRefusal(haveRender != 0, numInstances, configFlags, treeBuilder, d, sppBegin, sppCount, &what))
        return fail(rc, std::string("slrhip_render_motion_vertices: ") + what);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the block lengths of a slrhip_render_adaptive call.
int slrhip_debug_adaptive_blocks(uint32_t sppMin, uint32_t sppStep, uint32_t sppMax, uint32_t* blocks, uint32_t maxBlocks, uint32_t* numBlocks) {
    if (!numBlocks || (maxBlocks && !blocks)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_adaptive_blocks: null argument");
    const std::vector<uint32_t> plan = planAdaptiveBlocks(sppMin, sppStep, sppMax);
    *numBlocks = (uint32_t)plan.size();
    for (uint32_t k = 0; k < std::min<uint32_t>(*numBlocks, maxBlocks); ++k) blocks[k] = plan[k];
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): function-level BSDF queries through the device functions the shade kernel calls.
int slrhip_debug_work_distribution(uint32_t numPixels, uint32_t numSlots, uint32_t numPasses, uint32_t runLength, uint32_t* counts,
                                   uint32_t* queueLengths) {
    if (!counts || !queueLengths || numPixels == 0 || numSlots < 64 || numSlots % 64 || runLength == 0 || numPasses % runLength ||
        (uint64_t)numPixels * numPasses > 0xFFFFFFFFull)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_work_distribution: bad arguments");
    RenderParams rp;
    std::memset(&rp, 0, sizeof(rp));
    rp.numSlots = numSlots; rp.numWaves = numSlots / 64u; rp.numPixels = numPixels; rp.sppCount = numPasses;
    rp.workItems = numPixels * numPasses; rp.runLength = runLength; rp.numRuns = numPixels * (numPasses / runLength);
    for (uint32_t w = 0; w < rp.numWaves; ++w) {
        uint32_t taken = 0;
        for (;; ++taken) {
            const WorkItem it = workItemOf(rp, w, taken);
            if (!it.valid) break;
            ++counts[(size_t)it.pass * numPixels + it.pix];
        }
        queueLengths[w] = taken;
        if (workSamplesTaken(rp, w, taken + 7u) != taken) return fail(SLRHIP_ERR_HIP, "slrhip_debug_work_distribution: workSamplesTaken disagrees with the queue");
    }
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the render plan of render_plan.cpp for a frame, a shard and a call of num_passes passes.
int slrhip_debug_render_plan(int32_t width, int32_t height, uint32_t shardIndex, uint32_t shardCount, uint32_t stripes, int32_t mode,
                             uint32_t numPasses, uint64_t budgetBytes, uint32_t* plan, uint32_t* windows, uint32_t maxWindows,
                             uint32_t* numWindows, uint32_t* pixels, uint32_t maxPixels) {
    if (!plan || !numWindows || (maxWindows && !windows) || budgetBytes == 0 || stripes > SLRHIP_MAX_STRIPES ||
        (mode != SLRHIP_MODE_RGB && mode != SLRHIP_MODE_SPECTRAL))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_render_plan: bad arguments");
    const bool spectral = mode == SLRHIP_MODE_SPECTRAL;
    FramePlan frame;
    std::string err;
    if (const int rc = planFrame(width, height, shardIndex, shardCount, stripes, spectral, autoStripesOverride(), pairsMask(), &frame, &err))
        return fail(rc, err);
    const uint32_t window = frame.numPixels ? planWindows(frame.numPixels, spectral, numPasses, budgetBytes) : 0u;
    plan[0] = frame.numPixels; plan[1] = frame.stripes; plan[2] = frame.numSlots; plan[3] = window;
    *numWindows = window ? (numPasses + window - 1) / window : 0u;
    for (uint32_t k = 0; k < std::min(*numWindows, maxWindows); ++k) {
        windows[2 * k] = std::min(window, numPasses - k * window);
        windows[2 * k + 1] = planWindow(frame.numPixels, windows[2 * k], runLengthOverride()).runLength;
    }
    if (pixels) {
        if (maxPixels < frame.numPixels) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_render_plan: pixel buffer too small");
        if (frame.numPixels) { const std::vector<uint32_t> list = shardPixels(frame); std::memcpy(pixels, list.data(), list.size() * sizeof(uint32_t)); }
    }
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the primary pass of a window as renderWindow plans it.
int slrhip_debug_primary_plan(uint32_t numPixels, uint32_t numPasses, uint32_t configFlags, int32_t sceneClass, uint32_t* plan) {
    if (!plan) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_plan: null argument");
    const PrimaryPlan p = planPrimary(numPixels, numPasses, configFlags, (sceneClass & 1) != 0, (sceneClass & 2) != 0, (sceneClass & 4) != 0);
    plan[0] = p.on ? 1u : 0u; plan[1] = p.passesPerLaunch; plan[2] = p.numLaunches; plan[3] = p.instanceEntries ? 1u : 0u;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): where the primary pass's launches put their samples, with the helper the kernels call.
int slrhip_debug_primary_entries(uint32_t numPixels, uint32_t firstPass, uint32_t numPasses, uint32_t windowPasses, uint64_t* entries) {
    if (!entries) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_entries: null argument");
    if (numPasses == 0 || (uint64_t)firstPass + numPasses > windowPasses || (uint64_t)numPixels * numPasses > kPrimaryMaxSamples)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_entries: the launch's passes must be 1 or more, inside the window, and under 2^31 samples");
    const size_t first = windowEntry(0u, firstPass, windowPasses);       // launchPrimary's own arithmetic
    for (uint32_t i = 0; i < numPixels * numPasses; ++i) entries[i] = first + primaryLaunchEntry(i, numPasses, windowPasses);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the stream plane of a window as renderWindow plans it.
int slrhip_debug_primary_stream_plan(uint32_t numPixels, uint32_t numPasses, uint32_t configFlags, int32_t sceneClass, uint64_t* entries) {
    if (!entries) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_stream_plan: null argument");
    *entries = planPrimary(numPixels, numPasses, configFlags, (sceneClass & 1) != 0, (sceneClass & 2) != 0, (sceneClass & 4) != 0, (sceneClass & 8) != 0).rngEntries;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the entries of the stream plane the last window bound.
int slrhip_debug_primary_stream_entries(slrhip_ctx* ctx, uint64_t* entries) {
    if (!ctx || !entries) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_stream_entries: null argument");
    *entries = ctx->primaryRngEntries;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the kernel of a window's primary pass as renderWindow plans it.
int slrhip_debug_primary_kernel_plan(uint32_t numPixels, uint32_t numPasses, uint32_t configFlags, int32_t sceneClass, uint32_t* direct) {
    if (!direct) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_kernel_plan: null argument");
    *direct = planPrimary(numPixels, numPasses, configFlags, (sceneClass & 1) != 0, (sceneClass & 2) != 0, (sceneClass & 4) != 0, (sceneClass & 8) != 0).kernel ==
                      PrimaryKernel::Direct
                  ? 1u
                  : 0u;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the kernel the last window's primary pass was launched with.
int slrhip_debug_primary_kernel(slrhip_ctx* ctx, uint32_t* kernel) {
    if (!ctx || !kernel) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_kernel: null argument");
    *kernel = (uint32_t)ctx->primaryKernel;
    return SLRHIP_OK;
}

static void variantWords(const ShadeVariant& v, uint32_t* out) {
    const bool f[7] = {v.spectral, v.ldsTables, v.glossy, v.multi, v.textures, v.primary, v.resume};
    for (int i = 0; i < 7; ++i) out[i] = f[i] ? 1u : 0u;
}

// Diagnostic (include/slrhip_debug.h): the k_shade instantiation of a window as renderWindow plans it, and its rows in the table.
int slrhip_debug_shade_plan(uint32_t spectral, uint32_t shadeTables, uint32_t hasMicrofacet, uint32_t hasMulti, uint32_t numTextures, uint32_t primary,
                            uint32_t primaryRng, uint32_t* plan) {
    if (!plan) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_shade_plan: null argument");
    const ShadeVariant v = planShadeVariant(spectral != 0, shadeTables != 0, hasMicrofacet != 0, hasMulti != 0, numTextures, primary != 0, primaryRng != 0);
    variantWords(v, plan);
    plan[7] = findShadeKernel(v) ? 1u : 0u;
    plan[8] = findTailKernel(tailVariant(v)) ? 1u : 0u;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): what the last window's launchShade and launchTail launched.
int slrhip_debug_shade_kernel(slrhip_ctx* ctx, uint32_t* kernel) {
    if (!ctx || !kernel) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_shade_kernel: null argument");
    variantWords(ctx->shadeVariant, kernel);
    kernel[7] = ctx->shadeLaunched ? 1u : 0u;
    kernel[8] = ctx->tailLaunched ? 1u : 0u;
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): one launch of the primary pass, either kernel, into the caller's planes.
int slrhip_debug_primary_pass(slrhip_ctx* ctx, uint32_t kernel, uint32_t firstPass, uint32_t numPasses, uint32_t windowPasses, void* records,
                              void* streams) {
    if (!ctx || !records) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_pass: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_primary_pass: call slrhip_render_begin first");
    if (kernel > 1u) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_pass: kernel is 0 (ring) or 1 (direct)");
    RenderParams rp = ctx->params;
    PathBuffers pb = ctx->buffers;
    if (numPasses == 0 || (uint64_t)firstPass + numPasses > windowPasses || (uint64_t)rp.numPixels * numPasses > kPrimaryMaxSamples ||
        (uint64_t)rp.numPixels * windowPasses > 0xFFFFFFFFull)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_pass: the launch's passes must be 1 or more, inside the window, and under 2^31 samples");
    if (kernel == 1u && (ctx->scene.instances || ctx->scene.nodesQ))
        return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_debug_primary_pass: the direct kernel traces scenes without instances on the float nodes only");
    if (rp.numSlots == 0) return SLRHIP_OK;       // an empty shard
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    rp.sppBegin = 0; rp.sppCount = windowPasses;
    pb.results = static_cast<float4*>(records);
    pb.primaryRng = static_cast<uint4*>(streams);
    pb.primaryInstance = nullptr;
    if (ctx->scene.instances) {                   // the ring kernel's instance plane: the context's own, as a window of this size binds it
        HIP_TRY(ctx->primaryInstance.alloc((size_t)rp.numPixels * windowPasses));
        pb.primaryInstance = ctx->primaryInstance.ptr;
    }
    HIP_TRY(hipMemset(pb.errorWord, 0, sizeof(uint32_t)));
    launchPrimary(ctx->scene, pb, rp, firstPass, numPasses, kernel ? PrimaryKernel::Direct : PrimaryKernel::Ring, ctx->numCUs, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    uint32_t bits = 0;
    HIP_TRY(hipMemcpy(&bits, pb.errorWord, sizeof(bits), hipMemcpyDeviceToHost));
    if (bits) return fail(SLRHIP_ERR_HIP, "slrhip_debug_primary_pass: device-side error word set: " + std::to_string(bits));
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the camera draws forward and recovered, on the device.
int slrhip_debug_camera_draws(int32_t device, uint32_t n, const uint32_t* tuples, uint32_t* out) {
    if (!tuples || !out) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_camera_draws: null argument");
    if (n == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(device));
    DevArray<uint4> dIn;
    DevArray<uint32_t> dOut;
    HIP_TRY(dIn.alloc(n));
    HIP_TRY(dOut.alloc((size_t)n * 16u));
    HIP_TRY(hipMemcpy(dIn.ptr, tuples, (size_t)n * sizeof(uint4), hipMemcpyHostToDevice));
    launchCameraDraws(n, dIn.ptr, dOut.ptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dOut.ptr, (size_t)n * 16u * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the device's dead-sample predicate on the caller's (sum, compensation, contribution) triples.
int slrhip_debug_dead_light_samples(int32_t device, uint32_t n, const float* triples, uint32_t* dead) {
    if (!triples || !dead) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_dead_light_samples: null argument");
    if (n == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(device));
    DevArray<float> dIn;
    DevArray<uint32_t> dOut;
    HIP_TRY(dIn.alloc((size_t)n * 9u));
    HIP_TRY(dOut.alloc(n));
    HIP_TRY(hipMemcpy(dIn.ptr, triples, (size_t)n * 9u * sizeof(float), hipMemcpyHostToDevice));
    k_dead_light_samples<<<(n + 255u) / 256u, 256, 0, nullptr>>>(n, dIn.ptr, dOut.ptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(dead, dOut.ptr, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // extern "C"

// ---- the tree read-outs (include/slrhip_debug.h): one description of the arrays for the context's tree and the host-built one ----
namespace {
const uint32_t kTreeSummaryWords = 16, kTreeArrays = 7;
struct TreeView {
    uint32_t summary[kTreeSummaryWords];
    const void* src[kTreeArrays];        // per `what` (0 unused); null = the array does not exist for this tree
    size_t words[kTreeArrays];
};
void describeTree(TreeView& v, uint32_t builder, uint32_t numNodes, uint32_t depth, uint64_t leafRefs, uint32_t numTris, bool quantized,
                  uint32_t numInstances, uint32_t topNodes) {
    std::memset(&v, 0, sizeof(v));
    const uint32_t s[8] = {builder, numNodes, depth, (uint32_t)leafRefs, numTris, quantized ? 1u : 0u, numInstances, topNodes};
    std::copy(s, s + 8, v.summary);
    const size_t words[kTreeArrays] = {kTreeSummaryWords, (size_t)numNodes * (sizeof(QNode) / 4), quantized ? (size_t)numNodes * (sizeof(QNodeQ) / 4) : 0,
                                       (size_t)leafRefs * (sizeof(LeafTri) / 4), (size_t)numTris * (sizeof(ShadeTri) / 4),
                                       (size_t)numInstances * (sizeof(DevInstance) / 4), (size_t)numInstances * 8u};
    std::copy(words, words + kTreeArrays, v.words);
}
// the argument checks both read-outs share; *copyBytes = what to copy from v.src[what] (0: the summary was written, nothing to copy)
int treeReadOut(const char* who, const TreeView& v, uint32_t what, void* hostDst, size_t numWords, size_t* copyBytes) {
    *copyBytes = 0;
    if (what >= kTreeArrays) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string(who) + ": unknown `what`");
    if (what == 2 && !v.summary[5]) return fail(SLRHIP_ERR_UNSUPPORTED, std::string(who) + ": the quantized nodes are not in use");
    if (numWords < v.words[what]) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string(who) + ": host_dst too small");
    if (what == 0) std::memcpy(hostDst, v.summary, sizeof(v.summary));
    else *copyBytes = v.words[what] * 4u;
    return SLRHIP_OK;
}
// the scene slrhip_debug_host_tree prepared last on this thread (what = 0), for its other read-outs
thread_local std::unique_ptr<PreparedScene> t_hostTree;
} // namespace

extern "C" {

// Diagnostic (include/slrhip_debug.h): the tree of the context's scene, whichever builder made it, to host memory.
int slrhip_debug_tree(slrhip_ctx* ctx, uint32_t what, void* hostDst, size_t numWords) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_tree: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_tree: no scene uploaded");
    const DevScene& sc = ctx->scene;
    TreeView v;
    describeTree(v, ctx->treeBuilder, sc.numNodes, ctx->bvhDepth, ctx->bvhLeafRefs, (uint32_t)ctx->shadeTris.count, sc.nodesQ != nullptr,
                 sc.numInstances, sc.numInstances && !ctx->topLevelFirst.empty() ? ctx->topLevelFirst.back() : 0u);
    v.src[1] = ctx->nodes.ptr; v.src[2] = ctx->nodesQ.ptr; v.src[3] = ctx->leafTris.ptr; v.src[4] = ctx->shadeTris.ptr;
    v.src[5] = ctx->instances.ptr; v.src[6] = ctx->instBoxes.ptr;
    size_t bytes = 0;
    if (const int rc = treeReadOut("slrhip_debug_tree", v, what, hostDst, numWords, &bytes)) return rc;
    if (!bytes) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, v.src[what], bytes, hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the tree prepareScene builds on the host for a descriptor, without a context or a GPU.
int slrhip_debug_host_tree(const slrhip_scene_desc* desc, uint32_t configFlags, uint32_t what, void* hostDst, size_t numWords) {
    if (!hostDst || (what == 0 && !desc)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_host_tree: null argument");
    if (what == 0) {
        t_hostTree.reset();
        std::unique_ptr<PreparedScene> p(new PreparedScene());
        slrhip_config config;
        std::memset(&config, 0, sizeof(config));
        config.mode = SLRHIP_MODE_RGB; config.flags = configFlags;
        std::string err;
        if (const int rc = prepareScene(*desc, config, p.get(), &err)) return fail(rc, err);
        if (p->build == TreeBuild::Device)
            return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_debug_host_tree: slrhip_upload_scene leaves this scene's tree to the device build (bvh_device.hip); "
                                                "the host builds none for it");
        t_hostTree = std::move(p);
    }
    if (!t_hostTree) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_host_tree: no tree prepared on this thread (call with what = 0 first)");
    const PreparedScene& p = *t_hostTree;
    std::vector<float> boxes;
    for (const Box& b : p.bvh.instBoxes) boxes.insert(boxes.end(), {b.lo[0], b.lo[1], b.lo[2], 0.0f, b.hi[0], b.hi[1], b.hi[2], 0.0f});
    TreeView v;
    describeTree(v, treeBuilderOf(p), (uint32_t)p.bvh.nodes.size(), p.bvh.depth, p.bvh.leafTris.size(), (uint32_t)p.shadeTris.size(), p.quantized,
                 (uint32_t)p.instances.size(), p.instances.empty() ? 0u : p.bvh.topNodes);
    v.src[1] = p.bvh.nodes.data(); v.src[2] = p.bvh.quantized.data(); v.src[3] = p.bvh.leafTris.data(); v.src[4] = p.shadeTris.data();
    v.src[5] = p.instances.data(); v.src[6] = boxes.data();
    size_t bytes = 0;
    if (const int rc = treeReadOut("slrhip_debug_host_tree", v, what, hostDst, numWords, &bytes)) return rc;
    if (bytes) std::memcpy(hostDst, v.src[what], bytes);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): quantizeNodes of bvh.cpp on the caller's nodes.
int slrhip_debug_quantize_nodes(const void* nodes, uint32_t n, void* nodesQ) {
    if ((n && !nodes) || (n && !nodesQ)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_quantize_nodes: null argument");
    QBVH tree;
    tree.nodes.resize(n);
    if (n) std::memcpy(tree.nodes.data(), nodes, (size_t)n * sizeof(QNode));
    quantizeNodes(&tree);
    if (n) std::memcpy(nodesQ, tree.quantized.data(), (size_t)n * sizeof(QNodeQ));
    return SLRHIP_OK;
}

int slrhip_bsdf_queries(slrhip_ctx* ctx, uint32_t material, uint32_t n, const float* queries, float wl_offset, float u_lambda, float* out) {
    if (!ctx || !queries || !out) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_bsdf_queries: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_bsdf_queries: no scene uploaded");
    if (material >= ctx->scene.numMaterials) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_bsdf_queries: material index out of range");
    if (!(wl_offset >= 0.0f && wl_offset < 1.0f) || !(u_lambda >= 0.0f && u_lambda < 1.0f))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_bsdf_queries: wl_offset and u_lambda must be in [0, 1)");
    if (n == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const bool spectral = ctx->config.mode == SLRHIP_MODE_SPECTRAL;
    const uint32_t C = spectral ? 16u : 3u, planes = spectral ? 4u : 1u;
    // WavelengthSamples::createWithEqualOffsets (SpectrumTypes.h:60, RGBTypes.h:41)
    const uint32_t wl = std::min<uint32_t>((uint16_t)(C * u_lambda), C - 1);
    std::vector<float> in(queries, queries + (size_t)n * 12);
    DevArray<float> dIn;
    DevArray<float4> dGeo, dMisc, dFsS, dFsE;
    HIP_TRY(dIn.upload(in));
    HIP_TRY(dGeo.alloc(n));
    HIP_TRY(dMisc.alloc(n));
    HIP_TRY(dFsS.alloc((size_t)planes * n));
    HIP_TRY(dFsE.alloc((size_t)planes * n));
    launchBsdfQueries(ctx->scene, spectral, material, n, dIn.ptr, wl_offset, wl, dGeo.ptr, dMisc.ptr, dFsS.ptr, dFsE.ptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    std::vector<float4> geo(n), misc(n), fsS((size_t)planes * n), fsE((size_t)planes * n);
    HIP_TRY(hipMemcpy(geo.data(), dGeo.ptr, geo.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(misc.data(), dMisc.ptr, misc.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fsS.data(), dFsS.ptr, fsS.size() * sizeof(float4), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fsE.data(), dFsE.ptr, fsE.size() * sizeof(float4), hipMemcpyDeviceToHost));
    const uint32_t stride = 6 + 2 * C;
    for (uint32_t i = 0; i < n; ++i) {
        float* o = out + (size_t)stride * i;
        o[0] = geo[i].x; o[1] = geo[i].y; o[2] = geo[i].z; o[3] = geo[i].w; o[4] = misc[i].x;
        for (uint32_t k = 0; k < C; ++k) {
            const float* a = reinterpret_cast<const float*>(&fsS[(size_t)(k / 4) * n + i]);
            const float* b = reinterpret_cast<const float*>(&fsE[(size_t)(k / 4) * n + i]);
            o[5 + k] = a[k % 4];
            o[5 + C + k] = b[k % 4];
        }
        o[5 + 2 * C] = misc[i].y;
    }
    return SLRHIP_OK;
}

} // extern "C"
