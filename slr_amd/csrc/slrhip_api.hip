// slrhip_api.hip — the C ABI of include/slrhip.h over the HIP kernels: the context, the scene, the render loop and the framebuffer
// (the feature areas on top of them: slrhip_buffers.hip, slrhip_image.hip, slrhip_diagnostics.hip; what they share: slrhip_ctx.h).
// A scene is checked and flattened on the host by scene_prep.cpp, then committed here: the device tree build (if chosen),
// the uploads, the DevScene.  PathTracingRenderer::render's set-up (Renderers/PathTracingRenderer.cpp:27-70) is planned on the
// host by render_plan.cpp (pixel list, slot count, result windows, run lengths); render_begin allocates and binds the path state
// from that plan in one commit, and renderWindow drives the wavefront iterations of a window through one launch loop.
// There is no CPU fallback: without a HIP device every entry point fails loudly.
#include <dlfcn.h>

#include <chrono>

#include "pt_refit.h"
#include "pt_shade_variants.h"
#include "slrhip_ctx.h"

using namespace slrhip;

std::atomic<size_t> slrhip::g_skewCounter{0};
static_assert(kClampDropNonFinite == SLRHIP_CLAMP_DROP_NONFINITE, "pt_clamp.h's flag is the ABI's");

const int kDefaultPairs = 1;                   // SLRHIP_PAIRS: the ray pair pays, the radiance-sum pair does not
#ifndef SLR_TAIL_DIVISOR
#define SLR_TAIL_DIVISOR 8u      // the tail kernel never takes more than this fraction of the slots (1u in a variant build: the tail kernel as the whole renderer, measured in DESIGN.md)
#endif

static thread_local std::string g_lastError;

int slrhip::fail(int code, const std::string& msg) {
    g_lastError = msg;
    return code;
}

namespace {

// Device-side error word (PathBuffers::errorWord): every bounded spin that gives up and every dropped stack push sets a bit, so a
// logic error in a kernel fails the render instead of returning a wrong image with status 0.
int deviceError(uint32_t bits) {
    std::string what = "slrhip_render: device-side error word set:";
    if (bits & ERR_RING_SPACE) what += " [producer gave up waiting for ray-ring space]";
    if (bits & ERR_RING_RELEASE) what += " [consumer gave up waiting for the ring's release watermark]";
    if (bits & ERR_CONSUMER_IDLE) what += " [consumer wave gave up waiting for rays]";
    if (bits & ERR_STACK_OVERFLOW) what += " [traversal stack overflow: a push was dropped]";
    if (bits & ERR_QUEUE_OVERFLOW) what += " [queue region overflow]";
    return fail(SLRHIP_ERR_HIP, what);
}

} // namespace

// Sum the sharded statistics words (pt_kernels.h: totalIndex).
static int readTotals(slrhip_ctx* ctx, uint64_t* out) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<uint64_t> raw(ctx->totals.count);
    HIP_TRY(hipMemcpy(raw.data(), ctx->totals.ptr, raw.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < T_KINDS; ++k) {
        out[k] = 0;
        for (uint32_t sh = 0; sh < kShards; ++sh) out[k] += raw[totalIndex(k, sh)];
    }
    if (tuningEnv("SLRHIP_DEBUG_WS") && out[T_WS_STEPS])
        fprintf(stderr, "ws closest: rays %llu nodes %llu tris %llu | consumer wave-steps %llu refills %llu idle spins %llu | "
                        "consumer wave cycles %llu x64, idle %llu x64 | producer waits %llu | node blocks %llu tri blocks %llu active lanes %llu | shadow rays %llu nodes %llu tris %llu\n",
                (unsigned long long)out[T_EXT_RAYS], (unsigned long long)out[T_NODES_CLOSEST], (unsigned long long)out[T_TRIS_CLOSEST],
                (unsigned long long)out[T_WS_STEPS], (unsigned long long)out[T_WS_REFILLS], (unsigned long long)out[T_WS_IDLE_SPINS],
                (unsigned long long)out[T_WS_CYCLES], (unsigned long long)out[T_WS_IDLE_CYCLES], (unsigned long long)out[T_WS_PRODUCER_WAITS],
                (unsigned long long)out[T_WS_NODE_BLOCKS], (unsigned long long)out[T_WS_TRI_BLOCKS], (unsigned long long)out[T_WS_ACTIVE_LANES],
                (unsigned long long)out[T_SHADOW_RAYS], (unsigned long long)out[T_NODES_SHADOW], (unsigned long long)out[T_TRIS_SHADOW]);
    return SLRHIP_OK;
}

// Points a zero-initialised DevScene at the context's scene arrays and assigns it to ctx->scene in one go.
static void bindScene(slrhip_ctx* ctx, const slrhip_scene_desc& d, const PreparedScene& p, uint32_t numNodes, bool quantized) {
    DevScene sc{};
    sc.nodes = reinterpret_cast<const float4*>(ctx->nodes.ptr); sc.numNodes = numNodes;
    sc.nodesQ = quantized ? reinterpret_cast<const float4*>(ctx->nodesQ.ptr) : nullptr;
    sc.leafTris = reinterpret_cast<const float4*>(ctx->leafTris.ptr);
    sc.shadeTris = ctx->shadeTris.ptr;
    sc.instances = p.instances.empty() ? nullptr : reinterpret_cast<const float4*>(ctx->instances.ptr); sc.numInstances = (uint32_t)p.instances.size();
    sc.lightTris = ctx->lightTris.ptr; sc.numLights = (uint32_t)p.lightTris.size(); sc.lightPow2 = prevPowerOf2(sc.numLights);
    sc.lightPMF = ctx->lightPMF.ptr; sc.lightCDF = ctx->lightCDF.ptr; sc.aggImportance = p.lightIntegral;
    sc.materials = ctx->materials.ptr; sc.materialsS = ctx->materialsS.ptr; sc.numMaterials = (uint32_t)p.materials.size();
    sc.hasMicrofacet = p.hasMicrofacet; sc.hasMulti = p.hasMulti;
    sc.spectra = ctx->spectra.ptr; sc.numSpectra = (uint32_t)p.spectra.size();
    sc.spectrumPool = ctx->spectrumPool.ptr; sc.numSpectrumData = (uint32_t)p.spectrumPool.size();
    sc.textures = ctx->textures.ptr; sc.numTextures = (uint32_t)p.textures.size(); sc.matTex = ctx->matTex.ptr;
    sc.triUV = ctx->triUV.ptr; sc.alphaTris = ctx->alphaTris.ptr; sc.texTexels = ctx->texTexels.ptr;
    sc.shadeTables = p.tablesFit ? ctx->shadeTables.ptr : nullptr;
    std::memcpy(sc.tableEnd, p.tableEnd, sizeof(sc.tableEnd));
    if (d.env) {
        sc.hasEnv = 1; sc.envScale = d.env->scale;
        sc.envWidth = d.env->width; sc.envHeight = d.env->height; sc.envMapWidth = d.env->map_width; sc.envMapHeight = d.env->map_height;
    }
    sc.envTexels = ctx->envTexels.ptr;
    sc.envTopPDF = ctx->envTopPDF.ptr; sc.envTopCDF = ctx->envTopCDF.ptr; sc.envRowPDF = ctx->envRowPDF.ptr; sc.envRowCDF = ctx->envRowCDF.ptr;
    sc.gridWidth = p.gridWidth; sc.gridHeight = p.gridHeight;
    sc.gridCells = ctx->gridCells.ptr; sc.pointUV = ctx->pointUV.ptr; sc.pointSpectrum = ctx->pointSpectrum.ptr;
    sc.camera = p.camera;
    ctx->scene = sc;
}

// The device half of slrhip_upload_scene: the device tree build (when prepareScene chose it), the uploads, the DevScene.  An upload
// may free an array of the previous scene before it fails, so the context holds no scene from the first statement on until the
// last step has succeeded: a failure here leaves it without one (SLRHIP_ERR_NO_SCENE), never naming freed or mismatched arrays.
static int commitScene(slrhip_ctx* ctx, const slrhip_scene_desc& d, const PreparedScene& p) {
    ctx->haveScene = ctx->haveRender = false;
    ctx->topSeatReady = false;                    // slrhip_rebuild_top_level's tables are the previous scene's: its next call builds them again
    ctx->topPrimitives = ctx->topLastPath = ctx->topLastLaunches = 0;
    HIP_TRY(hipSetDevice(ctx->device));
    uint32_t numNodes = (uint32_t)p.bvh.nodes.size(), depth = p.bvh.depth;
    uint64_t leafRefs = p.bvh.leafTris.size();
    bool quantized = p.quantized;
    const std::vector<uint32_t>* levelFirst = &p.bvh.levelFirst;
    DeviceGeometry g;
    if (p.build == TreeBuild::Device) {
        // the whole geometry on the GPU: tree, quantized nodes, leaf packets, shading records (bvh_device.hip)
        std::string err;
        if (buildGeometryDevice(d.vertices, d.num_vertices, d.triangles, d.num_triangles, p.lightTriangles.data(), (uint32_t)p.lightTriangles.size(),
                                p.wantQuantized, &g, &err) != 0)
            return fail(SLRHIP_ERR_HIP, "slrhip_upload_scene: " + err);
        if (const int rc = checkTreeLimits(g.depth, g.numNodes, g.numLeafTris,
                                           "device-built tree deeper than the 64-entry traversal stack (QBVH.h:299); use the host build", &err)) {
            for (void* a : {(void*)g.nodes, (void*)g.nodesQ, (void*)g.leafTris, (void*)g.shadeTris}) (void)hipFree(a);
            return fail(rc, err);
        }
        ctx->nodes.adopt(g.nodes, g.numNodes);
        ctx->leafTris.adopt(g.leafTris, g.numLeafTris);
        ctx->shadeTris.adopt(g.shadeTris, d.num_triangles);
        quantized = g.nodesQ != nullptr && useQuantizedNodes(g.numNodes);
        if (quantized) ctx->nodesQ.adopt(g.nodesQ, g.numNodes); else (void)hipFree(g.nodesQ);
        numNodes = g.numNodes; depth = g.depth; leafRefs = g.numLeafTris;
        levelFirst = &g.levelFirst;
    }
    else {
        HIP_TRY(ctx->nodes.upload(p.bvh.nodes));
        if (p.quantized) HIP_TRY(ctx->nodesQ.upload(p.bvh.quantized));
        HIP_TRY(ctx->leafTris.upload(p.bvh.leafTris));
    }
    HIP_TRY(ctx->textures.upload(p.textures));
    HIP_TRY(ctx->texTexels.upload(p.texTexels));
    HIP_TRY(ctx->matTex.upload(p.matTex));
    HIP_TRY(ctx->triUV.upload(p.triUV));
    HIP_TRY(ctx->alphaTris.upload(p.alphaTris));
    if (p.build != TreeBuild::Device) HIP_TRY(ctx->shadeTris.upload(p.shadeTris));
    HIP_TRY(ctx->lightTris.upload(p.lightTris));
    HIP_TRY(ctx->instances.upload(p.instances));
    if (!p.instances.empty()) {
        // what slrhip_set_instance_transforms works from: allocated here, so that the call allocates nothing
        const auto boxes = [](const std::vector<Box>& v) {
            std::vector<float4> out;
            for (const Box& b : v) { out.push_back(make_float4(b.lo[0], b.lo[1], b.lo[2], 0.0f)); out.push_back(make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f)); }
            return out;
        };
        HIP_TRY(ctx->meshBoxes.upload(boxes(p.bvh.meshBoxes)));
        HIP_TRY(ctx->instBoxes.upload(boxes(p.bvh.instBoxes)));
        HIP_TRY(ctx->instanceStatus.alloc(1));
        HIP_TRY(hipMemset(ctx->instanceStatus.ptr, 0, sizeof(uint32_t)));
        ctx->topLevelFirst = p.bvh.levelFirst;
        ctx->topLevelFirst.push_back(p.bvh.topNodes);
    }
    HIP_TRY(ctx->materials.upload(p.materials));
    HIP_TRY(ctx->materialsS.upload(p.materialsS));
    HIP_TRY(ctx->spectrumPool.upload(p.spectrumPool));
    HIP_TRY(ctx->spectra.upload(p.spectra));
    HIP_TRY(ctx->lightPMF.upload(p.lightPMF));
    HIP_TRY(ctx->lightCDF.upload(p.lightCDF));
    HIP_TRY(ctx->shadeTables.upload(p.shadeTables));
    HIP_TRY(ctx->envTexels.upload(p.envTexels));
    HIP_TRY(ctx->envTopPDF.upload(p.envTopPDF)); HIP_TRY(ctx->envTopCDF.upload(p.envTopCDF));
    HIP_TRY(ctx->envRowPDF.upload(p.envRowPDF)); HIP_TRY(ctx->envRowCDF.upload(p.envRowCDF));
    HIP_TRY(ctx->gridCells.upload(p.gridCells)); HIP_TRY(ctx->pointUV.upload(p.pointUV)); HIP_TRY(ctx->pointSpectrum.upload(p.pointSpectrum));
    // what slrhip_set_vertices works from (SLRHIP_FLAG_DYNAMIC_GEOMETRY; flat scenes whose leaves hold whole triangles): allocated
    // here, so that the call allocates nothing.  Without the flag, nothing.
    // A scene with instances is kept only with SLRHIP_FLAG_DYNAMIC_INSTANCED as well: then also the mesh trees' merged level list
    // and the meshes' roots, and the level table is the top level's.
    ctx->geometryKept = ctx->geoInstanced = false;
    const bool dynamic = (ctx->config.flags & SLRHIP_FLAG_DYNAMIC_GEOMETRY) != 0;
    const bool keepInstanced = dynamic && (ctx->config.flags & SLRHIP_FLAG_DYNAMIC_INSTANCED) && p.build == TreeBuild::Instanced;
    if (keepInstanced) {
        const QBVH& t = p.bvh;
        if (t.meshLevelFirst.size() < 2 || t.meshLevelFirst.size() - 1u > kMaxTreeLevels || t.meshLevelFirst.back() != t.meshLevelNodes.size() ||
            (size_t)t.topNodes + t.meshLevelNodes.size() != numNodes || t.meshRoots.size() != t.meshBoxes.size() || levelFirst->empty() ||
            levelFirst->size() > kMaxTreeLevels)
            return fail(SLRHIP_ERR_HIP, "slrhip_upload_scene: the mesh trees have no level list (internal error)");
        HIP_TRY(ctx->geoMeshLevelNodes.upload(t.meshLevelNodes));
        HIP_TRY(ctx->geoMeshRoots.upload(t.meshRoots));
        ctx->geoMeshLevelFirst = t.meshLevelFirst;
    }
    if (keepInstanced || (dynamic && p.build != TreeBuild::Instanced && treeBuilderOf(p) != 1u)) {
        if (!keepInstanced && (levelFirst->empty() || levelFirst->size() > kMaxTreeLevels || levelFirst->size() != depth))
            return fail(SLRHIP_ERR_HIP, "slrhip_upload_scene: the tree has no level table (internal error)");
        HIP_TRY(ctx->geoVertices.alloc(d.num_vertices));
        HIP_TRY(hipMemcpy(ctx->geoVertices.ptr, d.vertices, (size_t)d.num_vertices * sizeof(slrhip_vertex), hipMemcpyHostToDevice));
        HIP_TRY(ctx->geoTriangles.alloc(d.num_triangles));
        HIP_TRY(hipMemcpy(ctx->geoTriangles.ptr, d.triangles, (size_t)d.num_triangles * sizeof(slrhip_triangle), hipMemcpyHostToDevice));
        HIP_TRY(ctx->geoLeafBoxes.alloc(2u * (size_t)leafRefs));
        HIP_TRY(ctx->geometryStatus.alloc(1));
        HIP_TRY(hipMemset(ctx->geometryStatus.ptr, 0, sizeof(uint32_t)));
        ctx->geoLevelFirst = *levelFirst;
        ctx->geoLevelFirst.push_back(keepInstanced ? p.bvh.topNodes : numNodes);
        ctx->geoInstanced = keepInstanced;
        ctx->geoNumVertices = d.num_vertices; ctx->geoNumTriangles = d.num_triangles; ctx->geoNumLights = (uint32_t)p.lightTris.size();
        ctx->geoNumAlphaRecords = (uint32_t)(p.alphaTris.size() / 2u); ctx->geoHasTriUV = !p.triUV.empty();
        ctx->geoLastLaunches = 0;
        ctx->geometryKept = true;
    }
    // the ray queries' error word: allocated here, so that a query call allocates nothing (and can be captured in a graph)
    HIP_TRY(ctx->queryError.alloc(1));
    HIP_TRY(hipMemset(ctx->queryError.ptr, 0, sizeof(uint32_t)));
    bindScene(ctx, d, p, numNodes, quantized);
    ctx->envOwnMap = false;
    // what slrhip_set_materials checks new tables against
    ctx->matKept.usage = p.usage;
    ctx->matKept.textures = p.textures;
    ctx->matKept.numTexTexels = p.texTexels.size() / 3u;
    ctx->matKept.upsampling = p.gridWidth != 0;
    ctx->matLastLaunches = 0; ctx->matLastRebuilt = false;
    ctx->bvhDepth = depth;
    ctx->bvhLeafRefs = leafRefs;
    ctx->treeBuilder = treeBuilderOf(p);
    ctx->haveScene = true;
    return SLRHIP_OK;
}

// Overrides of the render plan, each read once per process (the first two by measurement builds only: tuningEnv).
long slrhip::autoStripesOverride() { static const long v = [] { const char* e = tuningEnv("SLRHIP_AUTO_STRIPES"); return e ? atol(e) : 0L; }(); return v; }
int slrhip::pairsMask() { static const int v = [] { const char* e = tuningEnv("SLRHIP_PAIRS"); return e ? atoi(e) : kDefaultPairs; }(); return v; }
uint32_t slrhip::runLengthOverride() {
    static const uint32_t v = [] { const char* e = getenv("SLRHIP_RUN_LENGTH"); const long n = e ? atol(e) : 0L; return n >= 1 && n <= 4096 ? (uint32_t)n : 0u; }();
    return v;
}

// Points a zero-initialised PathBuffers at the context's render arrays and assigns it to ctx->buffers in one go.
static void bindBuffers(slrhip_ctx* ctx, const FramePlan& plan) {
    PathBuffers pb{};
    // per-slot path state; the second record of a pair (stride 2) is element 1 of the first one's array
    pb.rayStride = plan.rayStride; pb.spStride = plan.spStride; pb.hdrStride = plan.hdrStride;
    pb.rayOrg = ctx->rayOrg.ptr; pb.rayDir = plan.rayStride == 2 ? ctx->rayOrg.ptr + 1 : ctx->rayDir.ptr;
    pb.spR = ctx->spR.ptr; pb.spC = plan.spStride == 2 ? ctx->spR.ptr + 1 : ctx->spC.ptr;
    pb.hdr = ctx->hdr.ptr; pb.rng = plan.hdrStride == 2 ? ctx->hdr.ptr + 1 : ctx->rng.ptr;
    pb.hit = ctx->hit.ptr; pb.hitInstance = ctx->scene.instances ? ctx->hitInstance.ptr : nullptr;
    pb.alpha = ctx->alpha.ptr; pb.pdfPrev = plan.spectral ? ctx->pdfPrev.ptr : nullptr;
    pb.nee = ctx->nee.ptr; pb.shadowDir = ctx->shadowDir.ptr; pb.visible = ctx->visible.ptr; pb.flags = ctx->flags.ptr;
    // result window (slrhip_render sizes it), sensor, pixel list
    pb.results = ctx->results.ptr; pb.fbSum = ctx->fbSum.ptr; pb.fbComp = ctx->fbComp.ptr; pb.pixelXY = ctx->pixelXY.ptr;
    // queues and counters
    pb.cursor = ctx->cursor.ptr; pb.shadowQueue = ctx->shadowQueue.ptr; pb.tailList = ctx->tailList.ptr; pb.queueCount = ctx->queueCount.ptr;
    pb.idleShards = ctx->idleShards.ptr; pb.blockDead = ctx->blockDead.ptr; pb.totals = ctx->totals.ptr;
    // the status words
    uint32_t* const status = ctx->activeSlots.ptr;
    pb.activeSlots = status + S_LIVE; pb.errorWord = status + S_ERROR; pb.windowSamples = status + S_WINDOW_SAMPLES;
    pb.tailIdled = status + S_TAIL_IDLED; pb.tailMode = status + S_TAIL_MODE; pb.tailWords = status + S_TAIL_LENGTH;
    ctx->buffers = pb;
}

// Copies the first `count` status words to the host and waits for them.
static hipError_t readStatus(slrhip_ctx* ctx, uint32_t* words, uint32_t count, hipStream_t s) {
    const hipError_t e = hipMemcpyAsync(words, ctx->activeSlots.ptr, count * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
    return e == hipSuccess ? hipStreamSynchronize(s) : e;
}

// The window is complete only if the queues handed out exactly one sample per pixel and pass: the device's own count
// (k_count_samples over the queues' cursors) against the host's arithmetic.  A lost or repeated sample would leave a stale
// or overwritten entry in the result window — never silent.
static int checkWindow(slrhip_ctx* ctx, uint32_t workItems, hipStream_t s) {
    uint32_t words[kStatusWords] = {};
    HIP_TRY(readStatus(ctx, words, kStatusWords, s));
    if (words[S_ERROR]) return deviceError(words[S_ERROR]);
    if (words[S_WINDOW_SAMPLES] != workItems)
        return fail(SLRHIP_ERR_HIP, "slrhip_render: the work queues handed out " + std::to_string(words[S_WINDOW_SAMPLES]) + " samples for a window of " +
                                        std::to_string(workItems) + " (internal error)");
    return SLRHIP_OK;
}

// Tail mode seen in the status words: list the live slots, finish them, read the words again (live slots must be 0 then).
// `status` are the loop's words (S_LIVE .. S_TAIL_MODE), updated here.
static int runTail(slrhip_ctx* ctx, const PathBuffers& pb, const RenderParams& rp, uint32_t* status, hipStream_t s, bool timed) {
    struct Timer {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        ~Timer() { if (t0) (void)hipEventDestroy(t0); if (t1) (void)hipEventDestroy(t1); }
    } timer;
    if (timed) { HIP_TRY(hipEventCreate(&timer.t0)); HIP_TRY(hipEventCreate(&timer.t1)); HIP_TRY(hipEventRecord(timer.t0, s)); }
    if (!launchTail(ctx->shadeVariant, ctx->scene, pb, rp, status[S_LIVE], ctx->numCUs, s))
        return fail(SLRHIP_ERR_HIP, "slrhip_render: no k_tail is built for the window's shade variant (internal error)");
    ctx->tailLaunched = true;
    if (timed) HIP_TRY(hipEventRecord(timer.t1, s));
    HIP_TRY(hipGetLastError());
    const uint32_t liveBefore = status[S_LIVE];
    uint32_t words[S_TAIL_CURSOR + 1] = {};
    HIP_TRY(readStatus(ctx, words, S_TAIL_CURSOR + 1, s));
    std::memcpy(status, words, (S_TAIL_MODE + 1) * sizeof(uint32_t));
    if (timed) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, timer.t0, timer.t1));
        ctx->profMs[SLRHIP_KERNEL_TAIL] += ms;
        ++ctx->profLaunches[SLRHIP_KERNEL_TAIL];
    }
    if (status[S_ERROR]) return deviceError(status[S_ERROR]);
    if (words[S_TAIL_IDLED] != words[S_TAIL_LENGTH])
        return fail(SLRHIP_ERR_HIP, "slrhip_render: the tail kernel left " + std::to_string(words[S_TAIL_LENGTH] - words[S_TAIL_IDLED]) + " of " +
                                        std::to_string(words[S_TAIL_LENGTH]) + " listed slots live (live count before: " + std::to_string(liveBefore) +
                                        ", cursor " + std::to_string(words[S_TAIL_CURSOR]) + "; internal error)");
    // every listed slot ended idle and the wavefront kernels are off (tail mode): nothing is live any more
    HIP_TRY(hipMemsetAsync(ctx->activeSlots.ptr + S_LIVE, 0, sizeof(uint32_t), s));
    status[S_LIVE] = 0;
    return SLRHIP_OK;
}

// One wavefront iteration = k_shade (advance every live path by one vertex; finish and restart the paths that end) then
// k_trace_ws (the extension and shadow rays that left).  Each check of the live-slot word costs one small copy + stream
// sync; 16 iterations between checks keeps it < 1 %.
const int kCheckEvery = 16;
const int kEventsPerIteration = 3;    // SLRHIP_FLAG_TIME_KERNELS: before shade, after shade, after trace

// One block of kCheckEvery iterations as plain launches on `s`, with the context's timing events around each kernel if `timed`.
static hipError_t launchBlock(slrhip_ctx* ctx, const PathBuffers& pb, const RenderParams& rp, uint32_t traceBlocks, bool timed, hipStream_t s) {
    const bool count = (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) != 0;
    hipError_t e = hipSuccess;
    for (int k = 0; k < kCheckEvery; ++k) {
        const uint32_t parity = (uint32_t)(k & 1);
        hipEvent_t* ev = timed ? &ctx->events[(size_t)k * kEventsPerIteration] : nullptr;
        if (ev && e == hipSuccess) e = hipEventRecord(ev[0], s);
        if (!launchShade(ctx->shadeVariant, ctx->scene, pb, rp, parity, s)) return hipErrorInvalidDeviceFunction;      // (renderWindow has checked the row)
        ctx->shadeLaunched = true;
        if (ev && e == hipSuccess) e = hipEventRecord(ev[1], s);
        launchTraceWs(ctx->scene, pb, rp, parity, traceBlocks, count, s);
        if (ev && e == hipSuccess) e = hipEventRecord(ev[2], s);
    }
    return e;
}

// SLRHIP_ITER_LOG=path (with SLRHIP_FLAG_TIME_KERNELS): per-iteration kernel times of a window, one line per iteration
// "iteration shade_ms trace_ms live_slots_at_block_end" — how the drain of a render's last paths was measured
struct IterationTimes { float ms[2]; uint32_t live; };
static void writeIterationLog(const char* path, const RenderParams& rp, const std::vector<IterationTimes>& log) {
    FILE* f = log.empty() ? nullptr : fopen(path, "a");
    if (!f) return;
    fprintf(f, "# render: %u slots, %u passes from %u\n", rp.numSlots, rp.sppCount, rp.sppBegin);
    for (size_t i = 0; i < log.size(); ++i) fprintf(f, "%zu %.4f %.4f %u\n", i, log[i].ms[0], log[i].ms[1], log[i].live);
    fclose(f);
}

// The event times of the block just finished: into the profile, and into the iteration log if there is one.
static int readBlockTimes(slrhip_ctx* ctx, uint32_t live, std::vector<IterationTimes>* log) {
    static const int cls[2] = {SLRHIP_KERNEL_SHADE, SLRHIP_KERNEL_TRACE};
    for (int k = 0; k < kCheckEvery; ++k) {
        hipEvent_t* ev = &ctx->events[(size_t)k * kEventsPerIteration];
        IterationTimes t = {{0.0f, 0.0f}, live};
        for (int j = 0; j < 2; ++j) {
            HIP_TRY(hipEventElapsedTime(&t.ms[j], ev[j], ev[j + 1]));
            ctx->profMs[cls[j]] += t.ms[j];
            ++ctx->profLaunches[cls[j]];
        }
        if (log) log->push_back(t);
    }
    return SLRHIP_OK;
}

// hipGraph of one block of iterations: released on every path out of renderWindow
struct BlockGraph {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    ~BlockGraph() { if (exec) (void)hipGraphExecDestroy(exec); if (graph) (void)hipGraphDestroy(graph); }
};

// One window of passes [sppBegin, sppBegin + sppCount): every sample of the window rendered into the result window, then folded
// into the sensor in pass order.  slrhip_render sizes the windows.  The window runs on its OWN copy of the render parameters and
// the buffer table: ctx->params and ctx->buffers stay the shard's (the resolves, the statistics, the feature passes and
// slrhip_camera_rays read them).  `active` (slrhip_render_adaptive): the window is over that list — its length as the pixel count, its
// xy as the pixel list, its index as the map of the fold; the slots, the queues' owners and the tail bound stay the shard's.
int slrhip::renderWindow(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, hipStream_t stream, const ActiveWindow* active) {
    RenderParams rp = ctx->params;
    PathBuffers pb = ctx->buffers;
    if (active) { rp.numPixels = active->count; pb.pixelXY = active->xy; }
    const WindowPlan window = planWindow(rp.numPixels, sppCount, runLengthOverride());
    rp.sppBegin = sppBegin; rp.sppCount = sppCount;
    rp.workItems = window.workItems; rp.runLength = window.runLength; rp.numRuns = window.numRuns;
    // the primary pass of the window (render_plan.cpp, planPrimary); its instance plane is allocated before anything is queued
    const PrimaryPlan primary = planPrimary(rp.numPixels, sppCount, ctx->config.flags, ctx->scene.instances != nullptr, rp.spectral != 0,
                                            ctx->scene.hasEnv != 0, ctx->scene.nodesQ != nullptr);
    rp.primary = primary.on ? 1u : 0u;
    pb.primaryInstance = nullptr;
    if (primary.instanceEntries) {
        HIP_TRY(ctx->primaryInstance.alloc((size_t)primary.instanceEntries));
        pb.primaryInstance = ctx->primaryInstance.ptr;
    }
    // ... and so is the plane of the streams the pass leaves behind the camera draws (the fused start of k_shade goes on from them)
    pb.primaryRng = nullptr;
    if (primary.rngEntries) {
        HIP_TRY(ctx->primaryRng.alloc((size_t)primary.rngEntries));
        pb.primaryRng = ctx->primaryRng.ptr;
    }
    ctx->primaryRngEntries = pb.primaryRng ? ctx->primaryRng.count : 0u;       // what this window bound, not what the plan said
    ctx->primaryKernel = PrimaryKernel::None;                                  // ... and what it launched (set where the pass is launched, below)
    // the k_shade instantiation of the window, chosen once (render_plan.cpp, planShadeVariant); a variant no file builds is refused here
    ctx->shadeVariant = planShadeVariant(rp.spectral != 0, ctx->scene.shadeTables != nullptr, ctx->scene.hasMicrofacet != 0, ctx->scene.hasMulti != 0,
                                         ctx->scene.numTextures, rp.primary != 0, pb.primaryRng != nullptr);
    ctx->shadeLaunched = ctx->tailLaunched = false;
    if (!findShadeKernel(ctx->shadeVariant)) return fail(SLRHIP_ERR_HIP, "slrhip_render: no k_shade is built for the window's shade variant (internal error)");
    // the first window after render_begin also clears the sensor (the buffers are reused across render_begin calls), even when
    // it is asked for zero passes
    launchResetSlots(pb, rp, ctx->firstRenderCall, stream);
    ctx->firstRenderCall = false;
    if (sppCount == 0) return SLRHIP_OK;
    // persistent traversal workgroups of the wave-specialised kernel (pt_trace_ws.hip): a fixed number per CU
    const uint32_t traceBlocks = (uint32_t)ctx->numCUs * (uint32_t)traceWsBlocksPerCU(ctx->scene.nodesQ != nullptr);

    // the end of the window: the tail kernel's bound (render_plan.cpp, tailSlots)
    static const long envTail = [] { const char* e = getenv("SLRHIP_TAIL_SLOTS"); return e ? atol(e) : -1L; }();
    const bool counting = (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) != 0;
    rp.tailSlots = tailSlots(rp.numSlots, SLR_TAIL_DIVISOR, (ctx->config.flags & SLRHIP_FLAG_TAIL_KERNEL) != 0 || ctx->config.stripes == 0, envTail,
                             !counting);

    const bool timeKernels = (ctx->config.flags & SLRHIP_FLAG_TIME_KERNELS) != 0;
    if (timeKernels && ctx->events.empty()) {
        ctx->events.resize((size_t)kCheckEvery * kEventsPerIteration);
        for (hipEvent_t& e : ctx->events) HIP_TRY(hipEventCreate(&e));
    }
    static const char* iterLogPath = getenv("SLRHIP_ITER_LOG");
    std::vector<IterationTimes> iterLog;

    // The primary pass: every camera ray of the window, on the caller's stream after the reset (which clears the error word) and
    // before the iterations; a launch takes as many whole passes as stay under 2^31 samples.  With SLRHIP_FLAG_TIME_KERNELS its
    // launches and event time are booked under SLRHIP_KERNEL_TRACE (read once the window's stream work is complete, below).
    struct PrimaryTimer {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        ~PrimaryTimer() { if (t0) (void)hipEventDestroy(t0); if (t1) (void)hipEventDestroy(t1); }
    } primaryTimer;
    if (primary.on) {
        if (timeKernels) { HIP_TRY(hipEventCreate(&primaryTimer.t0)); HIP_TRY(hipEventCreate(&primaryTimer.t1)); HIP_TRY(hipEventRecord(primaryTimer.t0, stream)); }
        for (uint32_t first = 0; first < sppCount; first += primary.passesPerLaunch)
            launchPrimary(ctx->scene, pb, rp, first, std::min(primary.passesPerLaunch, sppCount - first), primary.kernel, ctx->numCUs, stream);
        if (timeKernels) HIP_TRY(hipEventRecord(primaryTimer.t1, stream));
        HIP_TRY(hipGetLastError());
        ctx->primaryKernel = primary.kernel;
    }

    // The block of kCheckEvery iterations is the same sequence of launches every time (the parity alternates inside it and is
    // back to 0 at its end), so it is captured ONCE per window into a hipGraph and replayed: one submission per block instead
    // of 32 launches with their dispatch gaps — what is left of the cost of the nearly empty iterations at the end of a
    // render.  Capture needs a real stream, so the work runs on the context's own stream, ordered after the caller's by an
    // event; render() returns only after that stream is idle, which orders the caller's later work after it.  Not when the
    // kernels are timed (the events go between the launches) and not for small frames.
    static const bool noGraph = [] { const char* e = getenv("SLRHIP_GRAPH"); return e && std::string(e) == "0"; }();
    BlockGraph block;
    hipStream_t s = stream;          // the stream of everything below
    if (!timeKernels && !noGraph && rp.numSlots >= (1u << 18)) {
        if (!ctx->workStream) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->workStream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ctx->userReady, hipEventDisableTiming));
        }
        s = ctx->workStream;
        HIP_TRY(hipEventRecord(ctx->userReady, stream));          // the reset kernel above and whatever the caller queued before
        HIP_TRY(hipStreamWaitEvent(s, ctx->userReady, 0));
        HIP_TRY(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        (void)launchBlock(ctx, pb, rp, traceBlocks, false, s);      // untimed: its only early return is a missing k_shade row, refused above
        hipError_t ce = hipStreamEndCapture(s, &block.graph);
        if (ce == hipSuccess) ce = hipGraphInstantiate(&block.exec, block.graph, nullptr, nullptr, 0);
        if (ce != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_render: hipGraph capture failed: ") + hipGetErrorString(ce));
    }

    const uint64_t maxIterations = ((uint64_t)rp.workItems / rp.numSlots + 2) * 128 + 1024;   // paths are <= 100 vertices long
    uint64_t it = 0;
    uint32_t status[S_TAIL_MODE + 1] = {rp.numSlots, 0u, 0u, 0u};
    while (status[S_LIVE] > 0) {
        hipError_t e = block.exec ? hipGraphLaunch(block.exec, s) : launchBlock(ctx, pb, rp, traceBlocks, timeKernels, s);
        if (e == hipSuccess && !block.exec) e = hipGetLastError();          // a failed launch surfaces here, not at the end of the render
        if (e == hipSuccess) e = readStatus(ctx, status, S_TAIL_MODE + 1, s);
        if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_render: ") + hipGetErrorString(e));
        it += kCheckEvery;
        if (status[S_ERROR]) return deviceError(status[S_ERROR]);
        if (timeKernels) {
            const int rc = readBlockTimes(ctx, status[S_LIVE], iterLogPath ? &iterLog : nullptr);
            if (rc != SLRHIP_OK) return rc;
        }
        if (status[S_TAIL_MODE] && status[S_LIVE]) {
            const int rc = runTail(ctx, pb, rp, status, s, timeKernels);
            if (rc != SLRHIP_OK) return rc;
        }
        if (it > maxIterations) return fail(SLRHIP_ERR_HIP, "slrhip_render: iteration bound exceeded (internal error)");
    }
    ctx->iterations += it;
    if (primary.on && timeKernels) {
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, primaryTimer.t0, primaryTimer.t1));       // complete: the loop above waited for work queued after it
        ctx->profMs[SLRHIP_KERNEL_TRACE] += ms;
        ctx->profLaunches[SLRHIP_KERNEL_TRACE] += primary.numLaunches;
    }
    launchCountSamples(pb, rp, s);     // samples rendered in this window, counted on the device (T_SAMPLES)
    const ClampParams clamp = clampParams(ctx);                                          // slrhip_clamp_begin: every sample through the clamp first
    if (active) launchFoldIndexed(pb, rp, ctx->stats.records.ptr, active->index, clamp, s);       // the same, scattered to the list's pixels of the shard
    else launchFold(pb, rp, ctx->stats.on ? ctx->stats.records.ptr : nullptr, clamp, s);       // sensor->add, in pass order (+ the noise records)
    HIP_TRY(hipGetLastError());
    const int rc = checkWindow(ctx, rp.workItems, s);
    if (rc == SLRHIP_OK && iterLogPath) writeIterationLog(iterLogPath, rp, iterLog);
    return rc;
}

int slrhip::clearStatistics(slrhip_ctx* ctx, hipStream_t stream) {
    const size_t bytes = std::max<size_t>(ctx->params.numPixels, 1u) * sizeof(float4);
    const auto clear = [&](auto& r) {
        if (!r.on || !r.clear) return hipSuccess;
        const hipError_t e = hipMemsetAsync(r.records.ptr, 0, bytes, stream);
        if (e == hipSuccess) r.clear = false;
        return e;
    };
    HIP_TRY(clear(ctx->clamp));          // the clamp records first: every statistics-aware call may touch them as well
    HIP_TRY(clear(ctx->stats));
    return SLRHIP_OK;
}

uint64_t slrhip::resultWindowBudget() {
    uint64_t budget = 16ull << 30;
    if (const char* e = getenv("SLRHIP_RESULT_WINDOW_MB")) { const long mb = atol(e); if (mb > 0) budget = (uint64_t)mb << 20; }
    return budget;
}

extern "C" {

const char* slrhip_last_error_string(void) { return g_lastError.c_str(); }
int slrhip_version(void) { return SLRHIP_VERSION; }

int slrhip_create(const slrhip_config* config, slrhip_ctx** out) {
    if (!config || !out) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_create: null argument");
    *out = nullptr;
    if (config->mode != SLRHIP_MODE_RGB && config->mode != SLRHIP_MODE_SPECTRAL)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_create: unknown mode");
    // the per-pixel sample pool tracks the stripes of a pixel in a 64-bit mask (PathBuffers::finishedMask)
    if (config->stripes > SLRHIP_MAX_STRIPES)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_create: at most 64 sample stripes per pixel (slrhip_config::stripes)");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(SLRHIP_ERR_NO_DEVICE, std::string("slrhip_create: no HIP device (") + hipGetErrorString(e) + ")");
    if (config->device < 0 || config->device >= n) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_create: device ordinal out of range");
    HIP_TRY(hipSetDevice(config->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, config->device));
    slrhip_ctx* ctx = new slrhip_ctx();
    ctx->config = *config;
    ctx->device = config->device;
    ctx->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    *out = ctx;
    return SLRHIP_OK;
}

int slrhip_destroy(slrhip_ctx* ctx) {
    if (!ctx) return SLRHIP_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    delete ctx;
    return SLRHIP_OK;
}

int slrhip_components(const slrhip_ctx* ctx) { return ctx && ctx->config.mode == SLRHIP_MODE_SPECTRAL ? 16 : 3; }

int slrhip_upload_scene(slrhip_ctx* ctx, const slrhip_scene_desc* d) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_upload_scene: null argument");
    const auto t0 = std::chrono::steady_clock::now();
    PreparedScene p;
    std::string err;
    if (const int rc = prepareScene(*d, ctx->config, &p, &err)) return fail(rc, err);     // the context is untouched so far
    if (const int rc = commitScene(ctx, *d, p)) return rc;
    ctx->buildSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return SLRHIP_OK;
}

int slrhip_render_begin(slrhip_ctx* ctx, const slrhip_render_settings* st, slrhip_shard shard) {
    if (!ctx || !st) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_begin: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render_begin: no scene uploaded");
    const bool spectral = ctx->config.mode == SLRHIP_MODE_SPECTRAL;
    FramePlan plan;
    std::string err;
    if (const int rc = planFrame(st->image_width, st->image_height, shard.shard_index, shard.shard_count, ctx->config.stripes, spectral,
                                 autoStripesOverride(), pairsMask(), &plan, &err))
        return fail(rc, err);                                                          // the context is untouched so far
    // An allocation may free an array of the previous render state before it fails, so the context holds no render state from
    // here on until the last step has succeeded (as commitScene does for the scene).
    ctx->haveRender = false;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t slots = plan.slotCapacity, planes = spectral ? 4 : 1, pixels = std::max(plan.numPixels, 1u);
    // The ORDER of the skewed allocations is part of the measured layout: g_skewCounter advances once per skewed array that
    // really allocates, so the order fixes every array's offset modulo the HBM channel interleave.
    hipError_t e = ctx->pixelXY.upload(shardPixels(plan));
    const auto alloc = [&e](auto& array, size_t n, bool skew) { if (e == hipSuccess) e = array.alloc(n, skew); };
    alloc(ctx->rayOrg, slots * plan.rayStride, true); alloc(ctx->rayDir, plan.rayStride == 2 ? 1 : slots, true); alloc(ctx->hit, slots, true);
    alloc(ctx->alpha, slots * planes, true); alloc(ctx->spR, slots * planes * plan.spStride, true); alloc(ctx->spC, plan.spStride == 2 ? 1 : slots * planes, true);
    alloc(ctx->fbSum, pixels * planes, true); alloc(ctx->fbComp, pixels * planes, true);
    alloc(ctx->nee, slots * planes, true); alloc(ctx->shadowDir, slots, true); alloc(ctx->pdfPrev, spectral ? slots : 1, true);
    alloc(ctx->hdr, slots * plan.hdrStride, true); alloc(ctx->rng, plan.hdrStride == 2 ? 1 : slots, true);
    alloc(ctx->cursor, slots / 64u, false); alloc(ctx->idleShards, kShards * kCounterStride, false);
    alloc(ctx->flags, slots, true); alloc(ctx->visible, slots, true);
    if (ctx->scene.instances) alloc(ctx->hitInstance, slots, true);
    alloc(ctx->shadowQueue, (size_t)plan.shardCapacity * kShards, true); alloc(ctx->tailList, slots, true);
    alloc(ctx->blockDead, plan.numBlocks, false); alloc(ctx->queueCount, 2 * kQueueSetWords, false);
    alloc(ctx->activeSlots, kStatusWords, false); alloc(ctx->totals, (size_t)T_KINDS * kShards * kTotalStride, false);
    if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_render_begin: allocating the path state: ") + hipGetErrorString(e));
    // The statistics restart here.  A memset of device memory is only ordered on the null stream, and slrhip_render may be
    // given a NON-BLOCKING stream, which the null stream does not wait for and which does not wait for it: the memset has to
    // be complete before this call returns.  (Round 1, gpurun_out/overlap.log: this function also cleared queueCount with a
    // second null-stream memset and did not wait; on a non-blocking stream k_reset_slots — which writes the initial regen
    // counts into queueCount — could run BEFORE that memset landed, the counts were wiped, no slot ever started a sample and
    // slrhip_render ran into its iteration bound.  queueCount is now written by k_reset_slots alone, in stream order.)
    HIP_TRY(hipMemsetAsync(ctx->totals.ptr, 0, ctx->totals.count * sizeof(uint64_t), nullptr));
    HIP_TRY(hipMemsetAsync(ctx->activeSlots.ptr, 0, kStatusWords * sizeof(uint32_t), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));

    bindBuffers(ctx, plan);
    RenderParams rp{};
    rp.numSlots = plan.numSlots; rp.numWaves = rp.numSlots / 64u;
    rp.numPixels = plan.numPixels; rp.stripes = plan.stripes;
    rp.runLength = 1;                                     // the window's passes, runs and tail bound: renderWindow
    rp.rngSeed = st->rng_seed; rp.timeStart = st->time_start; rp.timeEnd = st->time_end;
    rp.imageWidth = plan.width; rp.imageHeight = plan.height;
    rp.countSlots = (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) ? 1u : 0u;
#ifndef SLR_FORCE_TRACE_ALL_SHADOWS
#define SLR_FORCE_TRACE_ALL_SHADOWS 0      // 1 (variant builds): every context traces every shadow ray — the same kernels without the rays removed
#endif
    rp.traceAllShadows = (SLR_FORCE_TRACE_ALL_SHADOWS || (ctx->config.flags & (SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS | SLRHIP_FLAG_COUNT_TRAVERSAL))) ? 1u : 0u;
    rp.shardCapacity = plan.shardCapacity;
    rp.spectral = spectral ? 1u : 0u;
    rp.injectError = (ctx->config.flags & SLRHIP_FLAG_TEST_DEVICE_ERROR) ? 1u : 0u;
    ctx->params = rp;
    ctx->settings = *st;
    ctx->shard = shard;
    ctx->iterations = 0;
    ctx->firstRenderCall = true;
    ctx->featChannels = 0; ctx->featPassEnd = 0;                              // the feature accumulation restarts (its arrays are kept for reuse)
    ctx->featErrorReady = false; ctx->albReady = false; ctx->albPasses = 0;   // ... and the albedo accumulation and the error word they share
    ctx->motionReady = false;                                                 // ... and the motion accumulation
    ctx->stats.on = false; ctx->stats.clear = true;                           // statistics are per render (slrhip_statistics_begin); the records are kept, stale
    ctx->clamp.on = false; ctx->clamp.clear = true;                           // ... and so is the clamp (slrhip_clamp_begin)
    ctx->activePixels = plan.numPixels; ctx->activeList = -1;                 // every pixel is active again (slrhip_render_adaptive)
    ctx->haveRender = true;
    return SLRHIP_OK;
}

int slrhip_render(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render: call slrhip_render_begin first");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    const RenderParams& rp = ctx->params;
    if (rp.numSlots == 0) { ctx->firstRenderCall = false; return SLRHIP_OK; }
    if (const int rc = clearStatistics(ctx, stream)) return rc;       // ordered before the fold: renderWindow's own stream waits for `stream`
    const uint32_t window = planWindows(rp.numPixels, rp.spectral != 0, sppCount, resultWindowBudget());
    HIP_TRY(ctx->results.alloc((size_t)window * rp.numPixels * (rp.spectral ? 4u : 1u)));
    ctx->buffers.results = ctx->results.ptr;
    if (sppCount == 0) return renderWindow(ctx, sppBegin, 0, stream);
    for (uint32_t done = 0; done < sppCount; done += window) {
        const int rc = renderWindow(ctx, sppBegin + done, std::min(window, sppCount - done), stream);
        if (rc != SLRHIP_OK) return rc;
    }
    return SLRHIP_OK;
}

int slrhip_resolve_framebuffer(slrhip_ctx* ctx, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (!ctx || !deviceDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_framebuffer: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_resolve_framebuffer: nothing rendered");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_framebuffer: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), stream));
    if (rp.numPixels) launchResolve(ctx->buffers, rp, deviceDst, stream);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

// The one exchange step of the multi-GPU path: every rank resolves its shard (zeros outside its tiles) and the
// frames are summed onto `root` — disjoint supports, so the sum is a gather.  RCCL is loaded on first use (dlopen), so a
// single-GPU host does not need librccl at all; the communicator is the caller's (one process per GPU, ncclCommInitRank).
int slrhip_reduce_framebuffer(slrhip_ctx* ctx, void* ncclComm, int root, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (!ctx || !ncclComm) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_reduce_framebuffer: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_reduce_framebuffer: nothing rendered");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (deviceDst && numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_reduce_framebuffer: destination too small");
    typedef int (*reduce_fn)(const void*, void*, size_t, int, int, int, void*, hipStream_t);
    typedef int (*rank_fn)(void*, int*);
    static void* rccl = [] {
        void* h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        return h ? h : dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    }();
    static reduce_fn ncclReduceFn = rccl ? reinterpret_cast<reduce_fn>(dlsym(rccl, "ncclReduce")) : nullptr;
    static rank_fn ncclCommUserRankFn = rccl ? reinterpret_cast<rank_fn>(dlsym(rccl, "ncclCommUserRank")) : nullptr;
    if (!ncclReduceFn || !ncclCommUserRankFn) return fail(SLRHIP_ERR_UNSUPPORTED, "slrhip_reduce_framebuffer: librccl.so (ncclReduce) not found");
    // only the root receives: it must hand over a destination (RCCL would fault on a null recvbuff, not return an error)
    int myRank = -1;
    if (ncclCommUserRankFn(ncclComm, &myRank) != 0) return fail(SLRHIP_ERR_HIP, "slrhip_reduce_framebuffer: ncclCommUserRank failed");
    if (myRank == root && !deviceDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_reduce_framebuffer: the root rank needs a destination buffer");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    int rc = slrhip_resolve_framebuffer(ctx, ctx->resolveScratch.ptr, need, streamPtr);
    if (rc != SLRHIP_OK) return rc;
    const int kNcclFloat32 = 7, kNcclSum = 0;      // rccl.h: ncclDataType_t / ncclRedOp_t
    const int nrc = ncclReduceFn(ctx->resolveScratch.ptr, deviceDst, need, kNcclFloat32, kNcclSum, root, ncclComm, (hipStream_t)streamPtr);
    if (nrc != 0) return fail(SLRHIP_ERR_HIP, "slrhip_reduce_framebuffer: ncclReduce failed (" + std::to_string(nrc) + ")");
    return SLRHIP_OK;
}

int slrhip_read_framebuffer(slrhip_ctx* ctx, float* hostDst, size_t numFloats) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_framebuffer: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_read_framebuffer: nothing rendered");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_framebuffer: destination too small");
    return readThroughScratch(ctx, hostDst, need, need, false, nullptr, [&](float* scratch) { return slrhip_resolve_framebuffer(ctx, scratch, need, nullptr); });
}

int slrhip_synchronize(slrhip_ctx* ctx) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_synchronize: null context");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    return SLRHIP_OK;
}

int slrhip_get_counters(slrhip_ctx* ctx, slrhip_counters* out) {
    if (!ctx || !out) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_get_counters: null argument");
    std::memset(out, 0, sizeof(*out));
    out->bvh_nodes = ctx->nodes.count;
    out->bvh_depth = ctx->bvhDepth;
    out->bvh_leaf_references = ctx->bvhLeafRefs;
    out->build_seconds = ctx->buildSeconds;
    out->iterations = ctx->iterations;
    if (ctx->haveRender) {
        uint64_t t[T_KINDS];
        int rc = readTotals(ctx, t);
        if (rc != SLRHIP_OK) return rc;
        out->extension_rays = t[T_EXT_RAYS];
        out->shadow_rays = t[T_SHADOW_RAYS];
        out->samples = t[T_SAMPLES];          // counted on the device from the slots' sample headers (k_count_samples)
    }
    return SLRHIP_OK;
}

int slrhip_get_profile(slrhip_ctx* ctx, slrhip_profile* out) {
    if (!ctx || !out) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_get_profile: null argument");
    std::memset(out, 0, sizeof(*out));
    for (int k = 0; k < SLRHIP_KERNEL_COUNT; ++k) { out->launches[k] = ctx->profLaunches[k]; out->milliseconds[k] = ctx->profMs[k]; }
    if (ctx->haveRender) {
        uint64_t t[T_KINDS];
        int rc = readTotals(ctx, t);
        if (rc != SLRHIP_OK) return rc;
        out->rays[0] = t[T_EXT_RAYS]; out->rays[1] = t[T_SHADOW_RAYS];
        out->nodes[0] = t[T_NODES_CLOSEST]; out->triangles[0] = t[T_TRIS_CLOSEST];
        out->nodes[1] = t[T_NODES_SHADOW]; out->triangles[1] = t[T_TRIS_SHADOW];
        out->slot_visits = t[T_SLOT_VISITS];
    }
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): samples whose first hit came from the primary pass's record, as the kernels counted them.
int slrhip_debug_primary_samples(slrhip_ctx* ctx, uint64_t* samples) {
    if (!ctx || !samples) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_primary_samples: null argument");
    *samples = 0;
    if (!ctx->haveRender) return SLRHIP_OK;
    uint64_t t[T_KINDS];
    if (const int rc = readTotals(ctx, t)) return rc;
    *samples = t[T_PRIMARY_STARTS];
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): light samples k_shade did not trace, as it counted them (they are in shadow_rays as well).
int slrhip_debug_shadow_skipped(slrhip_ctx* ctx, uint64_t* rays) {
    if (!ctx || !rays) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_shadow_skipped: null argument");
    *rays = 0;
    if (!ctx->haveRender) return SLRHIP_OK;
    uint64_t t[T_KINDS];
    if (const int rc = readTotals(ctx, t)) return rc;
    *rays = t[T_SHADOW_SKIPPED];
    return SLRHIP_OK;
}

// Ray queries on device memory (slrhip_intersect_rays / slrhip_test_visibility): the render's wave-specialised traversal fed from
// the caller's ray array (pt_trace_indexed.hip, WsQueryIO).  Stream-ordered; no allocation, no copy, no host synchronisation: the
// only other work is clearing the query error word on the same stream.
static int checkQueryArgs(slrhip_ctx* ctx, const char* what, const void* rays, uint32_t n, const void* out, size_t outAlign, const void* extra) {
    const std::string w(what);
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": null context");
    if (n >= 0x80000000u) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": n >= 2^31 rays");
    if (n && (!rays || !out)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": null ray or result pointer");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)out & (outAlign - 1)) || ((uintptr_t)extra & 3u))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": misaligned pointer (rays: 16 bytes; hits: 16; instances / visible: 4)");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, w + ": no scene uploaded");
    return SLRHIP_OK;
}

static int runQuery(slrhip_ctx* ctx, const slrhip_ray* rays, uint32_t n, slrhip_hit* hits, int32_t* instances, uint32_t* visible, void* stream) {
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(ctx->queryError.ptr, 0, sizeof(uint32_t), s));
    launchQueryWs(ctx->scene, reinterpret_cast<const float4*>(rays), n, reinterpret_cast<float4*>(hits), instances, visible, ctx->queryError.ptr,
                  ctx->numCUs, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_intersect_rays(slrhip_ctx* ctx, const slrhip_ray* rays, uint32_t n, slrhip_hit* hits, int32_t* instances, void* stream) {
    int rc = checkQueryArgs(ctx, "slrhip_intersect_rays", rays, n, hits, 16, instances);
    if (rc != SLRHIP_OK || n == 0) return rc;
    return runQuery(ctx, rays, n, hits, instances, nullptr, stream);
}

int slrhip_test_visibility(slrhip_ctx* ctx, const slrhip_ray* rays, uint32_t n, uint32_t* visible, void* stream) {
    int rc = checkQueryArgs(ctx, "slrhip_test_visibility", rays, n, visible, 4, nullptr);
    if (rc != SLRHIP_OK || n == 0) return rc;
    return runQuery(ctx, rays, n, nullptr, nullptr, visible, stream);
}

int slrhip_query_status(slrhip_ctx* ctx, uint32_t* bits, void* stream) {
    if (!ctx || !bits) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_query_status: null argument");
    *bits = 0;
    if (!ctx->queryError.ptr) return SLRHIP_OK;          // no scene was ever uploaded: no query can have run
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(bits, ctx->queryError.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SLRHIP_OK;
}

} // extern "C"
