// slrhip_api.hip — the C ABI of include/slrhip.h over the HIP kernels.
//
// A scene is checked and flattened on the host by scene_prep.cpp, then committed here: the device tree build (if chosen),
// the uploads, the DevScene.  PathTracingRenderer::render's set-up (Renderers/PathTracingRenderer.cpp:27-70) is planned on the
// host by render_plan.cpp (pixel list, slot count, result windows, run lengths); render_begin allocates and binds the path state
// from that plan in one commit, and renderWindow drives the wavefront iterations of a window through one launch loop.
// There is no CPU fallback: without a HIP device every entry point fails loudly.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/slrhip.h"
#include "bvh.h"
#include "pt_clamp.h"
#include "pt_kernels.h"
#include "render_plan.h"
#include "scene_prep.h"

using namespace slrhip;

namespace {

const int kDefaultPairs = 1;                   // SLRHIP_PAIRS: the ray pair pays, the radiance-sum pair does not
const uint32_t kStatusWords = 8;               // PathBuffers::activeSlots .. tailWords: one small array, read back in one copy
enum StatusWord : uint32_t {                   // its words (bindBuffers points PathBuffers at them)
    S_LIVE = 0, S_ERROR = 1,                   // live slots; device error word
    S_TAIL_IDLED = 2, S_TAIL_MODE = 3,         // slots the tail kernel left idle; 1 + parity once the traversal kernel has handed over to it
    S_TAIL_LENGTH = 4, S_TAIL_CURSOR = 5,      // tail list length / cursor
    S_WINDOW_SAMPLES = 6                       // samples the queues handed out in the window
};
#ifndef SLR_TAIL_DIVISOR
#define SLR_TAIL_DIVISOR 8u      // the tail kernel never takes more than this fraction of the slots (1u in a variant build: the tail kernel as the whole renderer, measured in DESIGN.md)
#endif

thread_local std::string g_lastError;

int fail(int code, const std::string& msg) {
    g_lastError = msg;
    return code;
}

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

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(SLRHIP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));             \
    } while (0)

// hipMalloc returns 2 MiB-aligned blocks, so the record of slot i would sit at the same offset modulo
// the HBM channel interleave in every per-slot array, and a wave that loads its ten state records back to
// back would queue all of them on one channel ("partition camping").  Each array therefore starts at its
// own skew: a distinct odd multiple of 256 B plus a few KiB.
static std::atomic<size_t> g_skewCounter{0};     // shared by every context of the process; contexts may be set up from several threads

template <typename T>
struct DevArray {
    T* ptr = nullptr;
    void* base = nullptr;
    size_t count = 0, capacity = 0;
    ~DevArray() { release(); }
    void release() { if (base) { (void)hipFree(base); base = nullptr; ptr = nullptr; count = 0; capacity = 0; } }
    hipError_t alloc(size_t n, bool skew = false) {
        if (n == 0) n = 1;
        if (ptr && n <= capacity) { count = n; return hipSuccess; }     // reuse across render_begin calls
        release();
        capacity = n;
        size_t offset = 0;
        if (skew) { size_t k = ++g_skewCounter; offset = (k % 61) * 4352 + (k % 7) * 256; }
        hipError_t e = hipMalloc(&base, n * sizeof(T) + offset);
        if (e == hipSuccess) { ptr = reinterpret_cast<T*>(static_cast<char*>(base) + offset); count = n; }
        return e;
    }
    void adopt(T* devicePtr, size_t n) { release(); base = devicePtr; ptr = devicePtr; count = n; capacity = n; }      // takes ownership of a hipMalloc block
    hipError_t upload(const std::vector<T>& v) {
        hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpy(ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    }
};

uint32_t prevPowerOf2(uint32_t x) {   // defines.h:136-143
    x |= x >> 1; x |= x >> 2; x |= x >> 4; x |= x >> 8; x |= x >> 16;
    return x - (x >> 1);
}

} // namespace

struct slrhip_ctx {
    slrhip_config config;
    int device = 0;
    int numCUs = 256;
    bool haveScene = false;
    bool haveRender = false;

    // scene
    DevArray<QNode> nodes;
    DevArray<QNodeQ> nodesQ;
    DevArray<QNode8> nodes8;
    DevArray<DevTexture> textures;
    DevArray<DevMatTex> matTex;
    DevArray<float4> triUV, alphaTris;
    DevArray<float> texTexels;
    DevArray<LeafTri> leafTris;
    DevArray<ShadeTri> shadeTris;
    DevArray<LightTri> lightTris;
    DevArray<DevInstance> instances;
    DevArray<DevMaterial> materials;
    DevArray<DevMaterialS> materialsS;
    DevArray<DevSpectrum> spectra;
    DevArray<float> spectrumPool;
    DevArray<float> lightPMF, lightCDF;
    DevArray<float4> shadeTables;
    DevArray<float> envTexels, envTopPDF, envTopCDF, envRowPDF, envRowCDF;
    DevArray<uint8_t> gridCells;
    DevArray<float> pointUV, pointSpectrum;
    DevScene scene;
    uint32_t bvhDepth = 0;
    uint64_t bvhLeafRefs = 0;
    double buildSeconds = 0.0;

    // render state
    slrhip_render_settings settings;
    slrhip_shard shard;
    RenderParams params;
    DevArray<uint32_t> pixelXY;
    DevArray<uint4> rng;
    DevArray<float4> rayOrg, rayDir, hit, alpha, spR, spC, nee, shadowDir;
    DevArray<float4> results, fbSum, fbComp;      // result window of the current render call; the sensor (per-pixel Kahan sums)
    DevArray<uint32_t> cursor, idleShards;
    DevArray<float> pdfPrev;
    DevArray<uint4> hdr;
    DevArray<int32_t> hitInstance;
    DevArray<uint32_t> flags, visible, shadowQueue, tailList, queueCount, activeSlots, blockDead;
    DevArray<uint64_t> totals;
    DevArray<float> resolveScratch;
    DevArray<uint32_t> queryError;                // ERR_* bits of the ray queries (slrhip_query_status); apart from the render's error word
    // first-hit feature buffers (slrhip_render_features): allocated by the first feature call after render_begin, never by a render
    DevArray<float4> featGeometric, featShading, featTangent, featRecords;
    DevArray<float> featB2;
    DevArray<uint4> featIds;
    DevArray<uint32_t> featError;                 // ERR_* bits of the feature passes (slrhip_features_status)
    bool featReady = false;                       // sums allocated and cleared since render_begin
    uint32_t featChannels = 0;                    // the channel set of the feature calls since render_begin (0: none yet)
    uint32_t featWindow = 0;                      // passes per launch (the record window)
    uint64_t featPassEnd = 0;                     // 1 + the highest pass rendered since render_begin (whose ids the pixels hold)
    bool featErrorReady = false;                  // featError allocated and cleared since render_begin (by the first feature or albedo call)
    // the albedo buffer (slrhip_render_albedo): the sums are allocated by the first albedo call after render_begin; the record window is the feature pass's
    DevArray<float> albSums;                      // `components` planes of numPixels floats
    bool albReady = false;                        // sums allocated and cleared since render_begin
    uint32_t albWindow = 0;                       // passes per launch
    uint64_t albPasses = 0;                       // passes accumulated since render_begin
    // per-pixel noise statistics (slrhip_statistics_begin): allocated by the first enabling call, kept for later renders
    DevArray<float4> statRecords;                 // {mean, M2, n, max} per pixel of the shard, updated by k_fold
    DevArray<StatsTotals> statPartials, statTotals;      // the summary's first-stage partials and its result
    bool statsOn = false;                         // this render folds with the statistics instantiation of k_fold
    bool statsClear = false;                      // the records still hold an earlier render's: cleared in stream order before their first use
    // the sample clamp (slrhip_clamp_begin): allocated by the first enabling call, kept for later renders
    DevArray<float4> clampRecords;                // {clamped, dropped (uint32 bits), removed, largest} per pixel of the shard, updated by k_fold
    DevArray<ClampTotals> clampPartials, clampTotals;     // the summary's first-stage partials and its result
    bool clampOn = false;                         // this render folds with the clamp instantiation of k_fold
    bool clampClear = false;                      // as statsClear
    float clampLimit = 0.0f;
    uint32_t clampFlags = 0;
    // adaptive sampling (slrhip_render_adaptive): the list buffers are allocated by the first adaptive call and kept for later renders
    DevArray<uint32_t> adaptXY[2], adaptIndex[2]; // the active list (pt_kernels.h AdaptiveSelect), two pairs that alternate
    DevArray<uint32_t> adaptOffsets, adaptCount;  // the select's workgroup offsets; the new list's length (read back once per block)
    uint32_t activePixels = 0;                    // pixels of the shard not yet retired since render_begin
    int activeList = -1;                          // the pair that holds them; -1: every pixel of the shard (no check has run yet)
    // the denoiser (slrhip_denoise): allocated by the first call and by any call that needs more, never by a render
    DevArray<uint8_t> denoiseScratch;
    PathBuffers buffers;
    uint64_t iterations = 0;
    bool firstRenderCall = true;

    // SLRHIP_FLAG_TIME_KERNELS: 3 events per iteration (before shade, after shade, after trace)
    std::vector<hipEvent_t> events;
    // hipGraph of one block of iterations (slrhip_render): captured on the context's own stream, replayed until no slot is live
    hipStream_t workStream = nullptr;
    hipEvent_t userReady = nullptr;
    uint64_t profLaunches[SLRHIP_KERNEL_COUNT] = {};
    double profMs[SLRHIP_KERNEL_COUNT] = {};
    ~slrhip_ctx() {
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        if (userReady) (void)hipEventDestroy(userReady);
        if (workStream) (void)hipStreamDestroy(workStream);
    }
};

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

// Points a zero-initialised DevScene at the context's scene arrays and assigns it to ctx->scene in one go.
static void bindScene(slrhip_ctx* ctx, const slrhip_scene_desc& d, const PreparedScene& p, uint32_t numNodes, bool quantized) {
    DevScene sc{};
    sc.nodes = reinterpret_cast<const float4*>(ctx->nodes.ptr); sc.numNodes = numNodes;
    sc.nodesQ = quantized ? reinterpret_cast<const float4*>(ctx->nodesQ.ptr) : nullptr;
    sc.nodes8 = p.wide8 ? reinterpret_cast<const float4*>(ctx->nodes8.ptr) : nullptr;
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
    HIP_TRY(hipSetDevice(ctx->device));
    uint32_t numNodes = (uint32_t)p.bvh.nodes.size(), depth = p.bvh.depth;
    uint64_t leafRefs = p.bvh.leafTris.size();
    bool quantized = p.quantized;
    if (p.build == TreeBuild::Device) {
        // the whole geometry on the GPU: tree, quantized nodes, leaf packets, shading records (bvh_device.hip)
        DeviceGeometry g;
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
    }
    else {
        HIP_TRY(ctx->nodes.upload(p.bvh.nodes));
        if (p.quantized) HIP_TRY(ctx->nodesQ.upload(p.bvh.quantized));
        if (p.wide8) HIP_TRY(ctx->nodes8.upload(p.bvh.nodes8));
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
    // the ray queries' error word: allocated here, so that a query call allocates nothing (and can be captured in a graph)
    HIP_TRY(ctx->queryError.alloc(1));
    HIP_TRY(hipMemset(ctx->queryError.ptr, 0, sizeof(uint32_t)));
    bindScene(ctx, d, p, numNodes, quantized);
    ctx->bvhDepth = depth;
    ctx->bvhLeafRefs = leafRefs;
    ctx->haveScene = true;
    return SLRHIP_OK;
}

// Overrides of the render plan, each read once per process (the first two by measurement builds only: tuningEnv).
static long autoStripesOverride() { static const long v = [] { const char* e = tuningEnv("SLRHIP_AUTO_STRIPES"); return e ? atol(e) : 0L; }(); return v; }
static int pairsMask() { static const int v = [] { const char* e = tuningEnv("SLRHIP_PAIRS"); return e ? atoi(e) : kDefaultPairs; }(); return v; }
static uint32_t runLengthOverride() {
    static const uint32_t v = [] { const char* e = getenv("SLRHIP_RUN_LENGTH"); const long n = e ? atol(e) : 0L; return n >= 1 && n <= 4096 ? (uint32_t)n : 0u; }();
    return v;
}

static size_t frameFloats(const RenderParams& rp) { return (size_t)rp.imageWidth * rp.imageHeight * (rp.spectral ? 16 : 3); }

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
    launchTail(ctx->scene, pb, rp, status[S_LIVE], ctx->numCUs, s);
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
        launchShade(ctx->scene, pb, rp, parity, s);
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

// The pixels of a window of slrhip_render_adaptive: a compact list (pt_kernels.h AdaptiveSelect) instead of the shard's.
struct ActiveWindow {
    const uint32_t* xy;           // compact index -> x | y << 16
    const uint32_t* index;        // compact index -> pixel of the shard
    uint32_t count;
};

// One window of passes [sppBegin, sppBegin + sppCount): every sample of the window rendered into the result window, then folded
// into the sensor in pass order.  slrhip_render sizes the windows.  The window runs on its OWN copy of the render parameters and
// the buffer table: ctx->params and ctx->buffers stay the shard's (the resolves, the statistics, the feature passes and
// slrhip_camera_rays read them).  `active` (slrhip_render_adaptive): the window is over that list — its length as the pixel count, its
// xy as the pixel list, its index as the map of the fold; the slots, the queues' owners and the tail bound stay the shard's.
static ClampParams clampParams(const slrhip_ctx* ctx) { return ClampParams{ctx->clampOn ? ctx->clampRecords.ptr : nullptr, ctx->clampLimit, ctx->clampFlags}; }

static int renderWindow(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, hipStream_t stream, const ActiveWindow* active = nullptr) {
    RenderParams rp = ctx->params;
    PathBuffers pb = ctx->buffers;
    if (active) { rp.numPixels = active->count; pb.pixelXY = active->xy; }
    const WindowPlan window = planWindow(rp.numPixels, sppCount, runLengthOverride());
    rp.sppBegin = sppBegin; rp.sppCount = sppCount;
    rp.workItems = window.workItems; rp.runLength = window.runLength; rp.numRuns = window.numRuns;
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
                             tailKernelAvailable(ctx->scene, rp.spectral != 0) && !counting);

    const bool timeKernels = (ctx->config.flags & SLRHIP_FLAG_TIME_KERNELS) != 0;
    if (timeKernels && ctx->events.empty()) {
        ctx->events.resize((size_t)kCheckEvery * kEventsPerIteration);
        for (hipEvent_t& e : ctx->events) HIP_TRY(hipEventCreate(&e));
    }
    static const char* iterLogPath = getenv("SLRHIP_ITER_LOG");
    std::vector<IterationTimes> iterLog;

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
        (void)launchBlock(ctx, pb, rp, traceBlocks, false, s);
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
    launchCountSamples(pb, rp, s);       // samples rendered in this window, counted on the device (T_SAMPLES)
    const ClampParams clamp = clampParams(ctx);                                          // slrhip_clamp_begin: every sample through the clamp first
    if (active) launchFoldIndexed(pb, rp, ctx->statRecords.ptr, active->index, clamp, s);       // the same, scattered to the list's pixels of the shard
    else launchFold(pb, rp, ctx->statsOn ? ctx->statRecords.ptr : nullptr, clamp, s);       // sensor->add, in pass order (+ the noise records)
    HIP_TRY(hipGetLastError());
    const int rc = checkWindow(ctx, rp.workItems, s);
    if (rc == SLRHIP_OK && iterLogPath) writeIterationLog(iterLogPath, rp, iterLog);
    return rc;
}

// The noise records of an earlier render are cleared before their first use in this one, in order on the stream of that use.
static int clearStatistics(slrhip_ctx* ctx, hipStream_t stream) {
    if (ctx->clampOn && ctx->clampClear) {         // ... and the clamp records, which every statistics-aware call may touch as well
        HIP_TRY(hipMemsetAsync(ctx->clampRecords.ptr, 0, std::max<size_t>(ctx->params.numPixels, 1u) * sizeof(float4), stream));
        ctx->clampClear = false;
    }
    if (!ctx->statsOn || !ctx->statsClear) return SLRHIP_OK;
    HIP_TRY(hipMemsetAsync(ctx->statRecords.ptr, 0, std::max<size_t>(ctx->params.numPixels, 1u) * sizeof(float4), stream));
    ctx->statsClear = false;
    return SLRHIP_OK;
}

// the result window's budget (render_plan.cpp, planWindows): 16 GiB by default, SLRHIP_RESULT_WINDOW_MB overrides
static uint64_t resultWindowBudget() {
    uint64_t budget = 16ull << 30;
    if (const char* e = getenv("SLRHIP_RESULT_WINDOW_MB")) { const long mb = atol(e); if (mb > 0) budget = (uint64_t)mb << 20; }
    return budget;
}

static_assert(sizeof(StatsTotals) == sizeof(struct slrhip_statistics_summary) && offsetof(StatsTotals, sumVarianceOfMean) == offsetof(struct slrhip_statistics_summary, sum_variance_of_mean) &&
              offsetof(StatsTotals, maxSample) == offsetof(struct slrhip_statistics_summary, max_sample), "StatsTotals is slrhip_statistics_summary's layout");
static_assert(sizeof(ClampTotals) == sizeof(struct slrhip_clamp_summary) && offsetof(ClampTotals, removed) == offsetof(struct slrhip_clamp_summary, removed) &&
              offsetof(ClampTotals, largest) == offsetof(struct slrhip_clamp_summary, largest), "ClampTotals is slrhip_clamp_summary's layout");
static_assert(kClampDropNonFinite == SLRHIP_CLAMP_DROP_NONFINITE, "pt_clamp.h's flag is the ABI's");

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
    rp.numSlots = plan.numSlots; rp.numBlocks = rp.numSlots / 256u; rp.numWaves = rp.numSlots / 64u;
    rp.numPixels = plan.numPixels; rp.stripes = plan.stripes;
    rp.runLength = 1;                                     // the window's passes, runs and tail bound: renderWindow
    rp.rngSeed = st->rng_seed; rp.timeStart = st->time_start; rp.timeEnd = st->time_end;
    rp.imageWidth = plan.width; rp.imageHeight = plan.height;
    rp.countSlots = (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) ? 1u : 0u;
    rp.shardCapacity = plan.shardCapacity;
    rp.spectral = spectral ? 1u : 0u;
    rp.injectError = (ctx->config.flags & SLRHIP_FLAG_TEST_DEVICE_ERROR) ? 1u : 0u;
    ctx->params = rp;
    ctx->settings = *st;
    ctx->shard = shard;
    ctx->iterations = 0;
    ctx->firstRenderCall = true;
    ctx->featReady = false; ctx->featChannels = 0; ctx->featPassEnd = 0;      // the feature accumulation restarts (its arrays are kept for reuse)
    ctx->featErrorReady = false; ctx->albReady = false; ctx->albPasses = 0;   // ... and the albedo accumulation and the error word they share
    ctx->statsOn = false; ctx->statsClear = true;                             // statistics are per render (slrhip_statistics_begin); the records are kept, stale
    ctx->clampOn = false; ctx->clampClear = true;                             // ... and so is the clamp (slrhip_clamp_begin)
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
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    int rc = slrhip_resolve_framebuffer(ctx, ctx->resolveScratch.ptr, need, nullptr);
    if (rc != SLRHIP_OK) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
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

// Ray queries on device memory (slrhip_intersect_rays / slrhip_test_visibility): the render's wave-specialised traversal fed from
// the caller's ray array (pt_trace_ws.hip, k_query_ws).  Stream-ordered; no allocation, no copy, no host synchronisation: the
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

// ---- first-hit feature buffers (slrhip_render_features / slrhip_resolve_features / slrhip_camera_rays) -------------------------
static const uint64_t kFeatureRecordBytes = 512ull << 20;      // the record window: 16 B per (pixel, pass), 20 B with a vector channel
static const uint32_t kFeatureVectors = SLRHIP_FEATURE_GEOMETRIC_NORMAL | SLRHIP_FEATURE_SHADING_NORMAL | SLRHIP_FEATURE_SHADING_TANGENT;

static FeatureParams featureParams(const slrhip_ctx* ctx, uint32_t channels, uint32_t passBegin, uint32_t numPasses) {
    const RenderParams& rp = ctx->params;
    FeatureParams fp{};
    fp.pixelXY = ctx->pixelXY.ptr; fp.records = ctx->featRecords.ptr; fp.b2 = (channels & (kFeatureVectors & ~SLRHIP_FEATURE_GEOMETRIC_NORMAL)) ? ctx->featB2.ptr : nullptr; fp.errorWord = ctx->featError.ptr;
    fp.numPixels = rp.numPixels; fp.numPasses = numPasses; fp.passBegin = passBegin; fp.channels = channels;
    fp.rngSeed = rp.rngSeed; fp.timeStart = rp.timeStart; fp.timeEnd = rp.timeEnd;
    fp.imageWidth = rp.imageWidth; fp.imageHeight = rp.imageHeight;
    return fp;
}
// The error word the feature and the albedo passes share: allocated and cleared, in stream order, by whichever runs first after a
// slrhip_render_begin; sticky until the next one.
static int clearFeatureError(slrhip_ctx* ctx, hipStream_t s) {
    if (ctx->featErrorReady) return SLRHIP_OK;
    HIP_TRY(ctx->featError.alloc(1));
    HIP_TRY(hipMemsetAsync(ctx->featError.ptr, 0, sizeof(uint32_t), s));
    ctx->featErrorReady = true;
    return SLRHIP_OK;
}
static FeatureSums featureSums(const slrhip_ctx* ctx) { return FeatureSums{ctx->featGeometric.ptr, ctx->featShading.ptr, ctx->featTangent.ptr, ctx->featIds.ptr}; }

int slrhip_render_features(slrhip_ctx* ctx, uint32_t channels, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render_features: call slrhip_render_begin first");
    if (channels == 0 || (channels & ~SLRHIP_FEATURE_ALL)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: no or unknown channel bits");
    if ((uint64_t)sppBegin + sppCount > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: pass range beyond 2^32");
    if (sppCount == 0) return SLRHIP_OK;
    const RenderParams& rp = ctx->params;
    // one channel set between two slrhip_render_begin calls: every channel then sums over the same passes (sum / COVERAGE is a mean)
    if (ctx->featChannels && channels != ctx->featChannels)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: the channel set differs from that of the first feature call since slrhip_render_begin");
    const bool first = ctx->featChannels == 0;
    ctx->featChannels = channels;
    if (rp.numPixels == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (first) {
        // the first feature call since render_begin: the sums (cleared in stream order) and a record window whose size depends on
        // the shard and the channel set alone, so that no later call allocates whatever its pass count
        const size_t pixels = rp.numPixels;
        const bool wantB2 = (channels & (kFeatureVectors & ~SLRHIP_FEATURE_GEOMETRIC_NORMAL)) != 0;
        const uint64_t perPass = (uint64_t)pixels * (sizeof(float4) + (wantB2 ? sizeof(float) : 0));
        ctx->featWindow = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>({kFeatureRecordBytes / perPass, 0x7FFFFFFFull / pixels, 64u}));
        HIP_TRY(ctx->featGeometric.alloc(pixels)); HIP_TRY(ctx->featShading.alloc(pixels)); HIP_TRY(ctx->featTangent.alloc(pixels));
        HIP_TRY(ctx->featIds.alloc(pixels));
        HIP_TRY(ctx->featRecords.alloc(pixels * ctx->featWindow));
        if (wantB2) HIP_TRY(ctx->featB2.alloc(pixels * ctx->featWindow));
        HIP_TRY(hipMemsetAsync(ctx->featGeometric.ptr, 0, pixels * sizeof(float4), s));
        HIP_TRY(hipMemsetAsync(ctx->featShading.ptr, 0, pixels * sizeof(float4), s));
        HIP_TRY(hipMemsetAsync(ctx->featTangent.ptr, 0, pixels * sizeof(float4), s));
        HIP_TRY(hipMemsetAsync(ctx->featIds.ptr, 0xFF, pixels * sizeof(uint4), s));
        if (const int rc = clearFeatureError(ctx, s)) return rc;
        ctx->featReady = true;
    }
    const FeatureSums sums = featureSums(ctx);
    for (uint32_t done = 0; done < sppCount; done += ctx->featWindow) {
        const uint32_t n = std::min(ctx->featWindow, sppCount - done);
        // the pixels keep the ids of the highest pass rendered so far
        const uint64_t end = (uint64_t)sppBegin + done + n;
        const uint32_t idsPass = end >= ctx->featPassEnd ? n - 1u : 0xFFFFFFFFu;
        ctx->featPassEnd = std::max(ctx->featPassEnd, end);
        launchFeatures(ctx->scene, featureParams(ctx, channels, sppBegin + done, n), sums, idsPass, ctx->numCUs, s);
    }
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_resolve_features(slrhip_ctx* ctx, uint32_t channel, void* deviceDst, size_t numElements, void* streamPtr) {
    if (!ctx || !deviceDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: null argument");
    if ((uintptr_t)deviceDst & 3u) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: misaligned pointer (4 bytes)");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_resolve_features: call slrhip_render_begin first");
    if (channel == 0 || (channel & (channel - 1u)) || (channel & ~SLRHIP_FEATURE_ALL))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: `channel` must be one SLRHIP_FEATURE_* bit");
    if (!(ctx->featChannels & channel))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: no slrhip_render_features call since slrhip_render_begin asked for this channel");
    const RenderParams& rp = ctx->params;
    const size_t k = (channel & (SLRHIP_FEATURE_DISTANCE | SLRHIP_FEATURE_COVERAGE)) ? 1u : 3u;
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight * k;
    if (numElements < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemsetAsync(deviceDst, channel == SLRHIP_FEATURE_IDS ? 0xFF : 0, need * sizeof(uint32_t), s));
    if (rp.numPixels) launchFeatureResolve(featureParams(ctx, channel, 0, 0), featureSums(ctx), channel, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_features(slrhip_ctx* ctx, uint32_t channel, void* hostDst, size_t numElements) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_features: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_read_features: call slrhip_render_begin first");
    const size_t need = (size_t)ctx->params.imageWidth * ctx->params.imageHeight * 3u;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    HIP_TRY(hipDeviceSynchronize());                   // feature passes queued on any stream of the caller's
    int rc = slrhip_resolve_features(ctx, channel, ctx->resolveScratch.ptr, numElements, nullptr);
    if (rc != SLRHIP_OK) return rc;
    uint32_t bits = 0;
    if ((rc = slrhip_features_status(ctx, &bits, nullptr)) != SLRHIP_OK) return rc;
    if (bits) return fail(SLRHIP_ERR_HIP, "slrhip_read_features: the feature error word is set (a traversal gave up): " + std::to_string(bits));
    const size_t k = (channel & (SLRHIP_FEATURE_DISTANCE | SLRHIP_FEATURE_COVERAGE)) ? 1u : 3u;
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need / 3u * k * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

int slrhip_camera_rays(slrhip_ctx* ctx, uint32_t pass, slrhip_ray* rays, uint32_t* pixelXY, uint32_t capacity, uint32_t* count, void* streamPtr) {
    if (!ctx || !count) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: null context or count");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_camera_rays: call slrhip_render_begin first");
    const RenderParams& rp = ctx->params;
    *count = rp.numPixels;
    if (rp.numPixels == 0 || (!rays && !pixelXY && capacity == 0)) return SLRHIP_OK;          // the count alone
    if (!rays) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: null ray pointer");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)pixelXY & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: misaligned pointer (rays: 16 bytes; pixel_xy: 4)");
    if (capacity < rp.numPixels)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: capacity " + std::to_string(capacity) + " is smaller than the shard's " + std::to_string(rp.numPixels) + " pixels");
    HIP_TRY(hipSetDevice(ctx->device));
    launchCameraRays(ctx->scene, featureParams(ctx, 0, pass, 1), reinterpret_cast<float4*>(rays), pixelXY, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_features_status(slrhip_ctx* ctx, uint32_t* bits, void* stream) {
    if (!ctx || !bits) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_features_status: null argument");
    *bits = 0;
    if (!ctx->haveRender || !ctx->featErrorReady) return SLRHIP_OK;     // no feature or albedo pass can have run
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(bits, ctx->featError.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SLRHIP_OK;
}

// ---- the albedo buffer (slrhip_render_albedo / slrhip_resolve_albedo / slrhip_read_albedo) -----------------------------------------
// The traversal and the record window are the feature pass's; the fold and the sums are pt_albedo.hip's.
int slrhip_render_albedo(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_albedo: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render_albedo: call slrhip_render_begin first");
    if ((uint64_t)sppBegin + sppCount > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_albedo: pass range beyond 2^32");
    if (sppCount == 0) return SLRHIP_OK;
    const RenderParams& rp = ctx->params;
    if (rp.numPixels == 0) { ctx->albPasses += sppCount; return SLRHIP_OK; }
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    const bool wantB2 = ctx->scene.numTextures != 0;                 // the texture coordinate needs both barycentrics
    const uint32_t components = rp.spectral ? SLRHIP_SPECTRAL_COMPONENTS : SLRHIP_RGB_COMPONENTS;
    if (!ctx->albReady) {
        // the first albedo call since render_begin: the sums (cleared in stream order) and room in the record window, sized by the
        // shard and the scene alone, so that no later call allocates whatever its pass count.  The window's arrays only ever grow:
        // a feature call that sized them for more passes keeps its room.  Growing MOVES them (DevArray::alloc frees and allocates),
        // here and in the first feature call alike: graphs are captured after both first calls (include/slrhip.h).
        const size_t pixels = rp.numPixels;
        const uint64_t perPass = (uint64_t)pixels * (sizeof(float4) + (wantB2 ? sizeof(float) : 0));
        ctx->albWindow = (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>({kFeatureRecordBytes / perPass, 0x7FFFFFFFull / pixels, 64u}));
        HIP_TRY(ctx->albSums.alloc(pixels * components));
        HIP_TRY(ctx->featRecords.alloc(std::max(ctx->featRecords.capacity, pixels * ctx->albWindow)));
        if (wantB2) HIP_TRY(ctx->featB2.alloc(std::max(ctx->featB2.capacity, pixels * ctx->albWindow)));
        HIP_TRY(hipMemsetAsync(ctx->albSums.ptr, 0, pixels * components * sizeof(float), s));
        if (const int rc = clearFeatureError(ctx, s)) return rc;
        ctx->albReady = true;
    }
    for (uint32_t done = 0; done < sppCount; done += ctx->albWindow) {
        const uint32_t n = std::min(ctx->albWindow, sppCount - done);
        FeatureParams fp = featureParams(ctx, 0, sppBegin + done, n);
        fp.b2 = wantB2 ? ctx->featB2.ptr : nullptr;
        launchFeatureTrace(ctx->scene, fp, ctx->numCUs, s);
        launchAlbedoFold(ctx->scene, fp, rp.spectral != 0, ctx->albSums.ptr, s);
    }
    ctx->albPasses += sppCount;
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_resolve_albedo(slrhip_ctx* ctx, float* deviceDst, size_t numFloats, uint32_t* passes, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_albedo: null context");
    if (!deviceDst || ((uintptr_t)deviceDst & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_albedo: null or misaligned destination (4 bytes)");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_resolve_albedo: call slrhip_render_begin first");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_albedo: destination too small");
    if (passes) *passes = (uint32_t)std::min<uint64_t>(ctx->albPasses, 0xFFFFFFFFull);
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), s));
    if (rp.numPixels && ctx->albReady)
        launchAlbedoResolve(featureParams(ctx, 0, 0, 0), rp.spectral ? SLRHIP_SPECTRAL_COMPONENTS : SLRHIP_RGB_COMPONENTS, ctx->albSums.ptr, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_albedo(slrhip_ctx* ctx, float* hostDst, size_t numFloats, uint32_t* passes) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_albedo: null context");
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_albedo: null destination");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_read_albedo: call slrhip_render_begin first");
    const size_t need = frameFloats(ctx->params);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_albedo: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    HIP_TRY(hipDeviceSynchronize());                   // albedo passes queued on any stream of the caller's
    if (const int rc = slrhip_resolve_albedo(ctx, ctx->resolveScratch.ptr, need, passes, nullptr)) return rc;
    uint32_t bits = 0;
    if (const int rc = slrhip_features_status(ctx, &bits, nullptr)) return rc;
    if (bits) return fail(SLRHIP_ERR_HIP, "slrhip_read_albedo: the feature error word is set (a traversal gave up): " + std::to_string(bits));
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

// ---- per-pixel noise statistics (slrhip_statistics_begin / slrhip_resolve_statistics / slrhip_statistics_summary / slrhip_render_until) ----
int slrhip_statistics_begin(slrhip_ctx* ctx) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_statistics_begin: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_statistics_begin: call slrhip_render_begin first");
    if (!ctx->firstRenderCall) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_statistics_begin: this render has begun (call it before the first slrhip_render after slrhip_render_begin)");
    if (ctx->statsOn) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t pixels = ctx->params.numPixels;
    hipError_t e = ctx->statRecords.alloc(pixels);
    if (e == hipSuccess) e = ctx->statPartials.alloc(statsSummaryBlocks(pixels));
    if (e == hipSuccess) e = ctx->statTotals.alloc(1);
    if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_statistics_begin: allocating the records: ") + hipGetErrorString(e));
    ctx->statsOn = true; ctx->statsClear = true;
    return SLRHIP_OK;
}

static int checkStatistics(slrhip_ctx* ctx, const char* what) {
    const std::string w(what);
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, w + ": call slrhip_render_begin first");
    if (!ctx->statsOn) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": statistics are off (slrhip_statistics_begin after slrhip_render_begin switches them on)");
    return SLRHIP_OK;
}

int slrhip_resolve_statistics(slrhip_ctx* ctx, uint32_t channel, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (const int rc = checkStatistics(ctx, "slrhip_resolve_statistics")) return rc;
    if (channel == 0 || (channel & (channel - 1u)) || (channel & ~SLRHIP_STATISTICS_ALL))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_statistics: `channel` must be one SLRHIP_STATISTICS_* bit");
    if (!deviceDst || ((uintptr_t)deviceDst & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_statistics: null or misaligned destination (4 bytes)");
    const RenderParams& rp = ctx->params;
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight;
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_statistics: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, s)) return rc;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), s));
    launchStatsResolve(ctx->statRecords.ptr, ctx->pixelXY.ptr, rp.numPixels, rp.imageWidth, channel, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_statistics(slrhip_ctx* ctx, uint32_t channel, float* hostDst, size_t numFloats) {
    if (const int rc = checkStatistics(ctx, "slrhip_read_statistics")) return rc;
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_statistics: null destination");
    const size_t need = (size_t)ctx->params.imageWidth * ctx->params.imageHeight;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    HIP_TRY(hipDeviceSynchronize());                   // renders queued on any stream of the caller's
    if (const int rc = slrhip_resolve_statistics(ctx, channel, ctx->resolveScratch.ptr, numFloats, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

int slrhip_statistics_summary(slrhip_ctx* ctx, struct slrhip_statistics_summary* hostOut, void* streamPtr) {
    if (const int rc = checkStatistics(ctx, "slrhip_statistics_summary")) return rc;
    if (!hostOut) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_statistics_summary: null destination");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, s)) return rc;
    launchStatsSummary(ctx->statRecords.ptr, ctx->params.numPixels, ctx->statPartials.ptr, ctx->statTotals.ptr, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hostOut, ctx->statTotals.ptr, sizeof(*hostOut), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    hostOut->reserved = 0;
    return SLRHIP_OK;
}

// The stop check of slrhip_render_until: the metric of a summary, in double.
static double noiseMetric(const struct slrhip_statistics_summary& t, uint32_t metric) {
    if (t.pixels == 0) return 0.0;                     // an empty shard has no noise
    const double rmse = std::sqrt(t.sum_variance_of_mean / (double)t.pixels);
    if (metric == SLRHIP_NOISE_RMSE) return rmse;
    const double mean = t.sum_mean / (double)t.pixels;
    return mean == 0.0 ? INFINITY : rmse / mean;
}

int slrhip_render_until(slrhip_ctx* ctx, uint32_t sppBegin, const slrhip_noise_target* target, uint32_t* sppDone, struct slrhip_statistics_summary* last,
                        void* stream) {
    if (sppDone) *sppDone = 0;
    if (const int rc = checkStatistics(ctx, "slrhip_render_until")) return rc;
    if (!target || !sppDone) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: null argument");
    if (target->spp_step == 0 || target->spp_max == 0) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: spp_step and spp_max must be positive");
    if (target->metric != SLRHIP_NOISE_RMSE && target->metric != SLRHIP_NOISE_RELATIVE) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: unknown metric");
    if (std::isnan(target->target)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: the target is NaN");
    if ((uint64_t)sppBegin + target->spp_max > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: pass range beyond 2^32");
    struct slrhip_statistics_summary totals;
    std::memset(&totals, 0, sizeof(totals));
    for (uint32_t done = 0; done < target->spp_max;) {
        const uint32_t n = std::min(target->spp_step, target->spp_max - done);
        if (const int rc = slrhip_render(ctx, sppBegin + done, n, stream)) return rc;
        done += n;
        *sppDone = done;
        if (const int rc = slrhip_statistics_summary(ctx, &totals, stream)) return rc;
        if (last) *last = totals;
        // "at least 2 passes": the variance of one sample is not defined (the channels are 0 then, which would read as "no noise")
        if (totals.samples >= 2 * totals.pixels && noiseMetric(totals, target->metric) <= (double)target->target) break;
    }
    return SLRHIP_OK;
}

// ---- the sample clamp (slrhip_clamp_begin / slrhip_resolve_clamp / slrhip_clamp_summary; the rule: pt_clamp.h) ----
int slrhip_clamp_begin(slrhip_ctx* ctx, const slrhip_clamp_desc* d) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_clamp_begin: call slrhip_render_begin first");
    if (!ctx->firstRenderCall) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: this render has begun (call it before the first slrhip_render after slrhip_render_begin)");
    if (!(d->limit > 0.0f)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: the limit must be > 0 (and not NaN); INFINITY clamps nothing");
    if (d->flags & ~SLRHIP_CLAMP_DROP_NONFINITE) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: unknown flag bits");
    if (d->reserved[0] || d->reserved[1]) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: reserved must be 0");
    if (!ctx->clampOn) {
        HIP_TRY(hipSetDevice(ctx->device));
        const uint32_t pixels = ctx->params.numPixels;
        hipError_t e = ctx->clampRecords.alloc(pixels);
        if (e == hipSuccess) e = ctx->clampPartials.alloc(statsSummaryBlocks(pixels));
        if (e == hipSuccess) e = ctx->clampTotals.alloc(1);
        if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_clamp_begin: allocating the records: ") + hipGetErrorString(e));
    }
    ctx->clampLimit = d->limit; ctx->clampFlags = d->flags;
    ctx->clampOn = true; ctx->clampClear = true;
    return SLRHIP_OK;
}

static int checkClamp(slrhip_ctx* ctx, const char* what) {
    const std::string w(what);
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, w + ": call slrhip_render_begin first");
    if (!ctx->clampOn) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": the clamp is off (slrhip_clamp_begin after slrhip_render_begin switches it on)");
    return SLRHIP_OK;
}

int slrhip_resolve_clamp(slrhip_ctx* ctx, uint32_t channel, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (const int rc = checkClamp(ctx, "slrhip_resolve_clamp")) return rc;
    if (channel == 0 || (channel & (channel - 1u)) || (channel & ~SLRHIP_CLAMP_ALL))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_clamp: `channel` must be one SLRHIP_CLAMP_* bit");
    if (!deviceDst || ((uintptr_t)deviceDst & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_clamp: null or misaligned destination (4 bytes)");
    const RenderParams& rp = ctx->params;
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight;
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_clamp: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, s)) return rc;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), s));
    launchClampResolve(ctx->clampRecords.ptr, ctx->pixelXY.ptr, rp.numPixels, rp.imageWidth, channel, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_clamp(slrhip_ctx* ctx, uint32_t channel, float* hostDst, size_t numFloats) {
    if (const int rc = checkClamp(ctx, "slrhip_read_clamp")) return rc;
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_clamp: null destination");
    const size_t need = (size_t)ctx->params.imageWidth * ctx->params.imageHeight;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    HIP_TRY(hipDeviceSynchronize());                   // renders queued on any stream of the caller's
    if (const int rc = slrhip_resolve_clamp(ctx, channel, ctx->resolveScratch.ptr, numFloats, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

int slrhip_clamp_summary(slrhip_ctx* ctx, struct slrhip_clamp_summary* hostOut, void* streamPtr) {
    if (const int rc = checkClamp(ctx, "slrhip_clamp_summary")) return rc;
    if (!hostOut) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_summary: null destination");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, s)) return rc;
    launchClampSummary(ctx->clampRecords.ptr, ctx->params.numPixels, ctx->clampPartials.ptr, ctx->clampTotals.ptr, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hostOut, ctx->clampTotals.ptr, sizeof(*hostOut), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    hostOut->reserved = 0;
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
            float4* dst = window.data() + (size_t)p * elems + (size_t)i * planes;
            if (rp.spectral) for (uint32_t q = 0; q < 4; ++q) dst[q] = make_float4(src[4 * q], src[4 * q + 1], src[4 * q + 2], src[4 * q + 3]);
            else dst[0] = make_float4(src[0], src[1], src[2], 0.0f);
        }
    HIP_TRY(ctx->results.alloc(window.size()));
    ctx->buffers.results = ctx->results.ptr;
    HIP_TRY(hipMemcpy(ctx->results.ptr, window.data(), window.size() * sizeof(float4), hipMemcpyHostToDevice));
    rp.sppBegin = 0; rp.sppCount = passes;
    launchFold(ctx->buffers, rp, ctx->statsOn ? ctx->statRecords.ptr : nullptr, clampParams(ctx), nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SLRHIP_OK;
}

// ---- adaptive sampling (slrhip_render_adaptive / slrhip_resolve_framebuffer_mean / slrhip_adaptive_active) ----
// The retirement check after a block: the next active list from the current one (pt_adaptive.hip), its length read back.
static int adaptiveSelect(slrhip_ctx* ctx, const slrhip_adaptive_target& target, hipStream_t stream) {
    const int next = ctx->activeList < 0 ? 0 : ctx->activeList ^ 1;
    AdaptiveSelect a{};
    a.records = ctx->statRecords.ptr; a.shardXY = ctx->pixelXY.ptr;
    a.prevIndex = ctx->activeList < 0 ? nullptr : ctx->adaptIndex[ctx->activeList].ptr; a.prevCount = ctx->activePixels;
    a.nextXY = ctx->adaptXY[next].ptr; a.nextIndex = ctx->adaptIndex[next].ptr;
    a.blockOffsets = ctx->adaptOffsets.ptr; a.countWord = ctx->adaptCount.ptr;
    a.threshold = target.threshold; a.floor = target.floor;
    launchAdaptiveSelect(a, stream);
    HIP_TRY(hipGetLastError());
    uint32_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, ctx->adaptCount.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (count > ctx->activePixels) return fail(SLRHIP_ERR_HIP, "slrhip_render_adaptive: the active list grew from " + std::to_string(ctx->activePixels) + " to " + std::to_string(count) + " pixels (internal error)");
    ctx->activePixels = count; ctx->activeList = next;
    return SLRHIP_OK;
}

int slrhip_render_adaptive(slrhip_ctx* ctx, uint32_t sppBegin, const slrhip_adaptive_target* target, uint32_t* sppDone, uint64_t* samplesDone,
                           void* streamPtr) {
    if (sppDone) *sppDone = 0;
    if (samplesDone) *samplesDone = 0;
    if (const int rc = checkStatistics(ctx, "slrhip_render_adaptive")) return rc;
    if (!target || !sppDone) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: null argument");
    if (!(target->threshold >= 0.0f) || !(target->floor >= 0.0f)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: threshold and floor must be >= 0 (and not NaN)");
    if (target->spp_min < 2 || target->spp_step == 0 || target->spp_max < target->spp_min)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: need spp_min >= 2, spp_step >= 1 and spp_max >= spp_min");
    if ((uint64_t)sppBegin + target->spp_max > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: pass range beyond 2^32");
    const RenderParams& shard = ctx->params;
    if (shard.numSlots == 0 || ctx->activePixels == 0) return SLRHIP_OK;        // an empty shard, or every pixel has retired
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2; ++k) {
            if (e == hipSuccess) e = ctx->adaptXY[k].alloc(shard.numPixels);
            if (e == hipSuccess) e = ctx->adaptIndex[k].alloc(shard.numPixels);
        }
        if (e == hipSuccess) e = ctx->adaptOffsets.alloc(adaptiveSelectBlocks(shard.numPixels));
        if (e == hipSuccess) e = ctx->adaptCount.alloc(1);
        if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_render_adaptive: allocating the active lists: ") + hipGetErrorString(e));
    }
    if (const int rc = clearStatistics(ctx, stream)) return rc;
    const uint64_t budget = resultWindowBudget();
    uint32_t done = 0;
    while (ctx->activePixels > 0) {
        const uint32_t block = adaptiveBlock(target->spp_min, target->spp_step, target->spp_max, done);
        if (block == 0) break;                                                   // spp_max passes have been handed out
        // the block as the windows of an ordinary call of `block` passes over the active pixels
        ActiveWindow list{};
        const bool compact = ctx->activeList >= 0;
        if (compact) { list.xy = ctx->adaptXY[ctx->activeList].ptr; list.index = ctx->adaptIndex[ctx->activeList].ptr; list.count = ctx->activePixels; }
        const uint32_t window = planWindows(ctx->activePixels, shard.spectral != 0, block, budget);
        HIP_TRY(ctx->results.alloc((size_t)window * ctx->activePixels * (shard.spectral ? 4u : 1u)));
        ctx->buffers.results = ctx->results.ptr;
        for (uint32_t w = 0; w < block; w += window) {
            const uint32_t passes = std::min(window, block - w);
            if (const int rc = renderWindow(ctx, sppBegin + done + w, passes, stream, compact ? &list : nullptr)) return rc;
            if (samplesDone) *samplesDone += (uint64_t)ctx->activePixels * passes;
        }
        done += block;
        *sppDone = done;
        if (const int rc = adaptiveSelect(ctx, *target, stream)) return rc;
    }
    return SLRHIP_OK;
}

int slrhip_resolve_framebuffer_mean(slrhip_ctx* ctx, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (const int rc = checkStatistics(ctx, "slrhip_resolve_framebuffer_mean")) return rc;
    if (!deviceDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_framebuffer_mean: null argument");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_framebuffer_mean: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, stream)) return rc;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), stream));
    launchResolveMean(ctx->buffers, rp, ctx->statRecords.ptr, deviceDst, stream);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_framebuffer_mean(slrhip_ctx* ctx, float* hostDst, size_t numFloats) {
    if (const int rc = checkStatistics(ctx, "slrhip_read_framebuffer_mean")) return rc;
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_framebuffer_mean: null argument");
    const size_t need = frameFloats(ctx->params);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_framebuffer_mean: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(need));
    HIP_TRY(hipDeviceSynchronize());                   // renders queued on any stream of the caller's
    if (const int rc = slrhip_resolve_framebuffer_mean(ctx, ctx->resolveScratch.ptr, need, nullptr)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

int slrhip_adaptive_active(slrhip_ctx* ctx, uint32_t* hostCount, void*) {
    if (!ctx || !hostCount) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_adaptive_active: null argument");
    *hostCount = 0;
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_adaptive_active: call slrhip_render_begin first");
    *hostCount = ctx->activePixels;
    return SLRHIP_OK;
}

// The denoiser: argument checks, the scratch, the launch list (pt_denoise.hip).  It reads nothing of the render state.
int slrhip_denoise(slrhip_ctx* ctx, const slrhip_denoise_desc* d, void* streamPtr) {
    const auto refuse = [](const char* what) { return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_denoise: ") + what); };
    if (!ctx || !d) return refuse("null argument");
    if (d->reserved != 0) return refuse("reserved must be 0");
    if (d->components != 3 && d->components != 16) return refuse("components must be 3 or 16");
    if (d->iterations < 1 || d->iterations > 8) return refuse("iterations must be 1 .. 8");
    if (d->normal_power_log2 > 7) return refuse("normal_power_log2 must be 0 .. 7");
    if (d->sigma_luminance != d->sigma_luminance || d->sigma_distance != d->sigma_distance) return refuse("a sigma is NaN");
    const DenoiseScratch scratch = denoiseScratch(d->width, d->height, d->components);
    if (scratch.bytes == 0) return refuse("width and height must be >= 1 and width * height < 2^31");
    if (!d->color || !d->output) return refuse("null color or output");
    const size_t pixels = (size_t)d->width * d->height, plane = pixels * sizeof(float), frame = plane * d->components;
    struct Range { const void* p; size_t bytes; };
    const Range inputs[5] = {{d->color, frame}, {d->variance, plane}, {d->normal, 3 * plane}, {d->distance, plane}, {d->coverage, plane}};
    const Range outputs[2] = {{d->output, frame}, {d->output_variance, plane}};
    for (const Range& r : inputs) if ((uintptr_t)r.p & 3u) return refuse("a misaligned pointer (4 bytes)");
    for (const Range& r : outputs) if ((uintptr_t)r.p & 3u) return refuse("a misaligned pointer (4 bytes)");
    if ((d->normal || d->distance) && !d->coverage) return refuse("normal and distance need coverage");
    for (const Range& o : outputs)
        for (const Range& in : inputs)
            if (o.p && in.p && rangesOverlap(o.p, o.bytes, in.p, in.bytes)) return refuse("an output overlaps an input");
    if (d->output_variance && rangesOverlap(d->output, frame, d->output_variance, plane)) return refuse("output and output_variance overlap");

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

// Diagnostic (include/slrhip_debug.h): the argument checks of slrhip_modulate alone.
int slrhip_debug_modulate_check(const slrhip_modulate_desc* d) {
    if (!d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_modulate: null argument");
    if (const char* what = modulateRefusal(*d)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string("slrhip_modulate: ") + what);
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
