// slrhip_api.hip — the C ABI of include/slrhip.h over the HIP kernels.
//
// A scene is checked and flattened on the host by scene_prep.cpp, then committed here: the device tree build (if chosen),
// the uploads, the DevScene.  PathTracingRenderer::render's set-up (Renderers/PathTracingRenderer.cpp:27-70) lives here too:
// render_begin sizes the path state, render drives the wavefront iterations.
// There is no CPU fallback: without a HIP device every entry point fails loudly.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/slrhip.h"
#include "bvh.h"
#include "pt_kernels.h"
#include "scene_prep.h"

using namespace slrhip;

namespace {

const int kDefaultPairs = 1;                   // SLRHIP_PAIRS: the ray pair pays, the radiance-sum pair does not
const uint32_t kStatusWords = 8;               // PathBuffers::activeSlots .. tailWords: one small array, read back in one copy
const uint32_t kDefaultRunLength = 64;         // SLRHIP_RUN_LENGTH: passes of a pixel a wave takes in a row (pt_kernels.h WorkItem; measured: DESIGN.md)
#ifndef SLR_TAIL_DIVISOR
#define SLR_TAIL_DIVISOR 8u      // the tail kernel never takes more than this fraction of the slots (1u in a variant build: the tail kernel as the whole renderer, measured in DESIGN.md)
#endif
const uint32_t kDefaultTailSlots = 1u << 18;   // SLRHIP_TAIL_SLOTS: measured on the headline frame and its N = 8 shard

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
    if (st->image_width <= 0 || st->image_height <= 0 || st->image_width > 65535 || st->image_height > 65535)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_begin: image size out of range");
    if (shard.shard_count == 0 || shard.shard_index >= shard.shard_count)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_begin: bad shard");
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t W = (uint32_t)st->image_width, H = (uint32_t)st->image_height;
    const uint32_t tilesX = (W + 7) >> 3, tilesY = (H + 7) >> 3;     // ImageSensor.cpp:43-44, 8x8 tiles
    // pixel list of this shard: tiles t with t % count == index, row-major inside each tile, so 64
    // consecutive slots (one wavefront) are one 8x8 tile
    std::vector<uint32_t> pixels;
    for (uint32_t t = shard.shard_index; t < tilesX * tilesY; t += shard.shard_count) {
        uint32_t tx = t % tilesX, ty = t / tilesX;
        for (uint32_t ly = 0; ly < 8; ++ly)
            for (uint32_t lx = 0; lx < 8; ++lx) {
                uint32_t x = tx * 8 + lx, y = ty * 8 + ly;
                if (x < W && y < H) pixels.push_back(x | (y << 16));
            }
    }
    if (pixels.empty()) pixels.push_back(0xFFFFFFFFu);   // an empty shard keeps the buffers valid; numPixels = 0 below
    const uint32_t numPixels = pixels[0] == 0xFFFFFFFFu ? 0u : (uint32_t)pixels.size();
    uint32_t stripes = ctx->config.stripes;
    if (stripes == 0) {
        // Paths in flight: throughput keeps rising with the slot count (longer launches amortise the per-wave tail of the
        // traversal kernel: 807 / 1146 / 1267 Msamples/s at 0.9 / 3.7 / 7.4 M slots on the 1280x720 Cornell scene in round 1),
        // at ~200 B of HBM per slot; the per-pixel sample pool keeps the stripes of a pixel finishing together, so fewer, fuller
        // iterations keep paying.  The count is a power of two (the stripes of a pixel then fill whole lane groups of the shade
        // workgroup, PathBuffers): the smallest that reaches ~22 M slots in RGB mode, ~7.4 M in spectral mode (492 B per slot; its
        // shade kernel is latency-bound, not launch-bound), at most 64 (the width of the pool's mask; also the best count measured
        // for the eighth of the image a rank owns at N = 8).  Measured with the fused shade kernel, 16 vs 32 stripes at 1280x720
        // (profiles/r03_e_*): Cornell 2 709 vs 2 719, environment light 5 630 vs 6 061, 10 M-triangle grid 1 954 vs 1 981 Msamples/s.
        const uint32_t target = ctx->config.mode == SLRHIP_MODE_SPECTRAL ? 7372800u : 22118400u;
        static const long envStripes = [] { const char* e = tuningEnv("SLRHIP_AUTO_STRIPES"); return e ? atol(e) : 0L; }();      // measurement: force the automatic choice
        stripes = 1u;
        while (stripes < 64u && (uint64_t)numPixels * stripes < target) stripes *= 2u;
        if (numPixels == 0) stripes = 1u;
        if (envStripes >= 1 && envStripes <= 64) stripes = (uint32_t)envStripes;
    }
    // Slots are paths in flight, not places in the image (pt_kernels.h): `stripes` only sizes their number
    const size_t numSlots = std::max<size_t>(((size_t)numPixels * stripes + 255u) / 256u, 1) * 256u;
    if (numSlots > 0x7FFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_begin: too many path slots");

    const bool spectral = ctx->config.mode == SLRHIP_MODE_SPECTRAL;
    const size_t planes = spectral ? 4 : 1;
    HIP_TRY(ctx->pixelXY.upload(pixels));
    // SLRHIP_PAIRS (bit 0: ray origin + direction, bit 1: the path's radiance sum + its compensation, bit 2: sample header + RNG state): the two records of a pair
    // interleaved in one array, one 32-byte sector per slot (PathBuffers::rayStride / spStride)
    static const int envPairs = [] { const char* e = tuningEnv("SLRHIP_PAIRS"); return e ? atoi(e) : kDefaultPairs; }();
    const uint32_t rayStride = (envPairs & 1) ? 2u : 1u, spStride = (envPairs & 2) ? 2u : 1u, hdrStride = (envPairs & 4) ? 2u : 1u;
    HIP_TRY(ctx->rayOrg.alloc(numSlots * rayStride, true)); HIP_TRY(ctx->rayDir.alloc(rayStride == 2 ? 1 : numSlots, true)); HIP_TRY(ctx->hit.alloc(numSlots, true));
    HIP_TRY(ctx->alpha.alloc(numSlots * planes, true)); HIP_TRY(ctx->spR.alloc(numSlots * planes * spStride, true)); HIP_TRY(ctx->spC.alloc(spStride == 2 ? 1 : numSlots * planes, true));
    HIP_TRY(ctx->fbSum.alloc((size_t)std::max(numPixels, 1u) * planes, true)); HIP_TRY(ctx->fbComp.alloc((size_t)std::max(numPixels, 1u) * planes, true));
    HIP_TRY(ctx->nee.alloc(numSlots * planes, true));
    HIP_TRY(ctx->shadowDir.alloc(numSlots, true));
    HIP_TRY(ctx->pdfPrev.alloc(spectral ? numSlots : 1, true));
    HIP_TRY(ctx->hdr.alloc(numSlots * hdrStride, true)); HIP_TRY(ctx->rng.alloc(hdrStride == 2 ? 1 : numSlots, true));
    HIP_TRY(ctx->cursor.alloc(numSlots / 64u)); HIP_TRY(ctx->idleShards.alloc(kShards * kCounterStride));
    HIP_TRY(ctx->flags.alloc(numSlots, true)); HIP_TRY(ctx->visible.alloc(numSlots, true));
    if (ctx->scene.instances) HIP_TRY(ctx->hitInstance.alloc(numSlots, true));
    // queue regions: slot block b appends to region b % kShards, so a region holds at most ceil(numBlocks / kShards) blocks
    const uint32_t numBlocks = (uint32_t)((numSlots + 255) / 256);
    const uint32_t shardCapacity = ((numBlocks + kShards - 1) / kShards) * 256;
    HIP_TRY(ctx->shadowQueue.alloc((size_t)shardCapacity * kShards, true)); HIP_TRY(ctx->tailList.alloc(numSlots, true));
    HIP_TRY(ctx->blockDead.alloc(numBlocks));
    HIP_TRY(ctx->queueCount.alloc(2 * kQueueSetWords)); HIP_TRY(ctx->activeSlots.alloc(kStatusWords));      // [0] live slots, [1] device error word, [2] unused, [3] tail mode (1 + parity), [4..5] tail list length / cursor
    HIP_TRY(ctx->totals.alloc((size_t)T_KINDS * kShards * kTotalStride));
    // The statistics restart here.  A memset of device memory is only ordered on the null stream, and slrhip_render may be
    // given a NON-BLOCKING stream, which the null stream does not wait for and which does not wait for it: the memset has to
    // be complete before this call returns.  (Round 1, gpurun_out/overlap.log: this function also cleared queueCount with a
    // second null-stream memset and did not wait; on a non-blocking stream k_reset_slots — which writes the initial regen
    // counts into queueCount — could run BEFORE that memset landed, the counts were wiped, no slot ever started a sample and
    // slrhip_render ran into its iteration bound.  queueCount is now written by k_reset_slots alone, in stream order.)
    HIP_TRY(hipMemsetAsync(ctx->totals.ptr, 0, ctx->totals.count * sizeof(uint64_t), nullptr));
    HIP_TRY(hipMemsetAsync(ctx->activeSlots.ptr, 0, kStatusWords * sizeof(uint32_t), nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));

    PathBuffers& pb = ctx->buffers;
    pb.rng = hdrStride == 2 ? ctx->hdr.ptr + 1 : ctx->rng.ptr; pb.hdrStride = hdrStride; pb.rayOrg = ctx->rayOrg.ptr; pb.rayDir = rayStride == 2 ? ctx->rayOrg.ptr + 1 : ctx->rayDir.ptr; pb.hit = ctx->hit.ptr;
    pb.rayStride = rayStride; pb.spStride = spStride;
    pb.alpha = ctx->alpha.ptr; pb.spR = ctx->spR.ptr; pb.spC = spStride == 2 ? ctx->spR.ptr + 1 : ctx->spC.ptr; pb.fbSum = ctx->fbSum.ptr; pb.fbComp = ctx->fbComp.ptr; pb.results = ctx->results.ptr; pb.cursor = ctx->cursor.ptr;
    pb.nee = ctx->nee.ptr;
    pb.pdfPrev = spectral ? ctx->pdfPrev.ptr : nullptr; pb.hdr = ctx->hdr.ptr; pb.shadowDir = ctx->shadowDir.ptr; pb.flags = ctx->flags.ptr;
    pb.hitInstance = ctx->scene.instances ? ctx->hitInstance.ptr : nullptr;
    pb.visible = ctx->visible.ptr; pb.shadowQueue = ctx->shadowQueue.ptr; pb.tailList = ctx->tailList.ptr;
    pb.queueCount = ctx->queueCount.ptr; pb.activeSlots = ctx->activeSlots.ptr; pb.errorWord = ctx->activeSlots.ptr + 1; pb.tailMode = ctx->activeSlots.ptr + 3; pb.tailWords = ctx->activeSlots.ptr + 4; pb.tailIdled = ctx->activeSlots.ptr + 2; pb.windowSamples = ctx->activeSlots.ptr + 6; pb.idleShards = ctx->idleShards.ptr; pb.blockDead = ctx->blockDead.ptr; pb.totals = ctx->totals.ptr;
    pb.pixelXY = ctx->pixelXY.ptr;

    RenderParams& rp = ctx->params;
    rp.numSlots = numPixels ? (uint32_t)numSlots : 0u; rp.numBlocks = rp.numSlots / 256u; rp.numPixels = numPixels; rp.stripes = stripes;
    rp.sppBegin = 0; rp.sppCount = 0; rp.workItems = 0; rp.numWaves = rp.numSlots / 64u; rp.runLength = 1; rp.numRuns = 0;
    rp.rngSeed = st->rng_seed; rp.timeStart = st->time_start; rp.timeEnd = st->time_end;
    rp.imageWidth = W; rp.imageHeight = H;
    rp.countSlots = (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) ? 1u : 0u;
    rp.shardCapacity = shardCapacity;
    rp.spectral = spectral ? 1u : 0u;
    rp.injectError = (ctx->config.flags & SLRHIP_FLAG_TEST_DEVICE_ERROR) ? 1u : 0u;
    ctx->settings = *st;
    ctx->shard = shard;
    ctx->iterations = 0;
    ctx->firstRenderCall = true;
    ctx->haveRender = true;
    return SLRHIP_OK;
}

// One window of passes [sppBegin, sppBegin + sppCount): every sample of the window rendered into the result window, then folded
// into the sensor in pass order.  slrhip_render sizes the windows.
static int renderWindow(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, hipStream_t stream) {
    RenderParams& rp = ctx->params;
    rp.sppBegin = sppBegin;
    rp.sppCount = sppCount;
    rp.workItems = rp.numPixels * sppCount;                        // < 2^32: slrhip_render
    // passes per run (pt_kernels.h WorkItem): the largest power of two <= the default that divides the window's pass count
    static const uint32_t envRun = [] { const char* e = getenv("SLRHIP_RUN_LENGTH"); const long v = e ? atol(e) : 0L; return v >= 1 && v <= 4096 ? (uint32_t)v : 0u; }();
    rp.runLength = envRun ? envRun : kDefaultRunLength;
    while (rp.runLength > 1 && (sppCount % rp.runLength) != 0) rp.runLength /= 2;
    if (sppCount && sppCount % rp.runLength) rp.runLength = 1;
    rp.numRuns = rp.numPixels * (sppCount / std::max(rp.runLength, 1u));

    // the first window after render_begin also clears the sensor (the buffers are reused across render_begin calls), even when
    // it is asked for zero passes
    launchResetSlots(ctx->buffers, rp, ctx->firstRenderCall, stream);
    ctx->firstRenderCall = false;
    if (sppCount == 0) return SLRHIP_OK;
    // persistent traversal workgroups of the wave-specialised kernel (pt_trace_ws.hip): a fixed number per CU
    const uint32_t traceBlocks = (uint32_t)ctx->numCUs * (uint32_t)traceWsBlocksPerCU(ctx->scene.nodesQ != nullptr);

    uint32_t active = rp.numSlots;
    uint32_t status[4] = {active, 0u, 0u, 0u};       // device words: live slots, error bits, slots idled by the tail kernel, tail mode (PathBuffers)
    // The end of the window (pt_tail_kernels.h): once at most tailSlots slots are alive the traversal kernel raises the tail-mode
    // word instead of tracing, the rest of the block of iterations is no-ops, and the tail kernel finishes every remaining path
    // and sample in one launch.  The image does not depend on who finishes a sample (the sensor adds in pass order).  On with
    // the automatic slot count (slrhip_config::stripes = 0) and on request (SLRHIP_FLAG_TAIL_KERNEL, SLRHIP_TAIL_SLOTS=n); a
    // caller who fixes the slot count gets the pure wavefront schedule unless he asks (the parity tests compare the two).  Never
    // for more than an eighth of the slots (the wavefront kernels are the efficient way to advance many paths) and not in the
    // counting build (its per-ray figures come from the wavefront kernels).  SLRHIP_TAIL_SLOTS=0 turns it off.
    static const long envTail = [] { const char* e = getenv("SLRHIP_TAIL_SLOTS"); return e ? atol(e) : -1L; }();
    {
        const bool asked = (ctx->config.flags & SLRHIP_FLAG_TAIL_KERNEL) != 0 || envTail > 0 || ctx->config.stripes == 0;
        const uint32_t bound = envTail > 0 ? (uint32_t)std::min<long>(envTail, 0x7FFFFFFFL) : kDefaultTailSlots;
        const bool off = !asked || envTail == 0 || !tailKernelAvailable(ctx->scene, rp.spectral != 0) || (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) != 0;
        rp.tailSlots = off ? 0u : std::min(bound, active / SLR_TAIL_DIVISOR);
    }
    // The window is complete only if the queues handed out exactly one sample per pixel and pass: the device's own count
    // (k_count_samples over the queues' cursors) against the host's arithmetic.  A lost or repeated sample would leave a stale
    // or overwritten entry in the result window — never silent.
    const auto checkWindow = [&](hipStream_t s) -> int {
        uint32_t words[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(words, ctx->activeSlots.ptr, kStatusWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (words[1]) return deviceError(words[1]);
        if (words[6] != rp.workItems)
            return fail(SLRHIP_ERR_HIP, "slrhip_render: the work queues handed out " + std::to_string(words[6]) + " samples for a window of " +
                                            std::to_string(rp.workItems) + " (internal error)");
        return SLRHIP_OK;
    };
    // tail mode seen in the status words: list the live slots, finish them, read the words again (live slots must be 0 then)
    const auto runTail = [&](hipStream_t s, bool timed) -> int {
        hipEvent_t t0 = nullptr, t1 = nullptr;
        if (timed) { HIP_TRY(hipEventCreate(&t0)); HIP_TRY(hipEventCreate(&t1)); HIP_TRY(hipEventRecord(t0, s)); }
        launchTail(ctx->scene, ctx->buffers, rp, status[0], ctx->numCUs, s);
        if (timed) HIP_TRY(hipEventRecord(t1, s));
        HIP_TRY(hipGetLastError());
        const uint32_t liveBefore = status[0];
        uint32_t words[6] = {0, 0, 0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(words, ctx->activeSlots.ptr, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(status, words, 4 * sizeof(uint32_t));
        if (timed) {
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, t0, t1));
            ctx->profMs[SLRHIP_KERNEL_TAIL] += ms;
            ++ctx->profLaunches[SLRHIP_KERNEL_TAIL];
            (void)hipEventDestroy(t0); (void)hipEventDestroy(t1);
        }
        if (status[1]) return deviceError(status[1]);
        if (words[2] != words[4])
            return fail(SLRHIP_ERR_HIP, "slrhip_render: the tail kernel left " + std::to_string(words[4] - words[2]) + " of " + std::to_string(words[4]) +
                                            " listed slots live (live count before: " + std::to_string(liveBefore) + ", cursor " + std::to_string(words[5]) + "; internal error)");
        // every listed slot ended idle and the wavefront kernels are off (tail mode): nothing is live any more
        HIP_TRY(hipMemsetAsync(ctx->activeSlots.ptr, 0, sizeof(uint32_t), s));
        status[0] = 0;
        return SLRHIP_OK;
    };
    // One wavefront iteration = k_shade (advance every live path by one vertex; finish and restart the paths that end) then
    // k_trace_ws (the extension and shadow rays that left).  Each check of the live-slot word costs one small copy + stream
    // sync; 16 iterations between checks keeps it < 1 %.
    const int kCheckEvery = 16;
    const int kEv = 3;    // events per iteration: before shade, after shade, after trace
    const bool timeKernels = (ctx->config.flags & SLRHIP_FLAG_TIME_KERNELS) != 0;
    const bool count = (ctx->config.flags & SLRHIP_FLAG_COUNT_TRAVERSAL) != 0;
    if (timeKernels && ctx->events.empty()) {
        ctx->events.resize((size_t)kCheckEvery * kEv);
        for (hipEvent_t& e : ctx->events) HIP_TRY(hipEventCreate(&e));
    }
    const uint64_t maxIterations = ((uint64_t)rp.workItems / rp.numSlots + 2) * 128 + 1024;   // paths are <= 100 vertices long
    uint64_t it = 0;

    // The block of kCheckEvery iterations is the same sequence of launches every time (the parity alternates inside it and is
    // back to 0 at its end), so it is captured ONCE per call into a hipGraph and replayed: one submission per block instead
    // of 32 launches with their dispatch gaps — what is left of the cost of the nearly empty iterations at the end of a
    // render.  Capture needs a real stream, so the work runs on the context's own stream, ordered after the caller's by an
    // event; render() returns only after that stream is idle, which orders the caller's later work after it.
    static const bool noGraph = [] { const char* e = getenv("SLRHIP_GRAPH"); return e && std::string(e) == "0"; }();
    if (!timeKernels && !noGraph && rp.numSlots >= (1u << 18)) {
        if (!ctx->workStream) {
            HIP_TRY(hipStreamCreateWithFlags(&ctx->workStream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&ctx->userReady, hipEventDisableTiming));
        }
        hipStream_t ws = ctx->workStream;
        HIP_TRY(hipEventRecord(ctx->userReady, stream));          // the reset kernel above and whatever the caller queued before
        HIP_TRY(hipStreamWaitEvent(ws, ctx->userReady, 0));
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        HIP_TRY(hipStreamBeginCapture(ws, hipStreamCaptureModeThreadLocal));
        for (int k = 0; k < kCheckEvery; ++k) {
            launchShade(ctx->scene, ctx->buffers, rp, (uint32_t)(k & 1), ws);
            launchTraceWs(ctx->scene, ctx->buffers, rp, (uint32_t)(k & 1), traceBlocks, count, ws);
        }
        hipError_t ce = hipStreamEndCapture(ws, &graph);
        if (ce == hipSuccess) ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (ce != hipSuccess) {
            if (graph) (void)hipGraphDestroy(graph);
            return fail(SLRHIP_ERR_HIP, std::string("slrhip_render: hipGraph capture failed: ") + hipGetErrorString(ce));
        }
        int rc = SLRHIP_OK;
        while (active > 0 && rc == SLRHIP_OK) {
            hipError_t e = hipGraphLaunch(exec, ws);
            if (e == hipSuccess) e = hipMemcpyAsync(status, ctx->activeSlots.ptr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, ws);
            if (e == hipSuccess) e = hipStreamSynchronize(ws);
            if (e != hipSuccess) rc = fail(SLRHIP_ERR_HIP, std::string("slrhip_render: ") + hipGetErrorString(e));
            it += kCheckEvery;
            if (rc == SLRHIP_OK && status[1]) rc = deviceError(status[1]);
            if (rc == SLRHIP_OK && status[3] && status[0]) rc = runTail(ws, false);
            active = status[0];
            if (rc == SLRHIP_OK && it > maxIterations) rc = fail(SLRHIP_ERR_HIP, "slrhip_render: iteration bound exceeded (internal error)");
        }
        (void)hipGraphExecDestroy(exec);
        (void)hipGraphDestroy(graph);
        if (rc != SLRHIP_OK) return rc;
        ctx->iterations += it;
        launchCountSamples(ctx->buffers, rp, ws);      // samples rendered in this window, counted on the device (T_SAMPLES)
        launchFold(ctx->buffers, rp, ws);              // sensor->add, in pass order
        HIP_TRY(hipGetLastError());
        return checkWindow(ws);
    }

    // SLRHIP_ITER_LOG=path (with SLRHIP_FLAG_TIME_KERNELS): per-iteration kernel times of this call, one line per iteration
    // "iteration shade_ms trace_ms live_slots_at_block_end" — how the drain of a render's last paths was measured
    static const char* iterLog = getenv("SLRHIP_ITER_LOG");
    std::vector<float> iterMs;
    std::vector<uint32_t> iterActive;
    uint32_t parity = 0;
    while (active > 0) {
        for (int k = 0; k < kCheckEvery; ++k) {
            hipEvent_t* ev = timeKernels ? &ctx->events[(size_t)k * kEv] : nullptr;
            if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
            launchShade(ctx->scene, ctx->buffers, rp, parity, stream);
            if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
            launchTraceWs(ctx->scene, ctx->buffers, rp, parity, traceBlocks, count, stream);
            if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
            parity ^= 1;
            ++it;
        }
        HIP_TRY(hipGetLastError());                  // a failed launch surfaces here, not at the end of the render
        HIP_TRY(hipMemcpyAsync(status, ctx->activeSlots.ptr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        active = status[0];
        if (status[1]) return deviceError(status[1]);
        if (timeKernels) {
            static const int cls[2] = {SLRHIP_KERNEL_SHADE, SLRHIP_KERNEL_TRACE};
            for (int k = 0; k < kCheckEvery; ++k) {
                hipEvent_t* ev = &ctx->events[(size_t)k * kEv];
                for (int j = 0; j < 2; ++j) {
                    float ms = 0.0f;
                    HIP_TRY(hipEventElapsedTime(&ms, ev[j], ev[j + 1]));
                    ctx->profMs[cls[j]] += ms;
                    ++ctx->profLaunches[cls[j]];
                    if (iterLog) iterMs.push_back(ms);
                }
                if (iterLog) iterActive.push_back(active);
            }
        }
        if (status[3] && status[0]) {
            const int rc = runTail(stream, timeKernels);
            if (rc != SLRHIP_OK) return rc;
            active = status[0];
        }
        if (it > maxIterations) return fail(SLRHIP_ERR_HIP, "slrhip_render: iteration bound exceeded (internal error)");
    }
    ctx->iterations += it;
    launchCountSamples(ctx->buffers, rp, stream);       // samples rendered in this window, counted on the device (T_SAMPLES)
    launchFold(ctx->buffers, rp, stream);               // sensor->add, in pass order
    HIP_TRY(hipGetLastError());
    {
        const int rc = checkWindow(stream);
        if (rc != SLRHIP_OK) return rc;
    }
    if (iterLog && timeKernels && !iterActive.empty()) {
        if (FILE* f = fopen(iterLog, "a")) {
            const size_t per = iterMs.size() / iterActive.size();
            fprintf(f, "# render: %u slots, %u passes from %u\n", rp.numSlots, sppCount, sppBegin);
            for (size_t i = 0; i < iterActive.size(); ++i) {
                fprintf(f, "%zu", i);
                for (size_t j = 0; j < per; ++j) fprintf(f, " %.4f", iterMs[i * per + j]);
                fprintf(f, " %u\n", iterActive[i]);
            }
            fclose(f);
        }
    }
    return SLRHIP_OK;
}

int slrhip_render(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render: call slrhip_render_begin first");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    RenderParams& rp = ctx->params;
    if (rp.numSlots == 0) { ctx->firstRenderCall = false; return SLRHIP_OK; }
    // The result window (PathBuffers::results) holds one entry per pixel and pass: 16 B (RGB) / 64 B (spectral).  A call of more
    // passes than fit the budget — 16 GiB by default, SLRHIP_RESULT_WINDOW_MB overrides — or than 2^32 samples is rendered as
    // several windows, one after the other; the sensor adds in pass order either way, so the image does not depend on the split.
    const uint64_t entryBytes = (rp.spectral ? 4u : 1u) * sizeof(float4);
    uint64_t budget = 16ull << 30;
    if (const char* e = getenv("SLRHIP_RESULT_WINDOW_MB")) { const long mb = atol(e); if (mb > 0) budget = (uint64_t)mb << 20; }
    const uint64_t maxPasses = std::max<uint64_t>(1, std::min<uint64_t>(budget / ((uint64_t)rp.numPixels * entryBytes), 0xF0000000ull / rp.numPixels));      // (run ids + one round of waves stay inside 32 bits)
    // whole runs (RenderParams::runLength passes of a pixel in a row, pt_kernels.h) wherever the call is long enough: a window of
    // an odd number of passes would fall back to runs of one pass and lose the coherence of a wave's slots
    uint32_t window = (uint32_t)std::min<uint64_t>(maxPasses, std::max<uint32_t>(sppCount, 1u));
    if (window >= kDefaultRunLength) window -= window % kDefaultRunLength;
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
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight * (rp.spectral ? 16 : 3);
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
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight * (rp.spectral ? 16 : 3);
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
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight * (rp.spectral ? 16 : 3);
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
