// slrhip_ctx.h — the context behind the C ABI of include/slrhip.h and what its translation units share: slrhip_api.hip,
// slrhip_buffers.hip, slrhip_image.hip, slrhip_environment.hip, slrhip_instances.hip, slrhip_toplevel.hip, slrhip_geometry.hip, slrhip_materials.hip, slrhip_diagnostics.hip.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/slrhip.h"
#include "bvh.h"
#include "materials_prep.h"
#include "pt_clamp.h"
#include "pt_kernels.h"
#include "pt_motion.h"
#include "render_plan.h"
#include "scene_prep.h"

namespace slrhip {

const uint32_t kStatusWords = 8;               // PathBuffers::activeSlots .. tailWords: one small array, read back in one copy
enum StatusWord : uint32_t {                   // its words (bindBuffers points PathBuffers at them)
    S_LIVE = 0, S_ERROR = 1,                   // live slots; device error word
    S_TAIL_IDLED = 2, S_TAIL_MODE = 3,         // slots the tail kernel left idle; 1 + parity once the traversal kernel has handed over to it
    S_TAIL_LENGTH = 4, S_TAIL_CURSOR = 5,      // tail list length / cursor
    S_WINDOW_SAMPLES = 6                       // samples the queues handed out in the window
};

// Records `msg` as the calling thread's slrhip_last_error_string and returns `code` (slrhip_api.hip).
int fail(int code, const std::string& msg);

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
extern std::atomic<size_t> g_skewCounter;        // shared by every context of the process; contexts may be set up from several threads (slrhip_api.hip)

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

// One float4 record per pixel of the shard, updated by k_fold and read out as a channel or as totals (pt_stats.hip): the noise
// statistics and the sample clamp.  Allocated by the first enabling call (slrhip_*_begin), kept for later renders.
template <typename Totals> struct PixelRecords {
    DevArray<float4> records;
    DevArray<Totals> partials, totals;            // the summary's first-stage partials and its result
    bool on = false;                              // this render folds with this kind's instantiation of k_fold
    bool clear = false;                           // the records still hold an earlier render's: cleared in stream order before their first use
};

} // namespace slrhip

struct slrhip_ctx {
    template <typename T> using DevArray = slrhip::DevArray<T>;
    slrhip_config config;
    int device = 0;
    int numCUs = 256;
    bool haveScene = false;
    bool haveRender = false;

    // scene
    DevArray<slrhip::QNode> nodes;
    DevArray<slrhip::QNodeQ> nodesQ;
    DevArray<slrhip::DevTexture> textures;
    DevArray<slrhip::DevMatTex> matTex;
    DevArray<float4> triUV, alphaTris;
    DevArray<float> texTexels;
    DevArray<slrhip::LeafTri> leafTris;
    DevArray<slrhip::ShadeTri> shadeTris;
    DevArray<slrhip::LightTri> lightTris;
    DevArray<slrhip::DevInstance> instances;
    // slrhip_set_instance_transforms: the meshes' local boxes and the instances' world boxes (lo, hi: two float4 each), its status
    // word, and the top-level tree's extent in `nodes`: the first node of each level, then the number of top-level nodes
    DevArray<float4> meshBoxes, instBoxes;
    DevArray<uint32_t> instanceStatus;
    std::vector<uint32_t> topLevelFirst;
    // slrhip_rebuild_top_level (slrhip_toplevel.hip): what its first call after an upload builds and allocates — the leaf slots of
    // the top level depth-first, the primitives' child words in canonical order, the packets' boxes, the identity the radix sort
    // permutes — and what every call writes: keys by primitive, the order (slot i receives primitive topOrder[i]).  topSeatReady:
    // they belong to the scene in place (slrhip_upload_scene drops them).
    DevArray<uint32_t> topSlots, topRefs, topIdentity, topOrder;
    DevArray<float4> topPacketBoxes;
    DevArray<uint64_t> topKeys, topSortedKeys;
    DevArray<uint8_t> topSortTemp;
    std::vector<uint32_t> topSlotsHost, topRefsHost;
    bool topSeatReady = false;
    uint32_t topPrimitives = 0;
    uint32_t topLastPath = 0, topLastLaunches = 0;       // the last call: 1 one workgroup, 2 keys + radix sort + seat; its launches (0: none yet)
    // slrhip_set_vertices (contexts created with SLRHIP_FLAG_DYNAMIC_GEOMETRY; flat scenes without spatial splits): the scene's vertex
    // and index arrays, one box (lo, hi) per LeafTri record as scratch, its status word, and the first node of each tree level, then the
    // number of nodes.  geometryKept: the arrays belong to the scene in place (else they are empty or an earlier scene's, and unused).
    DevArray<slrhip_vertex> geoVertices;
    DevArray<slrhip_triangle> geoTriangles;
    DevArray<float4> geoLeafBoxes;
    DevArray<uint32_t> geometryStatus;
    std::vector<uint32_t> geoLevelFirst;
    bool geometryKept = false;
    uint32_t geoNumVertices = 0, geoNumTriangles = 0, geoNumLights = 0, geoNumAlphaRecords = 0;
    bool geoHasTriUV = false;
    uint32_t geoLastLaunches = 0;                 // launches of the last slrhip_set_vertices call (slrhip_debug_geometry's summary)
    // ... and of a scene WITH instances (contexts created with SLRHIP_FLAG_DYNAMIC_INSTANCED as well): geoInstanced, geoLevelFirst is
    // the top level's table (topLevelFirst), and the mesh trees' merged level list (bvh.h: QBVH::meshLevelNodes / meshLevelFirst) and
    // each mesh's root node are kept on the device.  The boxes the call rewrites are meshBoxes and instBoxes above.
    bool geoInstanced = false;
    DevArray<uint32_t> geoMeshLevelNodes, geoMeshRoots;
    std::vector<uint32_t> geoMeshLevelFirst;
    // slrhip_set_materials (slrhip_materials.hip): what it checks new tables against, the emitting bit per material and the workgroup
    // offsets of its light-list rebuild (allocated by the first call that rebuilds), and its last call for slrhip_debug_materials
    slrhip::MaterialsKept matKept;
    DevArray<uint32_t> matEmitMask, matOffsets;
    uint32_t matLastLaunches = 0;
    bool matLastRebuilt = false;
    DevArray<slrhip::DevMaterial> materials;
    DevArray<slrhip::DevMaterialS> materialsS;
    DevArray<slrhip::DevSpectrum> spectra;
    DevArray<float> spectrumPool;
    DevArray<float> lightPMF, lightCDF;
    DevArray<float4> shadeTables;
    DevArray<float> envTexels, envTopPDF, envTopCDF, envRowPDF, envRowCDF;
    DevArray<float> envImportance;                // slrhip_set_environment: the importance map it built (the upload's comes from the host and is not kept)
    DevArray<double> envSinRow;                   // ... and the rows' sines, copied from the host
    bool envOwnMap = false;                       // the environment is slrhip_set_environment's: envImportance belongs to it
    DevArray<uint8_t> gridCells;
    DevArray<float> pointUV, pointSpectrum;
    slrhip::DevScene scene;
    uint32_t bvhDepth = 0;
    uint64_t bvhLeafRefs = 0;
    uint32_t treeBuilder = 0;                     // SLRHIP_TREE_* (include/slrhip_debug.h): the builder behind the scene's tree, for slrhip_debug_tree
    double buildSeconds = 0.0;

    // render state
    slrhip_render_settings settings;
    slrhip_shard shard;
    slrhip::RenderParams params;
    DevArray<uint32_t> pixelXY;
    DevArray<uint4> rng;
    DevArray<float4> rayOrg, rayDir, hit, alpha, spR, spC, nee, shadowDir;
    DevArray<float4> results, fbSum, fbComp;      // result window of the current render call; the sensor (per-pixel Kahan sums)
    DevArray<uint32_t> cursor, idleShards;
    DevArray<float> pdfPrev;
    DevArray<uint4> hdr;
    DevArray<int32_t> hitInstance;
    DevArray<int32_t> primaryInstance;            // instanced scenes: the instance plane of the primary pass, one entry per sample of the window (renderWindow)
    DevArray<uint4> primaryRng;                   // windows with a primary pass: the stream after the camera draws, one entry per sample of the window (renderWindow)
    uint64_t primaryRngEntries = 0;               // ... as the last window bound it to PathBuffers::primaryRng; 0: that window had no pass (slrhip_debug_primary_stream_entries)
    slrhip::PrimaryKernel primaryKernel = slrhip::PrimaryKernel::None;      // the kernel the last window's primary pass was launched with; None: it ran no pass (slrhip_debug_primary_kernel)
    slrhip::ShadeVariant shadeVariant = {};       // the last window's k_shade instantiation (renderWindow), and whether launchShade launched it
    bool shadeLaunched = false, tailLaunched = false;      // ... and launchTail its twin (slrhip_debug_shade_kernel)
    DevArray<uint32_t> flags, visible, shadowQueue, tailList, queueCount, activeSlots, blockDead;
    DevArray<uint64_t> totals;
    DevArray<float> resolveScratch;
    DevArray<uint32_t> queryError;                // ERR_* bits of the ray queries (slrhip_query_status); apart from the render's error word
    // first-hit feature buffers (slrhip_render_features): allocated by the first feature call after render_begin, never by a render
    DevArray<float4> featGeometric, featShading, featTangent, featRecords;
    DevArray<float> featB2;
    DevArray<uint4> featIds;
    DevArray<uint32_t> featError;                 // ERR_* bits of the feature passes (slrhip_features_status)
    uint32_t featChannels = 0;                    // the channel set of the feature calls since render_begin (0: none yet)
    uint32_t featWindow = 0;                      // passes per launch (the record window)
    uint64_t featPassEnd = 0;                     // 1 + the highest pass rendered since render_begin (whose ids the pixels hold)
    bool featErrorReady = false;                  // featError allocated and cleared since render_begin (by the first feature or albedo call)
    // the albedo buffer (slrhip_render_albedo): the sums are allocated by the first albedo call after render_begin; the record window is the feature pass's
    DevArray<float> albSums;                      // `components` planes of numPixels floats
    bool albReady = false;                        // sums allocated and cleared since render_begin
    uint32_t albWindow = 0;                       // passes per launch
    uint64_t albPasses = 0;                       // passes accumulated since render_begin
    // the motion buffer (slrhip_render_motion): the sums are allocated by the first motion call after render_begin; the record window is the feature pass's
    DevArray<float4> motionSums;                  // {sum m.x, sum m.y, sum z', valid samples} per pixel of the shard
    bool motionReady = false;                     // sums allocated and cleared since render_begin
    uint32_t motionWindow = 0;                    // passes per launch of slrhip_render_motion (0: none since the sums were cleared)
    uint32_t motionVerticesWindow = 0;            // ... and of slrhip_render_motion_vertices, whose window also keeps b2
    // per-pixel noise statistics: records {mean, M2, n, max}; the sample clamp: records {clamped, dropped (uint32 bits), removed, largest}
    slrhip::PixelRecords<slrhip::StatsTotals> stats;
    slrhip::PixelRecords<slrhip::ClampTotals> clamp;
    float clampLimit = 0.0f;
    uint32_t clampFlags = 0;
    // adaptive sampling (slrhip_render_adaptive): the list buffers are allocated by the first adaptive call and kept for later renders
    DevArray<uint32_t> adaptXY[2], adaptIndex[2]; // the active list (pt_kernels.h AdaptiveSelect), two pairs that alternate
    DevArray<uint32_t> adaptOffsets, adaptCount;  // the select's workgroup offsets; the new list's length (read back once per block)
    uint32_t activePixels = 0;                    // pixels of the shard not yet retired since render_begin
    int activeList = -1;                          // the pair that holds them; -1: every pixel of the shard (no check has run yet)
    // the denoiser (slrhip_denoise): allocated by the first call and by any call that needs more, never by a render
    DevArray<uint8_t> denoiseScratch;
    slrhip::PathBuffers buffers;
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

namespace slrhip {

// ---- defined in slrhip_api.hip (featureParams: slrhip_buffers.hip), for the entry points of the other files ----
// The pixels of a window of slrhip_render_adaptive: a compact list (pt_kernels.h AdaptiveSelect) instead of the shard's.
struct ActiveWindow {
    const uint32_t* xy;           // compact index -> x | y << 16
    const uint32_t* index;        // compact index -> pixel of the shard
    uint32_t count;
};
int renderWindow(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, hipStream_t stream, const ActiveWindow* active = nullptr);
// The noise and clamp records of an earlier render are cleared before their first use in this one, in order on the stream of that use.
int clearStatistics(slrhip_ctx* ctx, hipStream_t stream);
// the result window's budget (render_plan.cpp, planWindows): 16 GiB by default, SLRHIP_RESULT_WINDOW_MB overrides
uint64_t resultWindowBudget();
long autoStripesOverride(); int pairsMask(); uint32_t runLengthOverride();      // overrides of the render plan, each read once per process

inline uint32_t prevPowerOf2(uint32_t x) {   // defines.h:136-143
    x |= x >> 1; x |= x >> 2; x |= x >> 4; x |= x >> 8; x |= x >> 16;
    return x - (x >> 1);
}

inline size_t frameFloats(const RenderParams& rp) { return (size_t)rp.imageWidth * rp.imageHeight * (rp.spectral ? 16 : 3); }
inline ClampParams clampParams(const slrhip_ctx* ctx) { return ClampParams{ctx->clamp.on ? ctx->clamp.records.ptr : nullptr, ctx->clampLimit, ctx->clampFlags}; }
FeatureParams featureParams(const slrhip_ctx* ctx, uint32_t channels, uint32_t passBegin, uint32_t numPasses);

// A read-out to host memory through the context's scratch: room for `scratchFloats`; with `syncFirst`, a wait for what is queued on any
// stream of the caller's; `resolve(scratch)` on the null stream; the feature error word (`featureErrorOf`: the entry point that reads
// it) or a wait for the device; `need` floats to `hostDst`.  The caller checks the arguments that the resolve it calls does not.
template <typename Resolve>
int readThroughScratch(slrhip_ctx* ctx, void* hostDst, size_t need, size_t scratchFloats, bool syncFirst, const char* featureErrorOf, Resolve resolve) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(ctx->resolveScratch.alloc(scratchFloats));
    if (syncFirst) HIP_TRY(hipDeviceSynchronize());
    if (const int rc = resolve(ctx->resolveScratch.ptr)) return rc;
    if (featureErrorOf) {
        uint32_t bits = 0;
        if (const int rc = slrhip_features_status(ctx, &bits, nullptr)) return rc;
        if (bits) return fail(SLRHIP_ERR_HIP, std::string(featureErrorOf) + ": the feature error word is set (a traversal gave up): " + std::to_string(bits));
    }
    else HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, ctx->resolveScratch.ptr, need * sizeof(float), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // namespace slrhip
