// pt_kernels.h — launch interface between the C-ABI layer (slrhip_api.hip and the slrhip_*.hip beside it) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slrhip.h"
#include "device_types.h"

namespace slrhip {

// Limits of the shading tables staged in LDS by k_shade / k_tail (ShadeLds, pt_shade_tables.h); larger scenes read them from HBM.
static const int kLdsMaterials = 32;
static const int kLdsLights = 16;
static const int kLdsSpectra = 96;
static const int kLdsPoolFloats = 6144;     // 24 KiB: the spectrum sample tables of a scene (spectral mode), staged per workgroup
static const int kShadeBlock = 256;         // slots per workgroup of the kernels that walk the slots: numSlots = 256 x workgroups

// Scene arrays resident in HBM (uploaded once by slrhip_upload_scene).
struct DevScene {
    const float4* nodes;          // QNode as 8 x float4, breadth-first
    const float4* leafTris;       // LeafTri as 3 x float4
    const ShadeTri* shadeTris;    // indexed by scene triangle index
    const LightTri* lightTris;    // indexed by light index
    const DevMaterial* materials;  // RGB mode
    const DevMaterialS* materialsS; // spectral mode: spectrum indices instead of constants
    const DevSpectrum* spectra;
    const float* spectrumPool;
    const float* lightPMF;        // RegularConstantDiscrete1D of the aggregate's light list
    const float* lightCDF;        // numLights + 1 entries
    uint32_t numNodes;
    const float4* nodesQ;         // QNodeQ array (4 x float4 per node) or nullptr: large scenes traverse this one
    uint32_t numMaterials;
    uint32_t numLights;
    uint32_t lightPow2;           // prevPowerOf2(numLights)
    uint32_t hasMicrofacet;       // any SLRHIP_MATERIAL_MICROFACET_* in the scene
    uint32_t hasMulti;            // any SLRHIP_MATERIAL_MULTI: k_shade with the MultiBSDF code
    // textures: null / 0 when the scene has none
    const DevTexture* textures;
    const DevMatTex* matTex;      // per material
    const float4* triUV;          // per scene triangle: (u0, v0, u1, v1), (u2, v2, -, -)
    const float4* alphaTris;      // per alpha record (LeafTri::alpha): the same two float4 + the alpha texture index
    const float* texTexels;       // texels of the image textures, 3 floats each: (r, g, b), spectral mode (u, v, s)
    // The tables k_shade / k_tail stage in LDS, packed by slrhip_upload_scene into ONE array in the order of ShadeLds'
    // segments — RGB: materials, lights, light PMF, light CDF; spectral: materials, spectra, sample pool, lights, PMF, CDF — each
    // padded to whole float4; tableEnd[k] = end of segment k in float4 (cumulative).  nullptr when the scene exceeds the LDS limits.
    const float4* shadeTables;
    uint32_t tableEnd[6];
    const float4* instances;      // DevInstance as 9 x float4, or nullptr: the scene has no instanced mesh
    uint32_t numInstances;
    uint32_t numTextures;
    uint32_t numSpectra;
    uint32_t numSpectrumData;     // floats in spectrumPool (padded to a multiple of 4 on upload)
    // environment sphere (InfiniteSphereSurfaceObject, SurfaceObject.cpp:137-222); RGB mode
    uint32_t hasEnv;
    uint32_t envWidth, envHeight, envMapWidth, envMapHeight;
    float envScale;
    float aggImportance;          // SurfaceObjectAggregate::importance() = integral of the light list distribution
    const float* envTexels;       // [height][width][3]
    const float* envTopPDF;       // RegularConstantContinuous2D: top distribution over rows (mapHeight, +1 for the CDF)
    const float* envTopCDF;
    const float* envRowPDF;       // [mapHeight][mapWidth]
    const float* envRowCDF;       // [mapHeight][mapWidth + 1]
    // spectral mode: the environment texels are (u, v, s); the Meng-15 tables to look them up at run time (slrhip_upsampling_tables)
    uint32_t gridWidth, gridHeight;
    const uint8_t* gridCells;     // 8 bytes per cell: inside, num_points, idx[6]
    const float* pointUV;         // 2 per data point
    const float* pointSpectrum;   // 95 per data point
    DevCamera camera;
};

// Queue counters.  A counter word that every wave bumps saturates near 88 atomics/us on this chip
// (MI355X_MICROARCH.md, rows "dequeue" / "fanin"), which made the first version of the shade kernel
// atomic-bound (14 400 waves -> 164 us).  So: (1) there is NO extension-ray queue — nearly every live
// slot has one, the traversal kernel walks all slots and reads the state flag; (2) there is no queue of
// finished paths either — the shade kernel restarts them itself (k_shade); (3) the shadow-ray queue is
// split into kShards regions, a workgroup appends to region (blockIdx % kShards) with ONE atomic per
// workgroup, and every counter sits on its own 128-byte line.
// One set of counters per iteration parity: k_shade(parity) FILLS set `parity`, k_trace_ws(parity) READS it
// and clears set `parity ^ 1` for the next k_shade.
static const uint32_t kShards = 16;
static const uint32_t kCounterStride = 32;                 // words: one 128-byte line per counter
enum { Q_SHADOW = 0, Q_KINDS = 1 };
static const uint32_t kQueueSetWords = Q_KINDS * kShards * kCounterStride;
__host__ __device__ inline uint32_t queueCounterIndex(uint32_t parity, uint32_t kind, uint32_t shard) {
    return parity * kQueueSetWords + (kind * kShards + shard) * kCounterStride;
}
// statistics, sharded the same way: [kind][shard] 64-bit words on separate lines
enum { T_EXT_RAYS = 0, T_SHADOW_RAYS = 1, T_NODES_CLOSEST = 2, T_TRIS_CLOSEST = 3, T_NODES_SHADOW = 4, T_TRIS_SHADOW = 5,
       T_SLOT_VISITS = 6,
       // schedule diagnostics of the wave-specialised closest-hit kernel (counting builds only; SLRHIP_DEBUG_WS prints them)
       T_WS_STEPS = 7, T_WS_IDLE_SPINS = 8, T_WS_CYCLES = 9, T_WS_IDLE_CYCLES = 10, T_WS_REFILLS = 11, T_WS_PRODUCER_WAITS = 12,
       T_WS_NODE_BLOCKS = 13, T_WS_TRI_BLOCKS = 14, T_WS_ACTIVE_LANES = 15,
       T_SAMPLES = 16,          // finished samples accumulated into pixels, summed from the slots' headers at the end of a render call
       T_PRIMARY_STARTS = 17,   // samples that took their first hit from the primary pass's record (k_shade's fused start, k_tail)
       T_SHADOW_SKIPPED = 18,   // light samples k_shade did not trace because they decide nothing (counted in T_SHADOW_RAYS too: rays the algorithm casts)
       T_KINDS = 19 };
// device error word bits (PathBuffers::errorWord): set by any kernel path that gives up or drops work
enum : uint32_t { ERR_RING_SPACE = 1u, ERR_RING_RELEASE = 2u, ERR_CONSUMER_IDLE = 4u, ERR_STACK_OVERFLOW = 8u, ERR_QUEUE_OVERFLOW = 16u };
static const uint32_t kTotalStride = 16;                   // 64-bit words: one 128-byte line
__host__ __device__ inline uint32_t totalIndex(uint32_t kind, uint32_t shard) { return (kind * kShards + shard) * kTotalStride; }

// Path state, SoA, one record per slot.  A slot is a path in flight, NOT a place in the image: whenever its path ends it takes the
// next sample — a (pixel, pass) pair — from the work queue of its wave of the shade kernel (WorkItem below) and writes the finished
// sample's contribution to the result window; the sensor's per-pixel Kahan sum (ImageSensor::add, in pass order) is done by
// k_fold once the window's passes are complete.  The image therefore does not depend on the number of slots, on which slot
// rendered which sample or on the shard size, and the slots stay busy until the LAST sample of the call has been handed out.
struct PathBuffers {
    uint4* rng;                   // xorshift128 state
    float4* rayOrg;               // extension / shadow ray origin, w = distMin
    float4* rayDir;               // extension ray direction, w = distMax
    float4* hit;                  // x = triangle (bits), y = t, z = b1, w = b2 (Moller-Trumbore's barycentrics)
    int32_t* hitInstance;         // instanced scenes only (else nullptr): the instance the hit went through, -1 = a loose triangle
    // spectrum-valued records: RGB = one float4 per slot (scalar in .w); spectral = 4 planes of numSlots float4
    float4* alpha;                // path throughput (+ pdf of the sampled direction)
    float4* spR;                  // path radiance Kahan sum (sp) (+ camera weight)
    float4* spC;                  // its compensation
    // Result window of the render call: one entry per (pixel of the shard, pass of the window), PIXEL-major — entry
    // windowEntry(pixel, pass, P) = pixel x P + pass with P the pass count of the window being rendered (RenderParams::sppCount,
    // not the allocation's: the windows of a call may differ in P); RGB one float4, spectral four (the sixteen bins of
    // SpectrumStorage) — written once by the slot whose path was that sample.  The 64 slots of a k_shade wave hold consecutive
    // passes of one pixel (WorkItem below), so a wave's results and records are one contiguous run (1 KiB in RGB), and the passes
    // of a pixel that k_fold adds are contiguous too.  Then the sensor itself: per pixel the Kahan sum and its compensation
    // (CompensatedSum, BasicTypes/CompensatedSum.h:24-30), kept across the render calls of one slrhip_render_begin.
    // While a sample has not finished, its entry holds the primary pass's record of its camera ray instead ({triangle, t, b1, b2}:
    // the whole RGB entry, the first float4 of a spectral one; RenderParams::primary) and primaryInstance[entry] the instance of
    // that hit (instanced scenes only, else nullptr).
    float4* results;
    int32_t* primaryInstance;
    float4* fbSum;
    float4* fbComp;
    float4* nee;                  // pending next-event contribution
    float4* shadowDir;            // shadow ray direction, w = distMax
    float* pdfPrev;               // spectral mode only: the scalar that rides in alpha.w in RGB mode
    // per-slot sample header, written when a sample starts: x = the sample's pixel (index into the shard's pixel list), y = its
    // camera weight (bits), z = its wavelength offset (bits; lambda_i = 360 + 470 (i + offset) / 16, spectral mode), w = its pass
    // relative to the first pass of the window
    uint4* hdr;
    uint32_t* flags;
    // Work queues (WorkItem below): per wave of the shade kernel (64 slots) the number of samples it has taken from its queue so
    // far.  Read and advanced by that wave alone in k_shade (no atomics); by atomics in the tail kernel, where the slots of a
    // wave may be held by lanes of several waves.
    uint32_t* cursor;
    uint32_t* visible;            // result of the shadow ray
    uint32_t* shadowQueue;        // kShards regions of shardCapacity slot indices: shadow rays of this iteration
    uint32_t* tailList;           // tail mode: the live slots, listed by k_tail_collect (numSlots entries)
    uint32_t* queueCount;         // [parity][kind][shard], see queueCounterIndex
    // Live slots.  A slot that finds its queue exhausted goes idle; k_shade counts them per workgroup and adds the count to one of
    // kShards words on separate lines (idleShards: the queues run out at about the same iteration everywhere, and ~10^5 atomics
    // per launch on ONE word would cost a millisecond each time).  Every workgroup of the traversal launch that follows sums the
    // shards (liveSlots below) for the tail-mode decision; its first workgroup publishes the sum in activeSlots[0] for the next
    // k_shade launch (which only asks "is anything left?") and for the host.
    uint32_t* activeSlots;
    uint32_t* idleShards;         // [kShards] x kCounterStride words
    // one word per block of 256 consecutive slots: set by k_shade once every slot of the block has run out of passes (a slot
    // never leaves ST_IDLE within a render call), cleared by k_reset_slots; the scanning kernels skip such blocks without
    // touching their state — the last iterations of a render, in which a few long paths are left, then cost launch overhead
    uint32_t* blockDead;
    uint32_t* errorWord;          // ERR_* bits, sticky until the next slrhip_render call; read back with activeSlots
    // The end of a render call (pt_tail_kernels.h): as soon as at most RenderParams::tailSlots slots are still live (a slot
    // goes idle only when its pixel has no pass left, so by then nearly every pixel is done), the traversal kernel of that
    // iteration raises tailMode (= 1 + the iteration's parity) instead of tracing: every later wavefront launch of the call is
    // a no-op and the host runs the tail kernels, which take each remaining path — and the passes the remaining pixels still
    // have to hand out — to the end in one launch.  tailWords = {list length, list cursor}.
    uint32_t* tailMode;
    uint32_t* tailWords;
    uint32_t* tailIdled;          // slots the tail kernel left idle: the host checks it against the list length (every listed slot must end idle)
    uint32_t* windowSamples;      // samples the queues handed out in this window (k_count_samples): the host checks it against pixels x passes
    uint64_t* totals;             // [kind][shard], see totalIndex
    const uint32_t* pixelXY;      // pixel-of-shard -> x | y << 16
    // Records that the same kernels touch at the same slots share a 32-byte sector when these strides are 2 (rayDir = rayOrg + 1,
    // spC = spR + 1, element index = slot x stride): a kernel that visits a fraction of the slots then moves one sector per
    // visited slot and pair instead of most sectors of two arrays.  1 = separate arrays.
    uint32_t rayStride, spStride, hdrStride;      // hdrStride 2: rng = hdr + 1 (sample header + RNG state of a slot in one sector)
    // primaryRng[entry], indexed like results: the sample's xorshift128 state after the camera draws, left by the primary pass's producer
    // for the fused start of k_shade (windows with a primary pass only, else nullptr).  The last member: every other one keeps the
    // offset it had in the kernels' argument block, so the kernels that do not read it are compiled as they were.
    uint4* primaryRng;
};

struct RenderParams {
    uint32_t numSlots;            // 256 x shade workgroups
    uint32_t traceAllShadows;     // SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS or _COUNT_TRAVERSAL: k_shade's RGB kernels trace dead light samples too
    uint32_t numPixels, stripes;  // stripes: slots per pixel the slot count was sized for (slrhip_config::stripes or the automatic choice)
    uint32_t sppBegin, sppCount;  // the passes of the current window
    uint32_t workItems;           // numPixels x sppCount (< 2^32: slrhip_render sizes the windows)
    uint32_t numWaves;            // numSlots / 64: the owners of the work queues
    uint32_t runLength;           // passes per run (divides sppCount)
    uint32_t numRuns;             // runs of the window = numPixels x sppCount / runLength
    int32_t rngSeed;
    float timeStart, timeEnd;
    uint32_t imageWidth, imageHeight;
    uint32_t countSlots;          // SLRHIP_FLAG_COUNT_TRAVERSAL: also count live slots per logic launch
    uint32_t shardCapacity;       // entries per queue region = ceil(numBlocks / kShards) * 256
    uint32_t spectral;            // 0 = RGB (3 components), 1 = 16 wavelength samples
    uint32_t injectError;         // SLRHIP_FLAG_TEST_DEVICE_ERROR: the reset kernel raises the device error word
    uint32_t tailSlots;           // enter tail mode once at most this many slots are live; 0 = never
    uint32_t primary;             // 1: the window's camera rays were traced by the primary pass (launchPrimary) before its first iteration:
                                  // a sample starts from its record, in the launch that starts it (k_shade), and no slot is ever
                                  // left in ST_FIRST_HIT by k_shade; 0: startSample leaves the camera ray to k_trace_ws
};

// Work distribution.  An item is one sample, a (pixel, pass) pair.  The unit that is dealt out is a RUN: runLength consecutive
// passes of ONE pixel.  Run r = (pass group, pixel) with the pixel fastest; queues belong to WAVES of the shade kernel (64
// consecutive slots): the j-th run of wave w is run j x numWaves + (w + j x kWorkRotate) mod numWaves — every run belongs to
// exactly one wave, and the rotation walks each wave over the image, so that its queue is a sample of the whole frame and the
// queues carry the same work to within a few per cent.  The lanes of a wave that need a sample take the next items of the
// wave's queue in lane order, so the 64 slots of a wave hold passes of one pixel (two while it moves on): their camera rays are
// all but identical and their first bounces start in the same place, which is what keeps the lanes of a traversal wave in step
// (measured: with the slots of a wave spread over an 8 x 8 tile the traversal launch took 2.1 ms instead of 1.76).  Static
// queues need no global counter: one word that every wave bumps saturates near 88 atomics per microsecond (above).
static const uint32_t kWorkRotate = 40503u;
// The entry of sample (pixel, pass of the window) in a result window of windowPasses passes (PathBuffers::results, in entries;
// PathBuffers::primaryInstance, in words).  It does not depend on the pixel count: a window over a compact list
// (slrhip_render_adaptive) is laid out the same way.
__host__ __device__ inline size_t windowEntry(uint32_t pix, uint32_t passOfWindow, uint32_t windowPasses) {
    return (size_t)pix * windowPasses + passOfWindow;
}
// The entry of sample i of a primary-pass launch (launchPrimary below) relative to the launch's first entry, windowEntry(0, its first
// pass): the launch numbers the samples of its numPasses passes with the pass fastest, i = pixel x numPasses + pass of the launch,
// and the window keeps windowPasses (>= numPasses) entries a pixel.  A launch of the whole window: i itself.
__host__ __device__ inline size_t primaryLaunchEntry(uint32_t i, uint32_t numPasses, uint32_t windowPasses) {
    size_t entry = i;
    if (windowPasses != numPasses) entry += (size_t)(i / numPasses) * (windowPasses - numPasses);
    return entry;
}
struct WorkItem {
    uint32_t pix, pass;           // pass relative to RenderParams::sppBegin
    bool valid;                   // false: the queue is exhausted (every later item of this queue is invalid too)
};
__host__ __device__ inline uint32_t workRun(const RenderParams& rp, uint32_t wave, uint32_t j) {
    return j * rp.numWaves + (uint32_t)(((uint64_t)wave + (uint64_t)j * kWorkRotate) % rp.numWaves);
}
__host__ __device__ inline WorkItem workItemOf(const RenderParams& rp, uint32_t wave, uint32_t taken) {
    const uint32_t j = taken / rp.runLength, r = taken - j * rp.runLength;
    WorkItem w;
    w.pix = 0; w.pass = 0; w.valid = false;
    if (j > rp.numRuns / rp.numWaves) return w;                                      // (also keeps j x numWaves inside 32 bits)
    const uint32_t run = workRun(rp, wave, j);
    if (run >= rp.numRuns) return w;
    const uint32_t group = run / rp.numPixels;
    w.pix = run - group * rp.numPixels;
    w.pass = group * rp.runLength + r;
    w.valid = true;
    return w;
}
// Samples among the first `taken` items of a wave's queue (what k_count_samples adds up: a cursor runs past the end of its
// queue by the lanes that found nothing).
__host__ __device__ inline uint32_t workSamplesTaken(const RenderParams& rp, uint32_t wave, uint32_t taken) {
    uint32_t runs = 0;
    for (uint32_t j = 0; j <= rp.numRuns / rp.numWaves; ++j) if (workRun(rp, wave, j) < rp.numRuns) ++runs;
    const uint32_t length = runs * rp.runLength;
    return taken < length ? taken : length;
}

// Evaluated by every workgroup of the traversal launch of an iteration: its input is stable during that launch (activeSlots
// is written by k_shade only), so all workgroups agree; the first one records the decision for the kernels that follow.
__device__ __forceinline__ uint32_t liveSlots(const PathBuffers& pb, uint32_t numSlots) {
    uint32_t idle = 0;
#pragma unroll
    for (uint32_t k = 0; k < kShards; ++k) idle += pb.idleShards[k * kCounterStride];
    return numSlots - idle;
}
__device__ __forceinline__ bool tailModeBegins(const PathBuffers& pb, uint32_t live, uint32_t tailSlots, uint32_t parity) {
    if (tailSlots == 0u) return false;
    if (pb.tailMode[0]) return true;
    if (live > tailSlots) return false;
    if (blockIdx.x == 0 && threadIdx.x == 0) pb.tailMode[0] = 1u + parity;
    return true;
}

void launchResetSlots(const PathBuffers& pb, const RenderParams& rp, bool clearSensor, hipStream_t stream);
// The sample clamp of a render (slrhip_clamp_begin; pt_clamp.h).  records == nullptr: off.  One record per pixel of the shard:
// {clamped, dropped (uint32 bits), removed, largest}.
struct ClampParams {
    float4* records;
    float limit;
    uint32_t flags;               // SLRHIP_CLAMP_* bits
};
// ... as the fold kernels take it: nothing at all in the instantiations without a clamp
template <bool kClamp> struct FoldClampArgs {};
template <> struct FoldClampArgs<true> : ClampParams {};
// ImageSensor::add for the window's passes, in pass order: the result window folded into the per-pixel Kahan sums
// statRecords != nullptr (slrhip_statistics_begin): the instantiation that also updates the per-pixel noise records
// clamp.records != nullptr (slrhip_clamp_begin): the instantiation that puts every sample through clampSample first
void launchFold(const PathBuffers& pb, const RenderParams& rp, float4* statRecords, const ClampParams& clamp, hipStream_t stream);
// one wavefront iteration = launchShade(parity) then launchTraceWs(parity).  `v`: the window's k_shade instantiation (render_plan.h,
// planShadeVariant), looked up in the table of built kernels (pt_shade.hip); false: the table has no such row and nothing was launched
bool launchShade(const ShadeVariant& v, const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, hipStream_t stream);
void launchCountSamples(const PathBuffers& pb, const RenderParams& rp, hipStream_t stream);
// the rest of a render call in one launch (after tailMode was raised): list the live slots, then one lane per path to its end, with
// the k_tail twin of `v` (every k_shade row has one); false as above
bool launchTail(const ShadeVariant& v, const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t liveSlots, int numCUs, hipStream_t stream);
void launchResolve(const PathBuffers& pb, const RenderParams& rp, float* dst, hipStream_t stream);
void launchBsdfQueries(const DevScene& sc, bool spectral, uint32_t material, uint32_t n, const float* in, float wlOffset, uint32_t wl,
                       float4* geo, float4* misc, float4* fsSample, float4* fsEval, hipStream_t stream);
// closest-hit ray queries (slrhip_trace_rays): one lane per ray, 64-ray batches (pt_trace.hip)
void launchTraceBatch(const DevScene& sc, const float4* org, const float4* dir, float4* out, uint32_t n, hipStream_t stream);
// wave-specialised traversal (pt_trace_ws.hip): ONE launch for the extension and the shadow rays of an iteration
void launchTraceWs(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, uint32_t blocks, bool count,
                   hipStream_t stream);
int traceWsBlocksPerCU(bool quantizedTree);
// The primary pass of a render window (pt_trace_indexed.hip, WsPrimaryIO): the camera ray of every sample of the passes
// [firstPass, firstPass + numPasses) of the window (relative to rp.sppBegin) through the wave-specialised consumer, made on the spot
// by the producer wave; the hit record goes to the sample's entry of the result window (PathBuffers::results, primaryInstance),
// errors to the render's error word, the ray count to T_EXT_RAYS.  numPixels x numPasses < 2^31 (render_plan.h, planPrimary).
// `kernel` is the plan's choice (render_plan.h, PrimaryPlan::kernel), made on the host: the ring kernel above, or the direct kernel
// (pt_primary_direct.hip, launchPrimaryDirect: one lane makes, traces and stores one sample; scenes without instances on the float
// nodes only).  Same records, same streams, same count, to the bit.
void launchPrimary(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t firstPass, uint32_t numPasses, PrimaryKernel kernel,
                   int numCUs, hipStream_t stream);
// records / streams: the entry of (pixel 0, firstPass) of the window; streams may be nullptr (no plane)
void launchPrimaryDirect(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t firstPass, uint32_t numPasses, float4* records,
                         uint4* streams, int numCUs, hipStream_t stream);
// ray queries (slrhip_intersect_rays / slrhip_test_visibility) through the same consumer (pt_trace_indexed.hip): rays = n slrhip_ray records (2 x float4);
// visible == nullptr: closest hit into hits (slrhip_hit) and, if given, instances; else visibility into visible.  n < 2^31.
void launchQueryWs(const DevScene& sc, const float4* rays, uint32_t n, float4* hits, int32_t* instances, uint32_t* visible, uint32_t* errorWord,
                   int numCUs, hipStream_t stream);

// First-hit feature pass (slrhip_render_features; pt_features.hip, traversal: pt_trace_indexed.hip): the passes [passBegin, passBegin + numPasses) of every pixel of
// the shard in one launch.  records: numPixels x numPasses float4 {triangle, instance, dist, b1}, pass-major; b2: as many floats,
// or nullptr when no vector channel is asked for (see WsFeatureIO).
struct FeatureParams {
    const uint32_t* pixelXY;      // pixel-of-shard -> x | y << 16 (the render's list)
    float4* records;
    float* b2;
    uint32_t* errorWord;          // ERR_* bits of the feature passes, sticky since slrhip_render_begin
    uint32_t numPixels, numPasses, passBegin;
    uint32_t channels;            // SLRHIP_FEATURE_* bits of this call
    int32_t rngSeed;
    float timeStart, timeEnd;
    uint32_t imageWidth, imageHeight;
};
// per pixel of the shard: plain float32 sums in pass order; .w of the three: distance, coverage, unused
struct FeatureSums {
    float4* geometric;
    float4* shading;
    float4* tangent;
    uint4* ids;                   // triangle, instance, material of the highest pass rendered so far
};
void launchFeatures(const DevScene& sc, const FeatureParams& fp, const FeatureSums& sums, uint32_t idsPass, int numCUs, hipStream_t stream);
void launchCameraRays(const DevScene& sc, const FeatureParams& fp, float4* rays, uint32_t* pixelXY, hipStream_t stream);
// slrhip_debug_camera_draws (pt_features.hip): n tuples (seed, x, y, pass) in, 16 words each out (DEVICE memory)
void launchCameraDraws(uint32_t n, const uint4* tuples, uint32_t* out, hipStream_t stream);
void launchFeatureResolve(const FeatureParams& fp, const FeatureSums& sums, uint32_t channel, void* dst, hipStream_t stream);
// the traversal half of launchFeatures alone: the window's records, and b2 when fp.b2 is given
void launchFeatureTrace(const DevScene& sc, const FeatureParams& fp, int numCUs, hipStream_t stream);

// The albedo feature buffer (slrhip_render_albedo; pt_albedo.hip): launchFeatureTrace fills the record window, launchAlbedoFold adds
// the base colour of each hit (a miss: one) to the pixel in pass order.  sums: `components` float planes of numPixels floats each.
// fp.b2 must be given when the scene has textures (the texture coordinate needs both barycentrics).
void launchAlbedoFold(const DevScene& sc, const FeatureParams& fp, bool spectral, float* sums, hipStream_t stream);
// the sums as [height][width][components] (dst cleared by the caller: pixels outside the shard stay 0)
void launchAlbedoResolve(const FeatureParams& fp, uint32_t components, const float* sums, float* dst, hipStream_t stream);
// slrhip_modulate (pt_albedo.hip): one launch on `stream`; the descriptor has passed modulateRefusal (render_plan.h)
void launchModulate(const slrhip_modulate_desc& d, hipStream_t stream);

// slrhip_reproject (pt_reproject.hip): one launch on `stream`; the descriptor has passed reprojectRefusal (render_plan.h)
void launchReproject(const slrhip_reproject_desc& d, hipStream_t stream);
// (the motion pass, slrhip_render_motion: launchFeatureTrace, then pt_motion.h's launchMotionFold)

// Per-pixel noise statistics (slrhip_statistics_begin; pt_stats.hip). One record per pixel of the shard, updated by k_fold in
// pass order: {mean, M2, n (uint32 bits), max} of the samples' luminance (float32 Welford).
static const uint32_t kStatsBlock = 256;                   // threads per block of the summary's first stage
static const uint32_t kStatsPixelsPerThread = 16;          // a block reduces kStatsBlock x kStatsPixelsPerThread consecutive pixels
struct StatsTotals {                                       // slrhip_statistics_summary's layout (checked in slrhip_buffers.hip)
    uint64_t pixels, samples;
    double sumMean, sumMeanSq, sumVarianceOfMean;
    float maxSample;
    uint32_t pad;
};
inline uint32_t statsSummaryBlocks(uint32_t numPixels) { return (numPixels + kStatsBlock * kStatsPixelsPerThread - 1) / (kStatsBlock * kStatsPixelsPerThread); }
// The clamp records (slrhip_clamp_begin) have the shape of the noise records and the same two read-outs, with the summary's grid.
struct ClampTotals {                                       // slrhip_clamp_summary's layout (checked in slrhip_buffers.hip)
    uint64_t clamped, dropped;
    double removed;
    float largest;
    uint32_t pad;
};
// The read-outs of either record kind, named by its totals struct (StatsTotals, ClampTotals; pt_stats.hip instantiates both).
// One SLRHIP_STATISTICS_* / SLRHIP_CLAMP_* channel as [height][width] floats (dst cleared by the caller: pixels outside the shard stay 0):
template <typename Totals>
void launchRecordResolve(const float4* records, const uint32_t* pixelXY, uint32_t numPixels, uint32_t imageWidth, uint32_t channel, float* dst,
                         hipStream_t stream);
// the shard's totals, in double, in a fixed order: partials[statsSummaryBlocks(numPixels)], then *out (both DEVICE memory)
template <typename Totals>
void launchRecordSummary(const float4* records, uint32_t numPixels, Totals* partials, Totals* out, hipStream_t stream);

// Adaptive sampling (slrhip_render_adaptive; pt_adaptive.hip).  The pixels that have not retired are a compact list in ascending
// shard-pixel order: activeXY (x | y << 16: what a window over the list hands the kernels as PathBuffers::pixelXY) and activeIndex
// (compact index -> pixel of the shard: where the indexed fold adds).  After a block of passes the check reads the noise records
// of the previous list's pixels and writes the next list: per-workgroup counts (wave ballots), an exclusive scan of the counts,
// a scatter — a stable compaction without atomics, so the order (neighbouring pixels in neighbouring runs: WorkItem above) and the
// run are reproducible.  Two list buffers alternate; the work is proportional to the previous list's length.
static const uint32_t kAdaptiveBlock = 256;                // entries of the previous list per workgroup
inline uint32_t adaptiveSelectBlocks(uint32_t count) { return (count + kAdaptiveBlock - 1) / kAdaptiveBlock; }
struct AdaptiveSelect {
    const float4* records;        // the noise records, per pixel of the shard
    const uint32_t* shardXY;      // the shard's pixel list (slrhip_render_begin)
    const uint32_t* prevIndex;    // the previous list; nullptr = every pixel of the shard (before the first check)
    uint32_t prevCount;
    uint32_t* nextXY;             // the next list: at least prevCount entries each
    uint32_t* nextIndex;
    uint32_t* blockOffsets;       // adaptiveSelectBlocks(prevCount) words: the counts, then their exclusive scan
    uint32_t* countWord;          // the next list's length
    float threshold, floor;       // slrhip_adaptive_target
};
void launchAdaptiveSelect(const AdaptiveSelect& a, hipStream_t stream);
// launchFold (with statistics) for a window over a compact list: rp.numPixels = the list's length, pb.fbSum / fbComp and
// statRecords are the shard's, compact pixel i adds into pixel indexMap[i]
void launchFoldIndexed(const PathBuffers& pb, const RenderParams& rp, float4* statRecords, const uint32_t* indexMap, const ClampParams& clamp,
                       hipStream_t stream);
// the frame as per-pixel means: sum / (float)n with n of the pixel's record, 0 where n == 0 (dst cleared by the caller)
void launchResolveMean(const PathBuffers& pb, const RenderParams& rp, const float4* records, float* dst, hipStream_t stream);

// The denoiser (slrhip_denoise; pt_denoise.hip): the filter of include/slrhip.h over the caller's buffers.  The scratch
// (render_plan.h: denoiseScratchBytes) holds, per pixel, one guide record {n.x, n.y, n.z, z} (a miss: n.x = -INFINITY), two {Y, v}
// records and two colour records (one float4 for 3 components, four for 16) that the iterations alternate between.
struct DenoiseParams {
    uint32_t width, height, components, iterations;
    const float* color; const float* variance; const float* normal; const float* distance; const float* coverage;
    float* output; float* outputVariance;
    float sigmaLuminance, sigmaDistance;
    uint32_t normalPowerLog2;
    float4* guides; float2* yv[2]; float4* planes[2];      // the scratch, cut up by the caller
};
// one prepare launch and `iterations` filter launches on `stream`
void launchDenoise(const DenoiseParams& dp, hipStream_t stream);

// The image export (slrhip_tonemap; pt_tonemap.hip): one launch on `stream`; the descriptor has passed tonemapRefusal (render_plan.h).
void launchTonemap(const slrhip_tonemap_desc& d, hipStream_t stream);

} // namespace slrhip
