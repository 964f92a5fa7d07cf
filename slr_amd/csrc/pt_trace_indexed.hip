// pt_trace_indexed.hip — the index-fed clients of the wave-specialised consumer (pt_trace_ws.h): launches whose rays are numbered
// 0 .. n-1.  One kernel, k_ring_ws, and one launcher, launchRingWs; a client says what ray an index is and where its result goes:
//
//   WsQueryIO    ray queries (slrhip_intersect_rays / slrhip_test_visibility): index = entry of the caller's slrhip_ray array
//   WsFeatureIO  the first-hit trace of the feature, albedo and motion passes: index = sample of the window, camera ray made on the spot
//   WsPrimaryIO  the primary pass of a render window: the same producer, the path tracer's own hit record — on instanced scenes,
//                on the quantized tree and with SLRHIP_FLAG_PRIMARY_RING; elsewhere the plan (render_plan.h) names the direct kernel of
//                pt_primary_direct.hip, where the lane that traces a camera ray makes it, and launchPrimary below hands the launch over
//
// A client is a by-value kernel argument, plain data, with
//   errorWord()              the ERR_* word of its API family
//   tag()                    0, or kShadowBit: the rays are visibility (any-hit) rays
//   makeRay(sc, i, o, d)     ray i as ring entry {org, tmin}, {dir, tmax}; called by the producer wave
//   produced(rays)           called by the producer wave with the number of rays its workgroup appended
//   finish<INST>(i, hit...)  called by the consumer lane that finished ray i (the ring's slot word: i | tag())
#include <hip/hip_runtime.h>

#include "pt_camera.h"
#include "pt_trace_ws.h"

namespace slrhip {

// Results in the public format.  visible == nullptr: closest hit into hits and, if given, instances; else visibility into visible.
struct WsQueryIO {
    const float4* rays;           // slrhip_ray: {org, dist_min}, {dir, dist_max}
    float4* hits;                 // slrhip_hit: {triangle, dist, b0, b1}
    int32_t* instances;           // or nullptr
    uint32_t* visible;
    uint32_t* error;              // the context's query error word (not the render's)
    __device__ __forceinline__ uint32_t* errorWord() const { return error; }
    __device__ __forceinline__ uint32_t tag() const { return visible ? kShadowBit : 0u; }
    __device__ __forceinline__ void makeRay(const DevScene&, uint32_t i, float4& o, float4& d) const {
        o = ntLoad4(&rays[2 * (size_t)i]);
        d = ntLoad4(&rays[2 * (size_t)i + 1]);
    }
    __device__ __forceinline__ void produced(uint32_t) const {}
    template <bool INST>
    __device__ __forceinline__ void finish(uint32_t slot, uint32_t hitTri, float hitT, float hitB1, float hitB2, int32_t hitInst) const {
        if (slot & kShadowBit) { visible[slot & ~kShadowBit] = hitTri == 0xFFFFFFFFu ? 1u : 0u; return; }
        // Intersection::u = 1 - b1 - b2, ::v = b1 (TriangleMesh.cpp:159,172-173), in that float order; zeros on a miss as
        // slrhip_trace_rays reports them
        const bool miss = hitTri == 0xFFFFFFFFu;
        const float b0 = 1.0f - hitB1 - hitB2;
        hits[slot] = make_float4(__uint_as_float(hitTri), hitT, miss ? 0.0f : b0, miss ? 0.0f : hitB1);
        if (instances) instances[slot] = hitInst;       // -1: a loose triangle or a miss (always -1 when the scene has no instance)
    }
};

// A ring entry is a sample of the launch's window, index = pass of the window x pixels of the shard + pixel of the shard (< 2^31:
// the host sizes the windows).  The producer wave GENERATES the camera ray of each index into the LDS ring — the path tracer's own
// draws and camera arithmetic (pt_camera.h) — so no ray array exists in HBM.  finish writes the hit record of the sample, as the
// query client does, plus the instance — the record plane {triangle, instance, dist, b1} and, when a vector channel is asked for,
// Moller-Trumbore's b2 in a float plane.  The surface point is computed by the fold kernel (k_feature_fold, pt_features.hip), one
// lane per pixel: with it inside `finish` (inlined at the two places a lane can finish) the instanced instantiation spilled 20
// registers and wrote 64 B per sample; measured in DESIGN.md 7.9.
struct WsFeatureIO {
    FeatureParams fp;
    __device__ __forceinline__ uint32_t* errorWord() const { return fp.errorWord; }      // the feature passes' own (not the render's, not the queries')
    __device__ __forceinline__ uint32_t tag() const { return 0u; }
    __device__ __forceinline__ void makeRay(const DevScene& sc, uint32_t i, float4& o, float4& d) const {
        uint32_t xy;
        featureCameraRay(sc.camera, fp, i, o, d, xy);
    }
    __device__ __forceinline__ void produced(uint32_t) const {}
    template <bool INST>
    __device__ __forceinline__ void finish(uint32_t slot, uint32_t hitTri, float hitT, float hitB1, float hitB2, int32_t hitInst) const {
        ntStore4(fp.records + slot, make_float4(__uint_as_float(hitTri), __uint_as_float((uint32_t)hitInst), hitT, hitB1));
        if (fp.b2) __builtin_nontemporal_store(hitB2, fp.b2 + slot);
    }
};

// The primary pass of a render window (launchPrimary, pt_kernels.h).  A camera ray is a function of (pixel, pass, seed) alone, so the
// first segment of every sample of a window is traced here, before the window's first iteration, instead of making a round trip
// through the slot state (startSample -> k_trace_ws -> k_shade).  A ring entry is a sample of the launch, index = pixel x passes of
// the launch + pass of the launch — the window's own order (windowEntry, pt_kernels.h), so consecutive ring entries are consecutive
// passes of one pixel: all but identical camera rays in a consumer wave, and consecutive record addresses.  finish writes
// {triangle, t, b1, b2} — what the render's client writes to PathBuffers::hit — to the sample's entry of the result window, which
// nobody else touches until the sample finishes (writeResult), and the instance to its plane.
// STREAMS: the producer also leaves every sample's stream behind the camera draws (PathBuffers::primaryRng) for the fused start of
// k_shade.  A template argument: the store and the four words kept for it cost the producer wave 48 B more scratch per lane, and where
// one producer feeds 15 consumers (large trees, instanced scenes) it is the pass's limit — there the plan keeps the plane off
// (render_plan.h) and the producer is the one it was.
template <bool STREAMS>
struct WsPrimaryIO {
    FeatureParams fp;             // the camera arguments of the launch; records = the entry of (pixel 0, the launch's first pass); errorWord = the render's
    int32_t* instances;           // that entry of PathBuffers::primaryInstance, or nullptr
    uint4* streams;               // that entry of PathBuffers::primaryRng
    uint64_t* totals;
    uint32_t stride;              // float4 per entry (RGB 1, spectral 4: the record is the first)
    uint32_t windowPasses;        // passes of the window (>= fp.numPasses, the launch's): the distance of two pixels' entries
    __device__ __forceinline__ uint32_t* errorWord() const { return fp.errorWord; }
    __device__ __forceinline__ uint32_t tag() const { return 0u; }
    __device__ __forceinline__ void makeRay(const DevScene& sc, uint32_t i, float4& o, float4& d) const {
        uint32_t xy;
        Rng after;
        primaryCameraRay(sc.camera, fp, i, o, d, xy, after);
        if constexpr (!STREAMS) return;
        // the stream behind the camera draws, for the launch of k_shade that starts the sample (its fused start goes on from here instead
        // of seeding again); the producer's lanes hold consecutive samples: 1 KiB contiguous per wave
        ntStore4(reinterpret_cast<float4*>(streams + primaryLaunchEntry(i, fp.numPasses, windowPasses)),
                 make_float4(__uint_as_float(after.s0), __uint_as_float(after.s1), __uint_as_float(after.s2), __uint_as_float(after.s3)));
    }
    // Scene::intersect of PathTracingRenderer.cpp:147, counted where it is traced: one atomic per workgroup
    __device__ __forceinline__ void produced(uint32_t rays) const {
        if (threadIdx.x == 0 && rays) atomicAdd((unsigned long long*)&totals[totalIndex(T_EXT_RAYS, blockIdx.x % kShards)], (unsigned long long)rays);
    }
    template <bool INST>
    __device__ __forceinline__ void finish(uint32_t slot, uint32_t hitTri, float hitT, float hitB1, float hitB2, int32_t hitInst) const {
        const size_t entry = primaryLaunchEntry(slot, fp.numPasses, windowPasses);
        ntStore4(fp.records + entry * stride, make_float4(__uint_as_float(hitTri), hitT, hitB1, hitB2));
        if (INST) __builtin_nontemporal_store(hitInst, instances + entry);
    }
};

template <int NC, bool QUANT, bool INST, class Client>
__global__ __launch_bounds__(64 * (NC + 1)) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_ring_ws(DevScene sc, Client client, uint32_t n, uint32_t refill) {
    __shared__ WsLds<NC> lds;
    wsResetRing(lds);
    WsCounts cnt;
    WsDebug dbg;
    if (threadIdx.x < 64)
        client.produced(wsProduceIndexed(n, client.tag(), client.errorWord(), lds, dbg, [&](uint32_t i, float4& o, float4& d) { client.makeRay(sc, i, o, d); }));
    else wsConsume<false, NC, QUANT, INST>(sc, client, lds, refill, cnt, dbg);
}

// n rays through nc consumer waves per workgroup.  The render's tree choice (launchTraceWs): instanced scenes have float nodes
// only, else the quantized nodes where the scene has them.  The grid: the resident workgroups, or one per 128-ray chunk if fewer.
template <class Client>
static void launchRingWs(const DevScene& sc, const Client& client, uint32_t n, int nc, int numCUs, hipStream_t stream) {
    const uint32_t chunks = (n + kSub * 64 - 1) / (kSub * 64);
    const dim3 grid(std::max(1u, std::min((uint32_t)numCUs * (uint32_t)wsBlocksPerCU(nc), chunks)));
    const uint32_t refill = wsTuning().refill;
    dispatchNc(nc, [&](auto c) {
        constexpr int NC = decltype(c)::value;
        const dim3 block(64 * (NC + 1));
        if (sc.instances) hipLaunchKernelGGL((k_ring_ws<NC, false, true, Client>), grid, block, 0, stream, sc, client, n, refill);
        else if (sc.nodesQ) hipLaunchKernelGGL((k_ring_ws<NC, true, false, Client>), grid, block, 0, stream, sc, client, n, refill);
        else hipLaunchKernelGGL((k_ring_ws<NC, false, false, Client>), grid, block, 0, stream, sc, client, n, refill);
    });
}
// the render's number of consumer waves for this scene's tree
static int sceneConsumers(const DevScene& sc) { return wsConsumers(sc.nodesQ != nullptr && !sc.instances); }

void launchQueryWs(const DevScene& sc, const float4* rays, uint32_t n, float4* hits, int32_t* instances, uint32_t* visible, uint32_t* errorWord,
                   int numCUs, hipStream_t stream) {
    launchRingWs(sc, WsQueryIO{rays, hits, instances, visible, errorWord}, n, sceneConsumers(sc), numCUs, stream);
}

// the traversal of a window alone: the records (and b2, if fp.b2 is given) of its samples; shared with the albedo and motion passes
void launchFeatureTrace(const DevScene& sc, const FeatureParams& fp, int numCUs, hipStream_t stream) {
    launchRingWs(sc, WsFeatureIO{fp}, fp.numPixels * fp.numPasses, sceneConsumers(sc), numCUs, stream);
}

template <bool STREAMS>
static void launchPrimaryWith(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t firstPass, uint32_t numPasses, int numCUs,
                              hipStream_t stream) {
    const uint32_t n = rp.numPixels * numPasses;
    WsPrimaryIO<STREAMS> io{};
    io.stride = rp.spectral ? 4u : 1u;
    io.windowPasses = rp.sppCount;
    const size_t first = windowEntry(0u, firstPass, rp.sppCount);
    io.fp.pixelXY = pb.pixelXY; io.fp.records = pb.results + first * io.stride; io.fp.errorWord = pb.errorWord;
    io.fp.numPixels = rp.numPixels; io.fp.numPasses = numPasses; io.fp.passBegin = rp.sppBegin + firstPass;
    io.fp.rngSeed = rp.rngSeed; io.fp.timeStart = rp.timeStart; io.fp.timeEnd = rp.timeEnd;
    io.fp.imageWidth = rp.imageWidth; io.fp.imageHeight = rp.imageHeight;
    io.instances = pb.primaryInstance ? pb.primaryInstance + first : nullptr;
    io.streams = STREAMS ? pb.primaryRng + first : nullptr;
    io.totals = pb.totals;
    // Consumers per producer.  Where k_trace_ws runs 7 (small trees) this pass runs 3: its producer wave seeds a stream and samples the
    // camera for every ray, a camera ray needs few nodes, and with 7 consumers the producer was the limit (headline frame: 306 ms
    // with 7, 294.5 ms with 3).  Quantized (large) trees and instanced scenes keep k_trace_ws's choice: not measured.
    static const int envNc = [] { const char* e = tuningEnv("SLRHIP_PRIMARY_NC"); return e ? atoi(e) : 0; }();      // measurement builds: 3 / 7 / 15
    const int ncTrace = sceneConsumers(sc);
    const int nc = envNc == 3 || envNc == 7 || envNc == 15 ? envNc : (ncTrace == 7 && !sc.instances ? 3 : ncTrace);
    launchRingWs(sc, io, n, nc, numCUs, stream);
}

void launchPrimary(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t firstPass, uint32_t numPasses, PrimaryKernel kernel,
                   int numCUs, hipStream_t stream) {
    const uint32_t n = rp.numPixels * numPasses;
    if (n == 0) return;
    if (kernel == PrimaryKernel::Direct) {
        // the plan's choice for scenes without instances on the float nodes (render_plan.h): the same entries of the same planes
        const size_t first = windowEntry(0u, firstPass, rp.sppCount);
        launchPrimaryDirect(sc, pb, rp, firstPass, numPasses, pb.results + first * (rp.spectral ? 4u : 1u), pb.primaryRng ? pb.primaryRng + first : nullptr,
                            numCUs, stream);
        return;
    }
    if (pb.primaryRng) launchPrimaryWith<true>(sc, pb, rp, firstPass, numPasses, numCUs, stream);
    else launchPrimaryWith<false>(sc, pb, rp, firstPass, numPasses, numCUs, stream);
}

} // namespace slrhip
