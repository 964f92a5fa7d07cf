// pt_primary_direct.hip — the primary pass of a render window with every camera ray made on the lane that traces it.
//
// The ring kernel of pt_trace_indexed.hip (k_ring_ws with WsPrimaryIO) exists for waves whose lanes need very different step counts:
// a producer wave makes the rays, they go through an LDS ring, and the consumer lanes take a new ray whenever theirs is finished.
// The primary pass numbers its samples with the pass fastest (primaryCameraRay, primaryLaunchEntry), so 64 consecutive indices are
// 64 passes of one pixel (two where a wave straddles pixels): rays that differ by the jitter inside the pixel and the lens position,
// walk almost the same nodes and finish almost together.  Here one lane takes one sample of the launch: it makes the camera ray
// (cameraRayOf: the same function, the same bits), stores the stream behind the camera draws, traces the ray with traverse()
// (pt_traverse.h: the slab, triangle and tie-rule functions wsConsume calls) in lock-step with its 63 neighbours and stores the
// record itself — no producer wave, no trip through LDS, none of the ring's per-step bookkeeping, and the records of a wave are one
// contiguous KiB as its streams are.  Scenes without instances on the float nodes only: traverse() has no quantized-node path, and on
// large or instanced trees the rays of a pixel part ways at the leaves (render_plan.h, planPrimary, keeps the ring kernel there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "pt_camera.h"
#include "pt_trace_ws.h"      // ntStore4
#include "pt_traverse.h"

namespace slrhip {

// what WsPrimaryIO carries, without the instance plane
struct PrimaryDirectIO {
    FeatureParams fp;             // the camera arguments of the launch; records = the entry of (pixel 0, the launch's first pass); errorWord = the render's
    uint4* streams;               // that entry of PathBuffers::primaryRng (STREAMS only)
    uint64_t* totals;
    uint32_t stride;              // float4 per entry (RGB 1, spectral 4: the record is the first)
    uint32_t windowPasses;        // passes of the window (>= fp.numPasses, the launch's): the distance of two pixels' entries
};

// the traversal stack of traverse(): kLdsStack entries per lane, [entry][lane]; no staged top nodes (8 KiB per workgroup)
struct PrimaryDirectLds {
    uint32_t stack[kLdsStack * kTraceBlock];
};

// One workgroup per 256-sample chunk of the launch; a wave takes 64 consecutive samples.  The two variants that were measured and not
// kept stay as template arguments for the measurement builds: PERSISTENT, resident workgroups striding over the chunks
// (the compiler then keeps the camera's loop-invariant products live across the traversal and spills 44 registers: slower than the ring
// kernel), and WAVE_PIXEL, for launches whose passes are a multiple of 64 — the 64 samples of a wave share a pixel and the index
// division is done once per wave (no measurable difference).  Both are launch-time choices of the host (launchPrimaryDirect).
template <bool STREAMS, bool PERSISTENT, bool WAVE_PIXEL>
__global__ __launch_bounds__(kTraceBlock) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_primary_direct(DevScene sc, PrimaryDirectIO io, uint32_t n) {
    __shared__ PrimaryDirectLds lds;
    uint32_t rays = 0;            // of the workgroup (uniform)
    // n < 2^31 and a resident grid's stride is under 2^24 samples: the chunk's first index stays inside 32 bits
    for (uint32_t base = blockIdx.x * kTraceBlock; base < n; base += gridDim.x * kTraceBlock) {
        rays += min(n - base, (uint32_t)kTraceBlock);
        const uint32_t i = base + threadIdx.x;
        if (i < n) {
            float4 o, d;
            size_t entry;
            {
                // primaryCameraRay's numbering (the pass fastest) and primaryLaunchEntry's arithmetic with one division for both; the
                // generation's registers are dead before the traversal starts
                const uint32_t pix = WAVE_PIXEL ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(i / io.fp.numPasses)) : i / io.fp.numPasses;
                const uint32_t pass = i - pix * io.fp.numPasses;
                uint32_t xy;
                Rng after;
                cameraRayOf(sc.camera, io.fp, pix, pass, o, d, xy, after);
                entry = (size_t)i + (size_t)pix * (io.windowPasses - io.fp.numPasses);
                // the stream behind the camera draws, for the launch of k_shade that starts the sample: 1 KiB contiguous per wave
                if constexpr (STREAMS)
                    ntStore4(reinterpret_cast<float4*>(io.streams + entry),
                             make_float4(__uint_as_float(after.s0), __uint_as_float(after.s1), __uint_as_float(after.s2), __uint_as_float(after.s3)));
            }
            HitRec hit;
            TravCount cnt;
            traverse<false, false, false>(sc, sc.nodes, sc.leafTris, nullptr, 0u, V3(o.x, o.y, o.z), V3(d.x, d.y, d.z), o.w, d.w, &hit,
                                          lds.stack + threadIdx.x, &cnt, io.fp.errorWord);
            // WsPrimaryIO::finish's record; a miss is traverse()'s initial {0xFFFFFFFF, inf, 0, 0}, as the consumer's is
            ntStore4(io.fp.records + entry * io.stride, make_float4(__uint_as_float(hit.tri), hit.t, hit.b1, hit.b2));
        }
        if (!PERSISTENT) break;
    }
    // Scene::intersect of PathTracingRenderer.cpp:147, counted where it is traced: one atomic per workgroup (WsPrimaryIO::produced)
    if (threadIdx.x == 0 && rays) atomicAdd((unsigned long long*)&io.totals[totalIndex(T_EXT_RAYS, blockIdx.x % kShards)], (unsigned long long)rays);
}

void launchPrimaryDirect(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t firstPass, uint32_t numPasses, float4* records,
                         uint4* streams, int numCUs, hipStream_t stream) {
    const uint32_t n = rp.numPixels * numPasses;
    if (n == 0) return;
    PrimaryDirectIO io{};
    io.stride = rp.spectral ? 4u : 1u;
    io.windowPasses = rp.sppCount;
    io.fp.pixelXY = pb.pixelXY; io.fp.records = records; io.fp.errorWord = pb.errorWord;
    io.fp.numPixels = rp.numPixels; io.fp.numPasses = numPasses; io.fp.passBegin = rp.sppBegin + firstPass;
    io.fp.rngSeed = rp.rngSeed; io.fp.timeStart = rp.timeStart; io.fp.timeEnd = rp.timeEnd;
    io.fp.imageWidth = rp.imageWidth; io.fp.imageHeight = rp.imageHeight;
    io.streams = streams;
    io.totals = pb.totals;
    const dim3 grid((n + kTraceBlock - 1) / kTraceBlock), block(kTraceBlock);      // at most 2^23 workgroups
#ifdef SLR_TUNING_KNOBS
    // measurement builds: SLRHIP_PRIMARY_DIRECT = persistent | wavepixel
    static const std::string variant = [] { const char* e = tuningEnv("SLRHIP_PRIMARY_DIRECT"); return std::string(e ? e : ""); }();
    if (variant == "persistent") {
        const dim3 resident(std::min((uint32_t)numCUs * 8u, grid.x));       // 8 waves per SIMD: 8 workgroups of 4 waves per CU
        if (streams) hipLaunchKernelGGL((k_primary_direct<true, true, false>), resident, block, 0, stream, sc, io, n);
        else hipLaunchKernelGGL((k_primary_direct<false, true, false>), resident, block, 0, stream, sc, io, n);
        return;
    }
    if (variant == "wavepixel" && numPasses % 64u == 0u) {
        if (streams) hipLaunchKernelGGL((k_primary_direct<true, false, true>), grid, block, 0, stream, sc, io, n);
        else hipLaunchKernelGGL((k_primary_direct<false, false, true>), grid, block, 0, stream, sc, io, n);
        return;
    }
#endif
    if (streams) hipLaunchKernelGGL((k_primary_direct<true, false, false>), grid, block, 0, stream, sc, io, n);
    else hipLaunchKernelGGL((k_primary_direct<false, false, false>), grid, block, 0, stream, sc, io, n);
}

} // namespace slrhip
