// pt_shade.hip — the table of built k_shade / k_tail kernels and launchShade, the launchers of the shading half's small kernels
// (gfx950, wave64) and those kernels: k_reset_slots, k_resolve, k_bsdf_queries, k_count_samples, k_fold.  k_shade itself is in
// pt_shade_kernels.h, its instantiations in pt_shade_{rgb,spec16,multi*,tex*}.hip.
#include <algorithm>
#include <type_traits>

#include "pt_bsdf.h"
#include "pt_bsdf_multi.h"
#include "pt_fold.h"
#include "pt_shade_tables.h"
#include "pt_shade_variants.h"
#include "pt_slot_state.h"
#include "pt_tex_spectrum.h"

namespace slrhip {

// ---- the table of built kernels: every k_shade and every k_tail of the library, each named once -------------------------------------
// A row is the instantiation's template arguments, read as a ShadeVariant, and the function that returns the kernel (pt_shade_variants.h;
// the translation unit named on the right builds it).  planShadeVariant (render_plan.cpp) chooses, the launchers below look up.
namespace {

struct ShadeRow { ShadeVariant v; ShadeKernel (*kernel)(); };
struct TailRow { ShadeVariant v; TailKernel (*kernel)(); };
template <class S, bool LDS_TABLES, bool MF, bool MULTI = false, bool TEX = false, bool PRIMARY = false, bool RESUME = false>
constexpr ShadeRow shadeRow() {
    return {{std::is_same<S, Spec16>::value, LDS_TABLES, MF, MULTI, TEX, PRIMARY, RESUME}, &shadeKernel<S, LDS_TABLES, MF, MULTI, TEX, PRIMARY, RESUME>};
}
template <class S, bool LDS_TABLES, bool MF, bool MULTI = false, bool TEX = false>
constexpr TailRow tailRow() {
    return {{std::is_same<S, Spec16>::value, LDS_TABLES, MF, MULTI, TEX, false, false}, &tailKernel<S, LDS_TABLES, MF, MULTI, TEX>};
}

//           mode, LDS tables, glossy lobes, MultiBSDF, textures, PRIMARY, RESUME
const ShadeRow kShadeRows[] = {
    shadeRow<RGB, true, false>(), shadeRow<RGB, true, true>(), shadeRow<RGB, false, false>(), shadeRow<RGB, false, true>(),      // pt_shade_rgb.hip
    shadeRow<RGB, true, false, false, false, true, true>(), shadeRow<RGB, true, true, false, false, true, true>(),                // pt_shade_rgb_primary.hip
    shadeRow<RGB, false, false, false, false, true, true>(), shadeRow<RGB, false, true, false, false, true, true>(),
    shadeRow<RGB, true, false, false, false, true>(), shadeRow<RGB, true, true, false, false, true>(),                            // pt_shade_rgb_primary_seeded.hip
    shadeRow<RGB, false, false, false, false, true>(), shadeRow<RGB, false, true, false, false, true>(),
    shadeRow<Spec16, true, false>(), shadeRow<Spec16, true, true>(), shadeRow<Spec16, false, false>(), shadeRow<Spec16, false, true>(),      // pt_shade_spec16.hip
    shadeRow<RGB, false, true, true>(),                                   // pt_shade_multi_rgb.hip
    shadeRow<RGB, false, true, true, false, true, true>(),                // pt_shade_multi_rgb_primary.hip
    shadeRow<RGB, false, true, true, false, true>(),                      // pt_shade_multi_rgb_primary_seeded.hip
    shadeRow<Spec16, false, true, true>(),                                // pt_shade_multi_spec.hip
    shadeRow<RGB, false, true, true, true>(),                             // pt_shade_tex_rgb.hip
    shadeRow<RGB, false, true, true, true, true, true>(),                 // pt_shade_tex_rgb_primary.hip
    shadeRow<RGB, false, true, true, true, true>(),                       // pt_shade_tex_rgb_primary_seeded.hip
    shadeRow<Spec16, false, true, true, true>(),                          // pt_shade_tex_spec.hip
};
const TailRow kTailRows[] = {
    tailRow<RGB, true, false>(), tailRow<RGB, true, true>(), tailRow<RGB, false, false>(), tailRow<RGB, false, true>(),                  // pt_tail_rgb.hip
    tailRow<Spec16, true, false>(), tailRow<Spec16, true, true>(), tailRow<Spec16, false, false>(), tailRow<Spec16, false, true>(),      // pt_tail_spec16.hip
    tailRow<RGB, false, true, true>(),                                    // pt_tail_multi_rgb.hip
    tailRow<Spec16, false, true, true>(),                                 // pt_tail_multi_spec.hip
    tailRow<RGB, false, true, true, true>(),                              // pt_tail_tex_rgb.hip
    tailRow<Spec16, false, true, true, true>(),                           // pt_tail_tex_spec.hip
};

} // namespace

ShadeKernel findShadeKernel(const ShadeVariant& v) {
    for (const ShadeRow& r : kShadeRows)
        if (r.v == v) return r.kernel();
    return nullptr;
}
TailKernel findTailKernel(const ShadeVariant& v) {
    for (const TailRow& r : kTailRows)
        if (r.v == v) return r.kernel();
    return nullptr;
}

bool launchShade(const ShadeVariant& v, const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, hipStream_t stream) {
    const ShadeKernel kernel = findShadeKernel(v);
    if (!kernel) return false;
    hipLaunchKernelGGL(kernel, dim3(rp.numSlots / kShadeBlock), dim3(kShadeBlock), 0, stream, sc, pb, rp, parity);
    return true;
}

// Start of a render window: every slot wants a sample (ST_REGEN), the queues are at their beginning.  `clearSensor`: the first
// window after slrhip_render_begin also zeroes the sensor (later calls continue the image, like ImageSensor::add does).
template <class S>
__global__ void k_reset_slots(PathBuffers pb, RenderParams rp, uint32_t clearSensor) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;     // blockDim == kShadeBlock, numSlots = 256 x gridDim
    pb.flags[slot] = F_MAKE((uint32_t)ST_REGEN, 0u, 0u, 0u, 0u, 0u);
    pb.hdr[(size_t)slot * pb.hdrStride] = make_uint4(0u, 0u, 0u, 0u);
    pb.visible[slot] = 0;
    if (threadIdx.x == 0) pb.blockDead[blockIdx.x] = 0u;
    if ((threadIdx.x & 63u) == 0u) pb.cursor[slot >> 6] = 0u;
    if (clearSensor) {
        constexpr uint32_t planes = S::N == 3 ? 1u : 4u;
        for (size_t e = slot; e < (size_t)rp.numPixels * planes; e += (size_t)gridDim.x * blockDim.x) {
            pb.fbSum[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            pb.fbComp[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    if (blockIdx.x == 0) {
        for (uint32_t k = threadIdx.x; k < 2 * kQueueSetWords; k += blockDim.x) pb.queueCount[k] = 0;
        if (threadIdx.x < kShards) pb.idleShards[threadIdx.x * kCounterStride] = 0u;
        if (threadIdx.x == 0) {
            pb.activeSlots[0] = rp.numSlots; pb.errorWord[0] = rp.injectError ? ERR_QUEUE_OVERFLOW : 0u;
            pb.tailMode[0] = 0u; pb.tailWords[0] = 0u; pb.tailWords[1] = 0u; pb.tailIdled[0] = 0u; pb.windowSamples[0] = 0u;
        }
    }
}

// ImageSensor read-out: [H][W][N] linear sums.
template <class S>
__global__ void k_resolve(PathBuffers pb, RenderParams rp, float* dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= rp.numPixels) return;
    const uint32_t xy = pb.pixelXY[pix];
    const uint32_t px = xy & 0xFFFFu, py = xy >> 16;
    float* o = dst + ((size_t)py * rp.imageWidth + px) * S::N;
    if (S::N == 3) {
        const float4 v = pb.fbSum[pix];
        o[0] = v.x; o[1] = v.y; o[2] = v.z;
    }
    else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 v = pb.fbSum[(size_t)pix * 4 + k];
            o[4 * k] = v.x; o[4 * k + 1] = v.y; o[4 * k + 2] = v.z; o[4 * k + 3] = v.w;
        }
    }
}

// Diagnostic (slrhip_bsdf_queries): the three BSDF entry points exactly as logicSlot calls them, one query per lane.
// geo[i] = (sampled dir_sn, dirPDF); misc[i] = (dirType, evaluatePDF, 0, 0); fsSample / fsEval in the SpecIO layout.
template <class S>
__global__ void __launch_bounds__(64) k_bsdf_queries(DevScene sc, uint32_t material, uint32_t n, const float* __restrict__ in, float wlOffset,
                                                     uint32_t wl, float4* __restrict__ geo, float4* __restrict__ misc,
                                                     float4* __restrict__ fsSample, float4* __restrict__ fsEval) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + 12 * (size_t)i;
    Mat<S> m = MatIO<S>::template load<false>(sc, nullptr, material, wlOffset);
    if (m.type & kMatTexturedBit) (void)texturizeMat<S>(sc, m, material, 0.0f, 0.0f, wlOffset);     // textures at texCoord (0, 0)
    const V3 dirOut(q[0], q[1], q[2]), gNorm(q[3], q[4], q[5]), dirIn(q[6], q[7], q[8]);
    BsdfSample bs;
    bs.dir_sn = V3(0, 0, 0);
    S fs, fe;
    float pdf;
    if (m.type == SLRHIP_MATERIAL_MULTI) {
        const auto loadComponent = [&](uint32_t idx) {
            Mat<S> cm = MatIO<S>::template load<false>(sc, nullptr, idx, wlOffset);
            if (cm.type & kMatTexturedBit) (void)texturizeMat<S>(sc, cm, idx, 0.0f, 0.0f, wlOffset);
            return cm;
        };
        const MultiBSDF<S, decltype(loadComponent)> multi = {buildMultiTree<S>(decodeMulti(m), loadComponent), 0u, loadComponent};
        const uint32_t type = multiType(multi.tr, 0u);
        fs = multi.sample(type, dirOut, gNorm, wl, q[9], q[10], q[11], &bs);
        fe = multi.evaluate(type, dirOut, gNorm, dirIn, wl, &pdf);
    }
    else {
        const uint32_t type = bsdfType(m.type, 0u);
        fs = bsdfSample<S, true>(m, type, dirOut, gNorm, wl, q[9], q[10], q[11], &bs);
        fe = bsdfEvaluate<S, true>(m, type, dirOut, gNorm, dirIn, wl, &pdf);
    }
    if (bs.dirPDF == 0.0f) { bs.dir_sn = V3(0, 0, 0); bs.dirType = 0; fs = S(); }
    geo[i] = make_float4(bs.dir_sn.x, bs.dir_sn.y, bs.dir_sn.z, bs.dirPDF);
    misc[i] = make_float4((float)bs.dirType, pdf, 0.0f, 0.0f);
    SpecIO<S>::store(fsSample, nullptr, i, n, fs, 0.0f);
    SpecIO<S>::store(fsEval, nullptr, i, n, fe, 0.0f);
}

void launchResetSlots(const PathBuffers& pb, const RenderParams& rp, bool clearAcc, hipStream_t stream) {
    const dim3 grid(rp.numSlots / kShadeBlock), block(kShadeBlock);
    if (rp.spectral) hipLaunchKernelGGL(k_reset_slots<Spec16>, grid, block, 0, stream, pb, rp, clearAcc ? 1u : 0u);
    else hipLaunchKernelGGL(k_reset_slots<RGB>, grid, block, 0, stream, pb, rp, clearAcc ? 1u : 0u);
}
void launchBsdfQueries(const DevScene& sc, bool spectral, uint32_t material, uint32_t n, const float* in, float wlOffset, uint32_t wl,
                       float4* geo, float4* misc, float4* fsSample, float4* fsEval, hipStream_t stream) {
    const dim3 grid((n + 63) / 64), block(64);
    if (spectral) hipLaunchKernelGGL(k_bsdf_queries<Spec16>, grid, block, 0, stream, sc, material, n, in, wlOffset, wl, geo, misc, fsSample, fsEval);
    else hipLaunchKernelGGL(k_bsdf_queries<RGB>, grid, block, 0, stream, sc, material, n, in, wlOffset, wl, geo, misc, fsSample, fsEval);
}
// Samples rendered in the window that just ended = what the waves took from their queues (PathBuffers::cursor, capped at
// the queue's length: a cursor runs past the end by the lanes that found nothing).  This is the device's own account of the
// work handed out — the host's numPixels x passes would be a tautology.  One atomic per workgroup on the sharded totals.
__global__ __launch_bounds__(kShadeBlock) void k_count_samples(PathBuffers pb, RenderParams rp) {
    __shared__ uint32_t red[kShadeBlock / 64];
    uint32_t n = 0;
    for (uint32_t w = blockIdx.x * kShadeBlock + threadIdx.x; w < rp.numWaves; w += gridDim.x * kShadeBlock) n += workSamplesTaken(rp, w, pb.cursor[w]);
    for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off);
    if ((threadIdx.x & 63u) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kShadeBlock / 64; ++w) t += red[w];
        if (t) {
            atomicAdd((unsigned long long*)&pb.totals[totalIndex(T_SAMPLES, blockIdx.x % kShards)], (unsigned long long)t);
            atomicAdd(pb.windowSamples, t);
        }
    }
}

// ImageSensor::add for the passes of a finished window, in pass order (+ the noise records with kStats): one thread per float4 of
// the sensor.  The body is foldElement (pt_fold.h), shared with the indexed instantiations of slrhip_render_adaptive
// (pt_adaptive.hip); here an element's pixel is its own.  kClamp (slrhip_clamp_begin): the samples go through the clamp first; the
// clamp needs the luminance, so without statistics there is a spectral instantiation of it too.
template <bool kClamp, bool kStats, bool kSpectral>
__global__ __launch_bounds__(256) void k_fold(PathBuffers pb, uint32_t elems, uint32_t passes, float4* statRecords, FoldClampArgs<kClamp> clamp) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= elems) return;
    foldElement<kClamp, kStats, kSpectral, false>(pb, e, elems, passes, statRecords, nullptr, clamp);
}

void launchFold(const PathBuffers& pb, const RenderParams& rp, float4* statRecords, const ClampParams& clamp, hipStream_t stream) {
    const uint32_t elems = rp.numPixels * (rp.spectral ? 4u : 1u);
    if (elems == 0 || rp.sppCount == 0) return;
    const dim3 grid((elems + 255) / 256), block(256);
    if (clamp.records) {
        FoldClampArgs<true> on;
        static_cast<ClampParams&>(on) = clamp;
        if (!statRecords && rp.spectral) hipLaunchKernelGGL((k_fold<true, false, true>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, on);
        else if (!statRecords) hipLaunchKernelGGL((k_fold<true, false, false>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, on);
        else if (rp.spectral) hipLaunchKernelGGL((k_fold<true, true, true>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, on);
        else hipLaunchKernelGGL((k_fold<true, true, false>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, on);
        return;
    }
    const FoldClampArgs<false> off;
    // (the plain fold too has a spectral instantiation: where a lane's entries lie depends on the planes per pixel)
    if (!statRecords && rp.spectral) hipLaunchKernelGGL((k_fold<false, false, true>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, off);
    else if (!statRecords) hipLaunchKernelGGL((k_fold<false, false, false>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, off);
    else if (rp.spectral) hipLaunchKernelGGL((k_fold<false, true, true>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, off);
    else hipLaunchKernelGGL((k_fold<false, true, false>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, off);
}
void launchCountSamples(const PathBuffers& pb, const RenderParams& rp, hipStream_t stream) {
    if (rp.numSlots == 0) return;
    const uint32_t blocks = std::min<uint32_t>((rp.numWaves + kShadeBlock - 1) / kShadeBlock, 2048u);
    hipLaunchKernelGGL(k_count_samples, dim3(blocks), dim3(kShadeBlock), 0, stream, pb, rp);
}
void launchResolve(const PathBuffers& pb, const RenderParams& rp, float* dst, hipStream_t stream) {
    const dim3 grid((rp.numPixels + 255) / 256), block(256);
    if (rp.spectral) hipLaunchKernelGGL(k_resolve<Spec16>, grid, block, 0, stream, pb, rp, dst);
    else hipLaunchKernelGGL(k_resolve<RGB>, grid, block, 0, stream, pb, rp, dst);
}

} // namespace slrhip
