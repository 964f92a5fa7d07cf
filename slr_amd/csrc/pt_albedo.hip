// pt_albedo.hip — device code of the albedo feature buffer (slrhip_render_albedo / slrhip_resolve_albedo) and of slrhip_modulate, as
// defined in include/slrhip.h.  gfx950, wave64.
//
// The traversal of an albedo pass is the feature pass's (launchFeatureTrace, pt_trace_indexed.hip: camera rays made on the spot, one hit record
// {triangle, instance, dist, b1} per sample, b2 in a plane of its own).  k_albedo_fold turns a window's records into base colours: one
// lane owns a pixel and takes its passes in pass order — the material record of the hit triangle (MatIO), its textures at the hit's
// texture coordinate (texturizeMat), BSDF::getBaseColor(All) of the lobe (bsdfBaseColor, pt_bsdf.h) or of the MultiBSDF
// (bsdfBaseColorMulti, pt_bsdf_multi.h) — and adds it to the pixel with plain float32 adds.  The tables are read from HBM, as
// k_bsdf_queries reads them.  The sample's wavelength offset is not in the record: the fold draws it again from (seed, pixel, pass).
#include "pt_bsdf.h"
#include "pt_bsdf_multi.h"
#include "pt_camera.h"
#include "pt_luminance.h"
#include "pt_shade_tables.h"
#include "pt_tex.h"
#include "pt_tex_spectrum.h"

namespace slrhip {

namespace {

// The sums: one float plane per component, plane k of pixel i at [k * numPixels + i] (components x 4 B per pixel, every plane a
// coalesced stream).
template <class S>
__device__ __forceinline__ S loadSums(const float* sums, uint32_t pix, uint32_t numPixels) {
    return S::make([&](int k) { return sums[(size_t)k * numPixels + pix]; });
}
template <class S>
__device__ __forceinline__ void storeSums(float* sums, uint32_t pix, uint32_t numPixels, const S& v) {
#pragma unroll
    for (int k = 0; k < S::N; ++k) sums[(size_t)k * numPixels + pix] = v.own(k);
}

template <class S>
__global__ __launch_bounds__(256) void k_albedo_fold(DevScene sc, FeatureParams fp, float* sums) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const uint32_t xy = fp.pixelXY[pix];
    S acc = loadSums<S>(sums, pix, fp.numPixels);
#pragma unroll 1
    for (uint32_t p = 0; p < fp.numPasses; ++p) {
        const size_t e = (size_t)p * fp.numPixels + pix;
        const float4 r = fp.records[e];
        const uint32_t tri = __float_as_uint(r.x);
        if (tri == 0xFFFFFFFFu) { acc = acc + S(1.0f); continue; }      // a miss (the environment sphere included): radiance that is divided by one
        float wlOffset = 0.0f;
        if (S::N != 3) {
            // the fourth draw of the camera sample (createWithEqualOffsets' offset), as the path tracer's startSample draws it
            Rng rng;
            wlOffset = drawCameraSample(rng, fp.rngSeed, xy & 0xFFFFu, xy >> 16, fp.passBegin + p, fp.timeStart, fp.timeEnd).wlOffset;
        }
        const uint32_t material = reinterpret_cast<const uint32_t*>(reinterpret_cast<const float4*>(sc.shadeTris) + (size_t)tri * 6)[3];
        float texU = 0.0f, texV = 0.0f;
        if (sc.numTextures) {
            // texCoord from the original barycentrics (TriangleMesh.cpp:160-161), as k_feature_fold does for the bump map
            const float4 uvA = sc.triUV[(size_t)tri * 2], uvB = sc.triUV[(size_t)tri * 2 + 1];
            hitTexCoord(uvA, uvB, r.w, fp.b2[e], &texU, &texV);
        }
        const auto load = [&](uint32_t idx) {
            Mat<S> cm = MatIO<S>::template load<false>(sc, nullptr, idx, wlOffset);
            if (cm.type & kMatTexturedBit) (void)texturizeMat<S>(sc, cm, idx, texU, texV, wlOffset);
            return cm;
        };
        const Mat<S> m = load(material);
        S color;
        if (m.type == SLRHIP_MATERIAL_MULTI) color = bsdfBaseColorMulti<S>(buildMultiTree<S>(decodeMulti(m), load), load);
        else color = bsdfBaseColor(m);
        acc = acc + color;
    }
    storeSums<S>(sums, pix, fp.numPixels, acc);
}

// slrhip_resolve_albedo: the sums scattered into a [height][width][components] image the caller has cleared
__global__ __launch_bounds__(256) void k_albedo_resolve(FeatureParams fp, uint32_t components, const float* sums, float* dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const uint32_t xy = fp.pixelXY[pix];
    float* o = dst + ((size_t)(xy >> 16) * fp.imageWidth + (xy & 0xFFFFu)) * components;
    for (uint32_t k = 0; k < components; ++k) o[k] = sums[(size_t)k * fp.numPixels + pix];
}

// slrhip_modulate: one thread per pixel.  Every operation is a float32 operation rounded on its own (the unit is built with
// -ffp-contract=off); the luminance is pt_luminance.h's, the expression of slrhip_sample_luminance.
template <int C>
__device__ __forceinline__ float luminanceOf(const float (&a)[C]) {
    if constexpr (C == 3) return sampleLuminanceRGB(a[0], a[1], a[2]);
    else {
        float p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) p[q] = sampleLuminancePlane((uint32_t)q, a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
        return sampleLuminanceOfPlanes(p[0] + p[1], p[2] + p[3]);
    }
}

template <int C, bool kMultiply>
__global__ __launch_bounds__(256) void k_modulate(slrhip_modulate_desc d, uint32_t numPixels) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= numPixels) return;
    const float passes = (float)d.albedo_passes;
    const float* al = d.albedo + (size_t)pix * C;
    const float* in = d.color + (size_t)pix * C;
    float* out = d.output + (size_t)pix * C;
    float a[C], c[C];
#pragma unroll
    for (int k = 0; k < C; ++k) { a[k] = fmaxf(al[k] / passes, d.floor); c[k] = in[k]; }      // fmaxf(NaN, floor) = floor
#pragma unroll
    for (int k = 0; k < C; ++k) out[k] = kMultiply ? c[k] * a[k] : c[k] / a[k];
    if (d.output_variance) {
        const float ya = luminanceOf<C>(a);
        const float y2 = ya * ya;
        const float v = d.variance[pix];
        d.output_variance[pix] = kMultiply ? v * y2 : v / y2;
    }
}

} // namespace

void launchAlbedoFold(const DevScene& sc, const FeatureParams& fp, bool spectral, float* sums, hipStream_t stream) {
    const dim3 grid((fp.numPixels + 255u) / 256u), block(256);
    if (spectral) hipLaunchKernelGGL(k_albedo_fold<Spec16>, grid, block, 0, stream, sc, fp, sums);
    else hipLaunchKernelGGL(k_albedo_fold<RGB>, grid, block, 0, stream, sc, fp, sums);
}

void launchAlbedoResolve(const FeatureParams& fp, uint32_t components, const float* sums, float* dst, hipStream_t stream) {
    hipLaunchKernelGGL(k_albedo_resolve, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, fp, components, sums, dst);
}

void launchModulate(const slrhip_modulate_desc& d, hipStream_t stream) {
    const uint32_t numPixels = d.width * d.height;                       // < 2^31 (checked by the caller)
    const dim3 grid((numPixels + 255u) / 256u), block(256);
    const bool mul = d.op == SLRHIP_MODULATE_MULTIPLY;
    if (d.components == 3) {
        if (mul) hipLaunchKernelGGL((k_modulate<3, true>), grid, block, 0, stream, d, numPixels);
        else hipLaunchKernelGGL((k_modulate<3, false>), grid, block, 0, stream, d, numPixels);
    }
    else {
        if (mul) hipLaunchKernelGGL((k_modulate<16, true>), grid, block, 0, stream, d, numPixels);
        else hipLaunchKernelGGL((k_modulate<16, false>), grid, block, 0, stream, d, numPixels);
    }
}

} // namespace slrhip
