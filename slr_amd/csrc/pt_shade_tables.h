// pt_shade_tables.h — the shading tables of a scene as the kernels read them (gfx950, wave64): material, emittance and light
// records from HBM or from the copy a workgroup stages in LDS (ShadeLds, stageShadeTables; limits: pt_kernels.h), and the light
// selection over the staged distribution.
#pragma once
#include "pt_bsdf.h"
#include "pt_kernels.h"

namespace slrhip {

// Material access per mode
template <class S> struct MatIO;
template <> struct MatIO<RGB> {
    template <bool LDS>
    static __device__ __forceinline__ Mat<RGB> load(const DevScene& sc, const float4* ldsMats, uint32_t idx, float) {
        return loadMat(LDS ? reinterpret_cast<const DevMaterial*>(ldsMats) + idx : sc.materials + idx);
    }
    template <bool LDS>
    static __device__ __forceinline__ RGB emittance(const DevScene& sc, const float4* ldsMats, uint32_t idx, float) {
        return loadEmittance(LDS ? reinterpret_cast<const DevMaterial*>(ldsMats) + idx : sc.materials + idx);
    }
};
// spectral mode, LDS tables: [DevMaterialS x kLdsMaterials][DevSpectrum x kLdsSpectra][sample pool, kLdsPoolFloats floats]
__device__ __forceinline__ const float* ldsPoolOf(const float4* ldsMats) {
    return reinterpret_cast<const float*>(ldsMats + 2 * kLdsMaterials + 2 * kLdsSpectra);
}
template <class S> struct MatIOSpectral {
    // spectral mode: the LDS table holds the DevMaterialS records (2 x float4 each) followed by the DevSpectrum records
    template <bool LDS>
    static __device__ __forceinline__ Mat<S> load(const DevScene& sc, const float4* ldsMats, uint32_t idx, float wlOffset) {
        const DevMaterialS* mats = LDS ? reinterpret_cast<const DevMaterialS*>(ldsMats) : sc.materialsS;
        const DevSpectrum* spectra = LDS ? reinterpret_cast<const DevSpectrum*>(ldsMats + 2 * kLdsMaterials) : sc.spectra;
        return loadMatSpectral<S>(mats, idx, spectra, LDS ? ldsPoolOf(ldsMats) : sc.spectrumPool, wlOffset);
    }
    template <bool LDS>
    static __device__ __forceinline__ S emittance(const DevScene& sc, const float4* ldsMats, uint32_t idx, float wlOffset) {
        const DevMaterialS* mats = LDS ? reinterpret_cast<const DevMaterialS*>(ldsMats) : sc.materialsS;
        const DevSpectrum* spectra = LDS ? reinterpret_cast<const DevSpectrum*>(ldsMats + 2 * kLdsMaterials) : sc.spectra;
        return evalSpectrum<S>(spectra, LDS ? ldsPoolOf(ldsMats) : sc.spectrumPool, mats[idx].spec[3], wlOffset);
    }
};
template <> struct MatIO<Spec16> : MatIOSpectral<Spec16> {};

// RegularConstantDiscrete1D::sample, Core/distributions.cpp:97-107
__device__ __forceinline__ uint32_t selectLight(const DevScene& sc, const float* cdf, const float* pmf, float u, float* prob) {
    int idx = (int)sc.numLights;
    for (int d = (int)sc.lightPow2; d > 0; d >>= 1)
        if (idx - d > 0 && cdf[idx - d] >= u) idx -= d;
    --idx;
    *prob = pmf[idx];
    return (uint32_t)idx;
}

template <bool SPECTRAL>
struct ShadeLds {
    // RGB: DevMaterial = 5 x float4 each.  Spectral: DevMaterialS (2 x float4 each), DevSpectrum (2 x float4 each), then the
    // spectrum sample pool: evaluating a spectrum is 16 x 2 scattered 16-byte reads per slot, which the vector L1 serves at
    // one cache line per clock (measured: the look-ups were 1.0-1.6 ms of a 1.4-2.0 ms launch); LDS serves them in banks
    float4 mats[SPECTRAL ? kLdsMaterials * 2 + kLdsSpectra * 2 + kLdsPoolFloats / 4 : kLdsMaterials * 5];
    float4 lights[kLdsLights * 9];         // LightTri   = 9 x float4
    float lightPMF[kLdsLights];
    float lightCDF[kLdsLights + 4];        // kLdsLights + 1 entries, padded to whole float4
};
static_assert(kLdsLights % 4 == 0, "the light PMF is staged as whole float4");

// Stage the shading tables of the scene (DevScene::shadeTables: one packed array, segments in the order of ShadeLds' members) in
// LDS.  One flat copy: every thread requests its (up to four) float4 first and writes them afterwards, so the whole table costs
// ONE memory round trip — the per-table loops this replaces waited for each table in turn, four to six dependent round trips at
// the top of every workgroup.  The caller's barrier publishes the tables.
template <bool SPECTRAL>
__device__ __forceinline__ void stageShadeTables(const DevScene& sc, ShadeLds<SPECTRAL>& lds) {
    constexpr uint32_t kSegments = SPECTRAL ? 6u : 4u;
    // float4 index of every segment's first element inside ShadeLds
    constexpr uint32_t matsF4 = SPECTRAL ? kLdsMaterials * 2 + kLdsSpectra * 2 + kLdsPoolFloats / 4 : kLdsMaterials * 5;
    const uint32_t dst[6] = {0u,
                             SPECTRAL ? (uint32_t)(kLdsMaterials * 2) : matsF4,
                             SPECTRAL ? (uint32_t)(kLdsMaterials * 2 + kLdsSpectra * 2) : matsF4 + kLdsLights * 9,
                             SPECTRAL ? matsF4 : matsF4 + kLdsLights * 9 + kLdsLights / 4,
                             matsF4 + kLdsLights * 9,
                             matsF4 + kLdsLights * 9 + kLdsLights / 4};
    float4* out = reinterpret_cast<float4*>(&lds);
    const uint32_t total = sc.tableEnd[kSegments - 1];
    for (uint32_t base = threadIdx.x; base < total; base += 4 * kShadeBlock) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = base + u * kShadeBlock;
            v[u] = sc.shadeTables[min(i, total - 1u)];      // unconditional (clamped), so that the four requests leave back to back
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) asm volatile("" : "+v"(v[u].x), "+v"(v[u].y), "+v"(v[u].z), "+v"(v[u].w));      // ... and are not sunk into the guarded writes below
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = base + u * kShadeBlock;
            if (i >= total) continue;
            uint32_t begin = 0, to = dst[0];
#pragma unroll
            for (uint32_t k = 0; k + 1 < kSegments; ++k)
                if (i >= sc.tableEnd[k]) { begin = sc.tableEnd[k]; to = dst[k + 1]; }
            out[to + (i - begin)] = v[u];
        }
    }
}

} // namespace slrhip
