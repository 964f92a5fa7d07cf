// pt_fold.h — the body of k_fold (pt_shade.hip) and of its indexed instantiations (pt_adaptive.hip): ImageSensor::add for the
// passes of a finished result window, in pass order, plus the per-pixel noise records.  gfx950, wave64.
#pragma once
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_luminance.h"

namespace slrhip {

// ImageSensor::add for the passes of a finished window (Core/ImageSensor.cpp:52-62 -> SpectrumStorage::add): per pixel and bin,
// sum += value with the compensated sum of BasicTypes/CompensatedSum.h:24-30, the entries taken in PASS ORDER — the order in which
// one thread of the reference adds the samples of a pixel, whatever slot rendered them here.  One thread per float4 of the
// sensor (RGB: one per pixel, the fourth component idles; spectral: four per pixel); the window is pass-major, so the threads of
// a wave read consecutive 16-byte entries at every pass: a streaming kernel (window bytes / HBM rate).
// kStats (slrhip_statistics_begin): the same pass over the window also updates the pixel's noise record {mean, M2, n, max} of the
// samples' luminance (pt_luminance.h) with float32 Welford steps in pass order — the entries are in registers already, the
// extra traffic is one 16-byte record per pixel and window.  Spectral: the four planes of a pixel are four adjacent lanes (elems
// is a multiple of 4, so a quad never straddles the early exit); two quad exchanges give every lane of the quad the same Y, all
// four take the same steps and lane 0 stores the record.  The kStats = false instantiation is the kernel without any of this.
// `pixel` is the record's index: the element's pixel of the shard.
template <bool kStats, bool kSpectral>
struct FoldStats {                         // kStats = false: nothing
    __device__ __forceinline__ FoldStats(const float4*, uint32_t) {}
    __device__ __forceinline__ void add(const float4&) {}
    __device__ __forceinline__ void store(float4*, uint32_t, bool) const {}
};
template <bool kSpectral>
struct FoldStats<true, kSpectral> {
    float mean, m2, maxY;
    uint32_t n;
    __device__ __forceinline__ FoldStats(const float4* records, uint32_t pixel) {
        const float4 r = records[pixel];
        mean = r.x; m2 = r.y; n = __float_as_uint(r.z); maxY = r.w;
    }
    __device__ __forceinline__ void add(const float4& v) {
        float Y;
        if (kSpectral) {
            const float p = sampleLuminancePlane(threadIdx.x & 3u, v.x, v.y, v.z, v.w);
            const float pair = p + __shfl_xor(p, 1);
            Y = sampleLuminanceOfPlanes(pair, __shfl_xor(pair, 2));
        }
        else Y = sampleLuminanceRGB(v.x, v.y, v.z);
        n += 1u;
        const float d = Y - mean;
        mean = mean + d / (float)n;
        m2 = m2 + d * (Y - mean);
        maxY = fmaxf(maxY, Y);
    }
    __device__ __forceinline__ void store(float4* records, uint32_t pixel, bool first) const {
        if (first) records[pixel] = make_float4(mean, m2, __uint_as_float(n), maxY);
    }
};

// Element e of a window of `elems` elements per pass (e < elems; the caller's early exit).  kIndexed (slrhip_render_adaptive): the
// window is over a compact pixel list, and compact pixel i adds into the sensor and the record of pixel indexMap[i] of the shard;
// a spectral quad (four adjacent elements, e >> 2 = the compact pixel) moves as a whole, so the quad exchange of FoldStats holds.
// The window is read at e either way.  Not indexed: the pixel is the element's own, and indexMap is not read.
template <bool kStats, bool kSpectral, bool kIndexed>
__device__ __forceinline__ void foldElement(const PathBuffers& pb, uint32_t e, uint32_t elems, uint32_t passes, float4* statRecords,
                                            const uint32_t* indexMap) {
    const uint32_t plane = kSpectral ? e & 3u : 0u;
    const uint32_t compact = kSpectral ? e >> 2 : e;
    const uint32_t pixel = kIndexed ? indexMap[compact] : compact;
    const uint32_t dst = kIndexed ? (kSpectral ? pixel * 4u + plane : pixel) : e;
    float4 s = pb.fbSum[dst], c = pb.fbComp[dst];
    FoldStats<kStats, kSpectral> st(statRecords, pixel);
    const float4* r = pb.results + e;
    uint32_t p = 0;
    for (; p + 4 <= passes; p += 4) {
        // four entries requested together; added one after the other
        const float4 v0 = r[(size_t)p * elems], v1 = r[(size_t)(p + 1) * elems], v2 = r[(size_t)(p + 2) * elems], v3 = r[(size_t)(p + 3) * elems];
        kahanAdd(s.x, c.x, v0.x); kahanAdd(s.y, c.y, v0.y); kahanAdd(s.z, c.z, v0.z); kahanAdd(s.w, c.w, v0.w);
        kahanAdd(s.x, c.x, v1.x); kahanAdd(s.y, c.y, v1.y); kahanAdd(s.z, c.z, v1.z); kahanAdd(s.w, c.w, v1.w);
        kahanAdd(s.x, c.x, v2.x); kahanAdd(s.y, c.y, v2.y); kahanAdd(s.z, c.z, v2.z); kahanAdd(s.w, c.w, v2.w);
        kahanAdd(s.x, c.x, v3.x); kahanAdd(s.y, c.y, v3.y); kahanAdd(s.z, c.z, v3.z); kahanAdd(s.w, c.w, v3.w);
        st.add(v0); st.add(v1); st.add(v2); st.add(v3);
    }
    for (; p < passes; ++p) {
        const float4 v = r[(size_t)p * elems];
        kahanAdd(s.x, c.x, v.x); kahanAdd(s.y, c.y, v.y); kahanAdd(s.z, c.z, v.z); kahanAdd(s.w, c.w, v.w);
        st.add(v);
    }
    pb.fbSum[dst] = s;
    pb.fbComp[dst] = c;
    st.store(statRecords, pixel, plane == 0u);
}

} // namespace slrhip
