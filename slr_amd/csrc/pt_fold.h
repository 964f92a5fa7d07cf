// pt_fold.h — the body of k_fold (pt_shade.hip) and of its indexed instantiations (pt_adaptive.hip): ImageSensor::add for the
// passes of a finished result window, in pass order, plus the per-pixel noise records.  gfx950, wave64.
#pragma once
#include "pt_clamp.h"
#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_luminance.h"

namespace slrhip {

// ImageSensor::add for the passes of a finished window (Core/ImageSensor.cpp:52-62 -> SpectrumStorage::add): per pixel and bin,
// sum += value with the compensated sum of BasicTypes/CompensatedSum.h:24-30, the entries taken in PASS ORDER — the order in which
// one thread of the reference adds the samples of a pixel, whatever slot rendered them here.  One thread per float4 of the
// sensor (RGB: one per pixel, the fourth component idles; spectral: four per pixel); the window is pixel-major (windowEntry,
// pt_kernels.h), so a thread's entries are contiguous and the threads of a wave are a pixel's passes apart: a thread asks for a
// whole 128-byte line of its pixel at a time (RGB: eight passes; spectral: a quad asks for four passes, 256 bytes), every line of
// the window is fetched once: a streaming kernel (window bytes / HBM rate).
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
    __device__ __forceinline__ void addY(float) {}
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
        addY(Y);
    }
    __device__ __forceinline__ void addY(float Y) {
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

// kClamp (slrhip_clamp_begin): every entry goes through clampSample (pt_clamp.h) before it is added, and the pixel's clamp record
// {clamped, dropped (uint32 bits), removed, largest} is kept beside the noise record: loaded and stored once per pixel and window.
// RGB: the thread holds the whole sample.  Spectral: the thread holds one plane, and the luminance ends in the quad exchange of
// FoldStats above, so all four lanes of a quad hold the same Y and the same factor, each scales its plane, all four keep the same
// record and the lane of plane 0 stores it.  apply() returns the luminance of the sample as the sensor receives it, which is what
// the Welford step takes (FoldStats::addY).  The kClamp = false instantiation is the kernel without any of this.
struct FoldLuminanceRGB {
    __device__ __forceinline__ float operator()(const float (&v)[3]) const { return sampleLuminanceRGB(v[0], v[1], v[2]); }
};
struct FoldLuminanceQuad {
    __device__ __forceinline__ float operator()(const float (&v)[4]) const {
        const float p = sampleLuminancePlane(threadIdx.x & 3u, v[0], v[1], v[2], v[3]);
        const float pair = p + __shfl_xor(p, 1);
        return sampleLuminanceOfPlanes(pair, __shfl_xor(pair, 2));
    }
};
template <bool kClamp, bool kSpectral>
struct FoldClamp {                         // kClamp = false: nothing
    __device__ __forceinline__ FoldClamp(const FoldClampArgs<false>&, uint32_t) {}
    __device__ __forceinline__ void store(const FoldClampArgs<false>&, uint32_t, bool) const {}
};
template <bool kSpectral>
struct FoldClamp<true, kSpectral> {
    uint32_t clamped, dropped;
    float removed, largest, limit;
    uint32_t flags;
    __device__ __forceinline__ FoldClamp(const FoldClampArgs<true>& a, uint32_t pixel) {
        const float4 r = a.records[pixel];
        clamped = __float_as_uint(r.x); dropped = __float_as_uint(r.y); removed = r.z; largest = r.w;
        limit = a.limit; flags = a.flags;
    }
    __device__ __forceinline__ float apply(float4& v) {
        float yIn, yOut;
        uint32_t what;
        if (kSpectral) {
            float a[4] = {v.x, v.y, v.z, v.w};
            what = clampSample(a, limit, flags, FoldLuminanceQuad(), yIn, yOut);
            v = make_float4(a[0], a[1], a[2], a[3]);
        }
        else {                             // the fourth component idles: it is left as it is
            float a[3] = {v.x, v.y, v.z};
            what = clampSample(a, limit, flags, FoldLuminanceRGB(), yIn, yOut);
            v.x = a[0]; v.y = a[1]; v.z = a[2];
        }
        const bool c = what == CLAMP_CLAMPED;
        dropped += what == CLAMP_DROPPED ? 1u : 0u;
        clamped += c ? 1u : 0u;
        removed = c ? removed + (yIn - yOut) : removed;
        largest = c ? fmaxf(largest, yIn) : largest;
        return yOut;
    }
    __device__ __forceinline__ void store(const FoldClampArgs<true>& a, uint32_t pixel, bool first) const {
        if (first) a.records[pixel] = make_float4(__uint_as_float(clamped), __uint_as_float(dropped), removed, largest);
    }
};

// Element e of a window of `elems` elements per pass (e < elems; the caller's early exit).  kIndexed (slrhip_render_adaptive): the
// window is over a compact pixel list, and compact pixel i adds into the sensor and the record of pixel indexMap[i] of the shard;
// a spectral quad (four adjacent elements, e >> 2 = the compact pixel) moves as a whole, so the quad exchange of FoldStats holds.
// The window is read at the compact pixel's entries either way.  Not indexed: the pixel is the element's own, and indexMap is not read.
template <bool kClamp, bool kStats, bool kSpectral, bool kIndexed>
__device__ __forceinline__ void foldElement(const PathBuffers& pb, uint32_t e, uint32_t elems, uint32_t passes, float4* statRecords,
                                            const uint32_t* indexMap, const FoldClampArgs<kClamp>& clampArgs) {
    const uint32_t plane = kSpectral ? e & 3u : 0u;
    const uint32_t compact = kSpectral ? e >> 2 : e;
    const uint32_t pixel = kIndexed ? indexMap[compact] : compact;
    const uint32_t dst = kIndexed ? (kSpectral ? pixel * 4u + plane : pixel) : e;
    float4 s = pb.fbSum[dst], c = pb.fbComp[dst];
    FoldStats<kStats, kSpectral> st(statRecords, pixel);
    FoldClamp<kClamp, kSpectral> cl(clampArgs, pixel);
    // the pixel's entries are contiguous (windowEntry): pass p of this lane's plane is r[p * planes]
    constexpr uint32_t planes = kSpectral ? 4u : 1u;
    const float4* r = pb.results + windowEntry(compact, 0u, passes) * planes + plane;
    uint32_t p = 0;
    if constexpr (!kSpectral) {
        // RGB: eight entries requested together — the 128 bytes of a pixel's passes p .. p + 7, so that a line is fetched once
        // (the lanes of a wave are `passes` entries apart); added one after the other
        for (; p + 8 <= passes; p += 8) {
            float4 v[8];
            float y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = r[p + k];
            if constexpr (kClamp) {
#pragma unroll
                for (int k = 0; k < 8; ++k) y[k] = cl.apply(v[k]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) { kahanAdd(s.x, c.x, v[k].x); kahanAdd(s.y, c.y, v[k].y); kahanAdd(s.z, c.z, v[k].z); kahanAdd(s.w, c.w, v[k].w); }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if constexpr (kClamp) st.addY(y[k]);
                else st.add(v[k]);
            }
        }
    }
    for (; p + 4 <= passes; p += 4) {
        // four entries requested together (spectral: the 256 bytes of a quad's four passes); added one after the other
        float4 v0 = r[(size_t)p * planes], v1 = r[(size_t)(p + 1) * planes], v2 = r[(size_t)(p + 2) * planes], v3 = r[(size_t)(p + 3) * planes];
        float y0, y1, y2, y3;
        if constexpr (kClamp) { y0 = cl.apply(v0); y1 = cl.apply(v1); y2 = cl.apply(v2); y3 = cl.apply(v3); }
        kahanAdd(s.x, c.x, v0.x); kahanAdd(s.y, c.y, v0.y); kahanAdd(s.z, c.z, v0.z); kahanAdd(s.w, c.w, v0.w);
        kahanAdd(s.x, c.x, v1.x); kahanAdd(s.y, c.y, v1.y); kahanAdd(s.z, c.z, v1.z); kahanAdd(s.w, c.w, v1.w);
        kahanAdd(s.x, c.x, v2.x); kahanAdd(s.y, c.y, v2.y); kahanAdd(s.z, c.z, v2.z); kahanAdd(s.w, c.w, v2.w);
        kahanAdd(s.x, c.x, v3.x); kahanAdd(s.y, c.y, v3.y); kahanAdd(s.z, c.z, v3.z); kahanAdd(s.w, c.w, v3.w);
        if constexpr (kClamp) { st.addY(y0); st.addY(y1); st.addY(y2); st.addY(y3); }
        else { st.add(v0); st.add(v1); st.add(v2); st.add(v3); }
    }
    for (; p < passes; ++p) {
        float4 v = r[(size_t)p * planes];
        float y;
        if constexpr (kClamp) y = cl.apply(v);
        kahanAdd(s.x, c.x, v.x); kahanAdd(s.y, c.y, v.y); kahanAdd(s.z, c.z, v.z); kahanAdd(s.w, c.w, v.w);
        if constexpr (kClamp) st.addY(y);
        else st.add(v);
    }
    pb.fbSum[dst] = s;
    pb.fbComp[dst] = c;
    st.store(statRecords, pixel, plane == 0u);
    cl.store(clampArgs, pixel, plane == 0u);
}

} // namespace slrhip
