// pt_sample_start.h — the two ends of a sample in the path tracer's kernels (gfx950, wave64): Job::kernel's camera half
// (Renderers/PathTracingRenderer.cpp:100-120: beginSample / resumeSample / startSample, and the primary pass's record of the
// camera ray's hit) and the finished sample's contribution written to the result window (writeResult, storageAddend).
#pragma once
#include "pt_bsdf.h"            // wavelengthOf
#include "pt_camera.h"
#include "pt_kernels.h"
#include "pt_slot_state.h"

namespace slrhip {

// SpectrumStorage::add.  RGB: the sample is Kahan-added to the pixel (RGBTypes.h:176-179).  Spectral: every component goes
// to the storage bin of its wavelength scaled by the reciprocal bin width, then the 16-bin addend is Kahan-added
// (SpectrumTypes.h:818-836).  Bin selection through compare-selects keeps the addend in registers.
__device__ __forceinline__ RGB storageAddend(const RGB& val, float) { return val; }
__device__ __forceinline__ Spec16 storageAddend(const Spec16& val, float wlOffset) {
    const float recBinWidth = 16 / (830.0f - 360.0f);
    uint32_t sBin[16];
    float v[16];
    bool near = true;           // every component lands in its own bin or a neighbour (it always does up to rounding: lambda_i = 360 + 470 (i + u) / 16)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        sBin[i] = min((uint32_t)((wavelengthOf(i, wlOffset) - 360.0f) / (830.0f - 360.0f) * 16), 15u);
        v[i] = val.c[i] * recBinWidth;
        near = near && (sBin[i] + 1u >= (uint32_t)i) && (sBin[i] <= (uint32_t)i + 1u);
    }
    Spec16 addend;
    if (near) {
        // bin b can only receive components b-1, b, b+1: three guarded adds in component order instead of sixteen
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            float a = 0.0f;
            if (b > 0) a = (sBin[b - 1] == (uint32_t)b) ? a + v[b - 1] : a;
            a = (sBin[b] == (uint32_t)b) ? a + v[b] : a;
            if (b < 15) a = (sBin[b + 1] == (uint32_t)b) ? a + v[b + 1] : a;
            addend.c[b] = a;
        }
    }
    else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
#pragma unroll
            for (int b = 0; b < 16; ++b) addend.c[b] = (sBin[i] == (uint32_t)b) ? addend.c[b] + v[i] : addend.c[b];
        }
    }
    return addend;
}

// Job::kernel's camera half (PathTracingRenderer.cpp:100-120): seeds the sample's stream, draws in source (left-to-right)
// order and leaves the slot with a camera ray in flight; writes the slot's sample header (k_shade's compacted start lanes;
// the tail kernel for the passes left when it takes over).
// What the camera half leaves in registers: the stream after the camera draws, the sample header's values and the camera ray.
struct SampleStart {
    Rng rng;
    uint32_t wl;
    float wlOffset, camWeight;
    V3 org, dir;
};
// ... from the draws on: st.rng holds the stream after them
template <class S>
__device__ __forceinline__ void sampleFromDraws(const DevScene& sc, const RenderParams& rp, const CameraDraws& draws, SampleStart& st) {
    // createWithEqualOffsets: RGBTypes.h:37-45 (offset unused, PDF 1) / SpectrumTypes.h:54-64 (PDF N / 470)
    st.wlOffset = draws.wlOffset;
    st.wl = min((uint32_t)(uint16_t)(S::N * draws.uLambda), (uint32_t)(S::N - 1));
    const float selectWLPDF = S::N == 3 ? 1.0f : S::N / (830.0f - 360.0f);
    // PerspectiveCamera::sample + PerspectiveIDF::sample (pt_camera.h)
    const CameraRay cam = sampleCameraRay(sc.camera, rp.imageWidth, rp.imageHeight, draws);
    const V3 lensN = cam.lensN;
    st.org = cam.org; st.dir = cam.dir;
    float dirPDF = sc.camera.imgPlaneDistance * sc.camera.imgPlaneDistance /
                   ((cam.dirLocalZ * cam.dirLocalZ * cam.dirLocalZ) * sc.camera.imgPlaneArea);
    // weight :126
    st.camWeight = absDot(st.dir, lensN) / (sc.camera.areaPDF * dirPDF * selectWLPDF);
}
template <class S>
__device__ __forceinline__ SampleStart beginSample(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t pix, uint32_t passOfWindow) {
    // Job::kernel PathTracingRenderer.cpp:100-120, draws in source (left-to-right) order
    const uint32_t xy = pb.pixelXY[pix];
    const uint32_t px = xy & 0xFFFFu, py = xy >> 16;
    SampleStart st;
    const CameraDraws draws = drawCameraSample(st.rng, rp.rngSeed, px, py, rp.sppBegin + passOfWindow, rp.timeStart, rp.timeEnd);
    sampleFromDraws<S>(sc, rp, draws, st);
    return st;
}
// The fused start (k_shade with a primary pass): the stream after the camera draws comes from the primary pass, which drew them for
// the same sample (PathBuffers::primaryRng), and the draws from the stream (recoverCameraDraws, pt_camera.h).
template <class S>
__device__ __forceinline__ SampleStart resumeSample(const DevScene& sc, const RenderParams& rp, uint32_t xy, const uint4& stream) {
    SampleStart st;
    st.rng.s0 = stream.x; st.rng.s1 = stream.y; st.rng.s2 = stream.z; st.rng.s3 = stream.w;
    sampleFromDraws<S>(sc, rp, recoverCameraDraws(st.rng, xy & 0xFFFFu, xy >> 16), st);
    return st;
}
template <class S>
__device__ __forceinline__ void startSample(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t slot, uint32_t pix,
                                            uint32_t passOfWindow) {
    const SampleStart st = beginSample<S>(sc, pb, rp, pix, passOfWindow);
    pb.flags[slot] = F_MAKE((uint32_t)ST_FIRST_HIT, 0u, st.wl, 0u, 0u, 0u);
    pb.rng[(size_t)slot * pb.hdrStride] = make_uint4(st.rng.s0, st.rng.s1, st.rng.s2, st.rng.s3);
    // alpha = 1, pdfPrev = 0 and sp = 0 are implied by ST_FIRST_HIT (see SpAcc): 48 B (RGB) / 196 B (spectral) not written
    pb.hdr[(size_t)slot * pb.hdrStride] = make_uint4(pix, __float_as_uint(st.camWeight), __float_as_uint(st.wlOffset), passOfWindow);
    pb.rayOrg[(size_t)slot * pb.rayStride] = make_float4(st.org.x, st.org.y, st.org.z, 0.0f);
    pb.rayDir[(size_t)slot * pb.rayStride] = make_float4(st.dir.x, st.dir.y, st.dir.z, INFINITY);
}

// The pre-traced first hit of sample (pix, passOfWindow) of the window: the primary pass's record in the sample's entry of the
// result window (launchPrimary, pt_kernels.h), and the instance where the scene has instances.
template <class S>
__device__ __forceinline__ void loadPrimaryRecord(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t pix, uint32_t passOfWindow,
                                                  float4& h, int32_t& inst) {
    const size_t entry = windowEntry(pix, passOfWindow, rp.sppCount);
    h = pb.results[entry * (S::N == 3 ? 1u : 4u)];
    inst = sc.instances ? pb.primaryInstance[entry] : -1;
}

// The finished sample's contribution, weight * C of sensor->add(p.x, p.y, wls, weight * C) (PathTracingRenderer.cpp:126-130) as
// the sensor's storage takes it (ImageSensor::add -> SpectrumStorage::add: RGB as it is, spectral spread over the 16 bins),
// written to the sample's entry of the result window; k_fold adds the entries of a pixel in pass order.  `inRegisters`: C is
// handed over by the caller (RGB in k_shade); else it is read from the slot's radiance sum in HBM, if the path ever wrote it
// (flag bit 10).
__device__ __forceinline__ void storeResult(float4* results, size_t entry, const RGB& v) { results[entry] = make_float4(v.r, v.g, v.b, 0.0f); }
__device__ __forceinline__ void storeResult(float4* results, size_t entry, const Spec16& v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) results[entry * 4 + k] = make_float4(v.c[4 * k], v.c[4 * k + 1], v.c[4 * k + 2], v.c[4 * k + 3]);
}
template <class S>
__device__ __forceinline__ void writeResult(const PathBuffers& pb, const RenderParams& rp, uint32_t slot, uint32_t flags, const uint4& hdr,
                                            bool inRegisters, S C) {
    float unusedW;
    const float camW = __uint_as_float(hdr.y);
    if (!inRegisters) {
        C = S();
        if (F_SPVALID(flags)) SpecIO<S>::load(pb.spR, nullptr, slot * pb.spStride, rp.numSlots * pb.spStride, C, unusedW);     // else the path gathered nothing: C = 0
    }
    const S weight = (S(1.0f) * S(1.0f)) * camW;
    storeResult(pb.results, windowEntry(hdr.x, hdr.w, rp.sppCount), storageAddend(weight * C, S::N == 3 ? 0.0f : __uint_as_float(hdr.z)));
}

} // namespace slrhip
