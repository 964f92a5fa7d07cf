// pt_luminance.h — the luminance Y of one sample (a result-window entry: weight x C as ImageSensor::add receives it), the value
// the per-pixel noise statistics are taken of.  ONE definition for the host export (slrhip_sample_luminance, host_util.cpp) and
// the fold kernel (pt_shade.hip); the constants are those of slrhip_tonemap_bgr8 / ImageSensor::saveImage.  float32 operations
// in the order written (both sides are built with -ffp-contract=off), so host and device agree bit for bit.
#pragma once
#include <cstdint>

#include "cmf16_table.h"

#ifdef __HIP__
#define SLR_HOST_DEV __host__ __device__ inline __attribute__((always_inline))
#else
#define SLR_HOST_DEV inline
#endif

namespace slrhip {

// RGB: saveImage's Y line (ImageSensor.cpp:172): double literals, float operands, rounded to float once.  No clamp, no scale.
SLR_HOST_DEV float sampleLuminanceRGB(float r, float g, float b) { return (float)(0.222485 * r + 0.716905 * g + 0.060610 * b); }

// Spectral: the sixteen bins are four float4 planes; plane q holds bins 4q .. 4q + 3.  Its part of the ybar sum
// (DiscretizedSpectrum::getRGB's Y, SpectrumTypes.h:702-721), left to right:
SLR_HOST_DEV float sampleLuminancePlane(uint32_t q, float x, float y, float z, float w) {
    // (selected by comparison: the table is a host constant, and an index known at compile time keeps it out of device memory)
    const float w0 = q == 0 ? kCmfY16[0] : q == 1 ? kCmfY16[4] : q == 2 ? kCmfY16[8] : kCmfY16[12];
    const float w1 = q == 0 ? kCmfY16[1] : q == 1 ? kCmfY16[5] : q == 2 ? kCmfY16[9] : kCmfY16[13];
    const float w2 = q == 0 ? kCmfY16[2] : q == 1 ? kCmfY16[6] : q == 2 ? kCmfY16[10] : kCmfY16[14];
    const float w3 = q == 0 ? kCmfY16[3] : q == 1 ? kCmfY16[7] : q == 2 ? kCmfY16[11] : kCmfY16[15];
    return ((w0 * x + w1 * y) + w2 * z) + w3 * w;
}
// ... and the four parts: pairs first (what two quad exchanges give every lane of a quad), then the normalisation.
SLR_HOST_DEV float sampleLuminanceOfPlanes(float p01, float p23) { return (p01 + p23) / kIntegralCmf16; }

} // namespace slrhip
