// pt_tonemap.h — one pixel of the image export: linear floats -> three 8-bit channels, the pipeline of ImageSensor::saveImage
// (Core/ImageSensor.cpp:138-186) as include/slrhip.h states it for slrhip_tonemap.  ONE definition for the host export
// (slrhip_tonemap_bgr8, host_util.cpp) and the kernel (pt_tonemap.hip).  float32 operations in the order written (both sides
// are built with -ffp-contract=off), the steps with double literals in double, so host and device agree bit for bit up to the two
// library calls, which the caller supplies through M:
//     static float  M::expNeg(float Y)     e of the tone curve: exp(-Y), rounded to float
//     static double M::gammaPow(float v)   pow((double)v, 1.0 / 2.4) of the gamma segment
#pragma once
#include <cmath>
#include <cstdint>

#include "cmf16_table.h"
#include "pt_luminance.h"          // SLR_HOST_DEV

namespace slrhip {

// sRGB_gamma, BasicTypes/Spectrum.cpp:15-21 (float instantiation; literals are double)
template <class M>
SLR_HOST_DEV float tonemapGamma(float value) {
    if (value <= 0.0031308) return (float)(12.92 * value);
    return (float)(1.055 * M::gammaPow(value) - 0.055);
}

// p: the pixel's C = 3 or 16 floats.  bgr: the bytes in the order a BMP stores them.
template <int C, class M>
SLR_HOST_DEV void tonemapPixel(const float* p, float scale, uint8_t bgr[3]) {
    float RGB[3];
    if (C == 3) {
        RGB[0] = p[0] * scale; RGB[1] = p[1] * scale; RGB[2] = p[2] * scale;               // pixel(j, i) * scale
    }
    else {
        // DiscretizedSpectrum::getRGB, BasicTypes/SpectrumTypes.h:702-721: 16 storage bins -> XYZ -> sRGB
        // (the loop is unrolled: every table index is a compile-time constant, the tables become literals in device code)
        float XYZ[3] = {0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const float v = p[b] * scale;                                                  // pixel(j, i) * scale
            XYZ[0] += kCmfX16[b] * v;
            XYZ[1] += kCmfY16[b] * v;
            XYZ[2] += kCmfZ16[b] * v;
        }
        XYZ[0] /= kIntegralCmf16; XYZ[1] /= kIntegralCmf16; XYZ[2] /= kIntegralCmf16;
        // XYZ_to_sRGB, BasicTypes/Spectrum.h:60-64 (double literals, float operands and results)
        RGB[0] = (float)(3.2404542 * XYZ[0] - 1.5371385 * XYZ[1] - 0.4985314 * XYZ[2]);
        RGB[1] = (float)(-0.9692660 * XYZ[0] + 1.8760108 * XYZ[1] + 0.0415560 * XYZ[2]);
        RGB[2] = (float)(0.0556434 * XYZ[0] - 0.2040259 * XYZ[1] + 1.0572252 * XYZ[2]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) RGB[k] = RGB[k] < 0.0f ? 0.0f : RGB[k];
    const float Y = (float)(0.222485 * RGB[0] + 0.716905 * RGB[1] + 0.060610 * RGB[2]);
    const float scaleY = Y != 0 ? (1.0f - M::expNeg(Y)) / Y : 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float v = fminf(scaleY * RGB[k], 1.0f);
        bgr[2 - k] = (uint8_t)(256 * fminf(tonemapGamma<M>(v), 0.999f));
    }
}

} // namespace slrhip
