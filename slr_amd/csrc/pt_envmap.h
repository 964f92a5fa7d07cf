// pt_envmap.h — the environment map's preprocessing: what the reference does to an image before and while it becomes the
// environment sphere's importance distribution.  ONE definition of every step for the host (slrhip_env_importance,
// slrhip_env_texels_to_uvs: host_util.cpp; prepareEnvironment: scene_prep.cpp) and the kernels of slrhip_set_environment
// (pt_envmap.hip).  float32 operations in the order written (both sides are built with -ffp-contract=off), the steps with double
// literals in double, so host and device agree bit for bit.  No library call is made here: the one the tables need, the sine of a
// row's polar angle, is evaluated on the host for both sides (envSinRow) and handed in.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "pt_luminance.h"          // SLR_HOST_DEV

namespace slrhip {

// A value as the reference's RGBA16F / uvsA16F image holds it (Core/Image.h:38-40): binary16, round to nearest even, subnormals
// kept, beyond 65504 infinity.
SLR_HOST_DEV float envHalf(float v) { return (float)(_Float16)v; }

// CompensatedSum<float>, BasicTypes/CompensatedSum.h:15-32
struct EnvSum {
    float result = 0.0f, comp = 0.0f;
    SLR_HOST_DEV void add(float value) {
        const float cInput = value - comp;
        const float sumTemp = result + cInput;
        comp = (sumTemp - result) - cInput;
        result = sumTemp;
    }
};

// Image2D::areaAverage over one 4x4 block of one component (Core/Image.cpp:19-120): the corner, edge and interior texels are
// added in that order with unit coefficients, the sum is divided by the area and stored back as binary16.  b[4 y + x]: the block.
SLR_HOST_DEV float envAreaAverage(const float b[16]) {
    EnvSum sum;
    sum.add(1.0f * b[0]);  sum.add(1.0f * b[3]);  sum.add(1.0f * b[12]); sum.add(1.0f * b[15]);     // corners UL, UR, LL, LR
    sum.add(1.0f * b[1]);  sum.add(1.0f * b[13]); sum.add(1.0f * b[2]);  sum.add(1.0f * b[14]);     // top / bottom edges, interleaved
    sum.add(1.0f * b[4]);  sum.add(1.0f * b[7]);  sum.add(1.0f * b[8]);  sum.add(1.0f * b[11]);     // left / right edges
    sum.add(1.0f * b[5]);  sum.add(1.0f * b[6]);  sum.add(1.0f * b[9]);  sum.add(1.0f * b[10]);     // interior
    return envHalf(sum.result / 16.0f);
}

// The luminance createIBLImportanceMap's pickFunc takes of the averaged texel (Textures/image_textures.cpp:81-108,131).
SLR_HOST_DEV float envLuminance(float r, float g, float b) { return (0.222485f * r + 0.716905f * g) + 0.060610f * b; }

// RGB build: the averaged texel is (r, g, b).
SLR_HOST_DEV float envImportanceRGB(float a0, float a1, float a2) { return envLuminance(a0, a1, a2); }

// Spectral build: the averaged texel is (u, v, s); Upsampling::uvs_to_sRGB (BasicTypes/Spectrum.h:174-195, Illuminant): uv_to_xy,
// XYZ = (x s, y s, s - X - Y), XYZ_to_sRGB (double literals, float operands and results), then the same luminance.
SLR_HOST_DEV float envImportanceUVS(float au, float av, float as) {
    const float x = (float)(0.0491440520940413 * au - 0.02361291916573777 * av + 0.13292069743203658);
    const float y = (float)(0.022853819546830627 * au + 0.05077639329371236 * av - 0.006895157122499944);
    const float X = x * as, Y = y * as;
    const float Z = (as - X) - Y;
    const float r = (float)(3.2404542 * X - 1.5371385 * Y - 0.4985314 * Z);
    const float g = (float)(-0.9692660 * X + 1.8760108 * Y + 0.0415560 * Z);
    const float b = (float)(0.0556434 * X - 0.2040259 * Y + 1.0572252 * Z);
    return envLuminance(r, g, b);
}

// What the reference's spectral build stores for a texel of an RGB radiance image: Upsampling::sRGB_to_uvs (Spectrum.h:148-171,
// Illuminant): sRGB_to_XYZ with double literals, b = X + Y + Z, xy (one third each for a black texel), xy_to_uv, s = b; kept as halves.
SLR_HOST_DEV void envRgbToUvs(float r, float g, float b, float& u, float& v, float& s) {
    const float X = (float)(0.4124564 * r + 0.3575761 * g + 0.1804375 * b);
    const float Y = (float)(0.2126729 * r + 0.7151522 * g + 0.0721750 * b);
    const float Z = (float)(0.0193339 * r + 0.1191920 * g + 0.9503041 * b);
    const float sum = (X + Y) + Z;
    const float x = sum == 0 ? (float)(1.0 / 3.0) : X / sum;
    const float y = sum == 0 ? (float)(1.0 / 3.0) : Y / sum;
    u = envHalf((float)(16.730260708356887 * x + 7.7801960340706 * y - 2.170152247475828));
    v = envHalf((float)(-7.530081094743006 * x + 16.192422314095225 * y + 1.1125529268825947));
    s = envHalf(sum);
}

// The function the 2-D distribution is built over (image_textures.cpp:126-133): sin(theta) of the row times the cell's importance.
// sinRow = envSinRow(y, mapHeight), evaluated on the HOST for both sides: a device libm's sine need not round as the host's does.
SLR_HOST_DEV float envRowValue(double sinRow, float importance) { return (float)(sinRow * importance); }
inline double envSinRow(uint32_t y, uint32_t mapHeight) { return std::sin(M_PI * (y + 0.5f) / mapHeight); }

// RegularConstantContinuous1D's constructor (Core/distributions.cpp:127-147) in its two steps, so that a kernel can spread them over
// lanes while the sum itself stays the sequential chain it is: CDF[i + 1] = envCdfStep(sum, PDF[i], n) for i = 0 .. n - 1 in index
// order (CDF[0] = 0), then PDF[i] and CDF[i + 1] are each divided by sum.result, which is the integral.
SLR_HOST_DEV float envCdfStep(EnvSum& sum, float pdf, uint32_t n) { sum.add(pdf / n); return sum.result; }

inline float envBuild1D(float* PDF, float* CDF, uint32_t n) {
    EnvSum sum;
    CDF[0] = 0.0f;
    for (uint32_t i = 0; i < n; ++i) CDF[i + 1] = envCdfStep(sum, PDF[i], n);
    for (uint32_t i = 0; i < n; ++i) { PDF[i] /= sum.result; CDF[i + 1] /= sum.result; }
    return sum.result;
}

#ifdef __HIP__
// slrhip_set_environment's device work (pt_envmap.hip): store the texels, build the importance map, the row distributions and the top
// distribution: five launches on `stream`.  The sizes have passed environmentRefusal (render_plan.h).
static const uint32_t kEnvMaxMapSide = 8192;               // 32768 / 4: the top distribution's integrals fit one workgroup's LDS
struct EnvBuild {
    uint32_t width, height, mapWidth, mapHeight;           // mapWidth = width / 4, mapHeight = height / 4
    bool spectral, storeHalf, toUvs;                       // importance of (u, v, s) texels; SLRHIP_ENV_STORE_HALF; TEXELS_RGB in a spectral context
    const float* src;                                      // the caller's texels, 16-byte aligned
    float* texels;                                         // the context's copy [height][width][3]
    float* importance;                                     // [mapHeight][mapWidth]
    const double* sinRow;                                  // [mapHeight], evaluated on the host (envSinRow)
    float* topPDF; float* topCDF;                          // [mapHeight], [mapHeight + 1]
    float* rowPDF; float* rowCDF;                          // [mapHeight][mapWidth], [mapHeight][mapWidth + 1]
};
void launchEnvBuild(const EnvBuild& e, hipStream_t stream);
#endif

} // namespace slrhip
