// pt_denoise.hip — device code of slrhip_denoise: the variance-guided a-trous filter defined in include/slrhip.h.  One prepare launch
// (k_denoise_prepare: the guide record and the first {Y, v} record of every pixel), then one launch per iteration
// (k_denoise_iteration: one thread per pixel gathers its 25 taps).  gfx950, wave64.
//
// Every float operation is written as its IEEE-rounded intrinsic (__fmul_rn, __fadd_rn, __fsub_rn, __fdiv_rn) and the square root as
// sqrtf, which hipcc rounds correctly by default (__fsqrt_rn is NOT that: without OCML_BASIC_ROUNDED_OPERATIONS it is the native,
// approximate root).  The definition has no fused multiply-add, and each pixel's sums are formed by ONE thread in the definition's
// order (dy outer, dx inner), so the result depends neither on scheduling nor on the tile shape.
#include "../../include/slrhip.h"
#include "pt_kernels.h"
#include "pt_luminance.h"

namespace slrhip {

namespace {

// A workgroup is a tile of 64 x 4 pixels, a wave one row of it: the lanes of a wave read consecutive records for every tap.
const uint32_t kDenoiseTileX = 64, kDenoiseTileY = 4;
const uint32_t kDenoiseGuides = 1u, kDenoiseNormal = 2u, kDenoiseDistance = 4u, kDenoiseLuminance = 8u;      // DenoiseIteration::flags

// A miss is marked in the guide record by n.x = -INFINITY.  A hit pixel never holds it: n.x = Nx / len is formed only when
// len > 0, an infinite Nx makes len infinite and the quotient NaN, and for finite Nx a finite len is at least sqrtf(fl(Nx * Nx)),
// about |Nx| (or Nx * Nx underflowed, and then |Nx| < len): the quotient is of the order of 1.
__device__ __forceinline__ bool guideHit(const float4& g) { return !(g.x == -INFINITY); }

template <int C>
__device__ __forceinline__ float denoiseLuminance(const float* c) {
    if (C == 3) return sampleLuminanceRGB(c[0], c[1], c[2]);
    float p[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) p[q] = sampleLuminancePlane(q, c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
    return sampleLuminanceOfPlanes(__fadd_rn(p[0], p[1]), __fadd_rn(p[2], p[3]));
}

// The colour of pixel q: from the caller's [H][W][C] floats (4-byte aligned) or from a scratch plane of float4s.
template <int C, bool kCaller>
__device__ __forceinline__ void denoiseLoadColor(const float* __restrict__ color, const float4* __restrict__ plane, uint32_t q, float* c) {
    if (kCaller) {
        const float* s = color + (size_t)q * C;
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = s[k];
    }
    else if (C == 3) {
        const float4 v = plane[q];
        c[0] = v.x; c[1] = v.y; c[2] = v.z;
    }
    else {
#pragma unroll
        for (int j = 0; j < C / 4; ++j) {
            const float4 v = plane[(size_t)q * (C / 4) + j];
            c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
        }
    }
}

struct DenoisePrepare {
    uint32_t numPixels;
    const float* color; const float* variance; const float* normal; const float* distance; const float* coverage;
    float4* guides; float2* yv;
};

template <int C>
__global__ __launch_bounds__(256) void k_denoise_prepare(DenoisePrepare a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.numPixels) return;
    float c[C];
    denoiseLoadColor<C, true>(a.color, nullptr, p, c);
    a.yv[p] = make_float2(denoiseLuminance<C>(c), a.variance ? a.variance[p] : 0.0f);
    if (!a.coverage) return;                               // no hit classes: the guide records are not read
    const float cov = a.coverage[p];
    float4 g = make_float4(-INFINITY, 0.0f, 0.0f, 0.0f);
    if (cov > 0.0f) {
        g.x = 0.0f;
        if (a.normal) {
            const float nx = a.normal[(size_t)p * 3], ny = a.normal[(size_t)p * 3 + 1], nz = a.normal[(size_t)p * 3 + 2];
            const float len = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(nx, nx), __fmul_rn(ny, ny)), __fmul_rn(nz, nz)));
            if (len > 0.0f) { g.x = __fdiv_rn(nx, len); g.y = __fdiv_rn(ny, len); g.z = __fdiv_rn(nz, len); }
        }
        if (a.distance) g.w = __fdiv_rn(a.distance[p], cov);
    }
    a.guides[p] = g;
}

struct DenoiseIteration {
    uint32_t width, height, tilesX, step, flags, normalPowerLog2;
    float sigmaLuminance, sigmaDistance;
    const float* colorIn;         // first iteration: the caller's colour
    const float4* planeIn;        // later ones: the plane the iteration before wrote
    float4* planeOut;             // all but the last
    float* output;                // the last: the caller's output and (may be null) output_variance
    float* outputVariance;
    const float4* guides;
    const float2* yvIn;           // {Y(c), v} of this iteration's input
    float2* yvOut;
};

template <int C, bool kFirst, bool kLast>
__global__ __launch_bounds__(256) void k_denoise_iteration(DenoiseIteration it) {
    const uint32_t x = (blockIdx.x % it.tilesX) * kDenoiseTileX + (threadIdx.x & 63u);
    const uint32_t y = (blockIdx.x / it.tilesX) * kDenoiseTileY + (threadIdx.x >> 6);
    if (x >= it.width || y >= it.height) return;
    const uint32_t p = y * it.width + x;
    const bool guides = (it.flags & kDenoiseGuides) != 0u;
    const float4 gP = guides ? it.guides[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const bool hitP = guides && guideHit(gP);
    const bool stopN = hitP && (it.flags & kDenoiseNormal), stopZ = hitP && (it.flags & kDenoiseDistance);
    const bool stopL = (it.flags & kDenoiseLuminance) != 0u;
    const float2 yvP = it.yvIn[p];

    // sigma_luminance * sd_p + 1e-20f, sd_p from the 3 x 3 prefilter of v (offsets of one pixel, in-image taps, row-major)
    float denomL = 1.0f;
    if (stopL) {
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const uint32_t qx = x + (uint32_t)dx, qy = y + (uint32_t)dy;      // a negative coordinate wraps to >= 2^32 - 1
                if (qx >= it.width || qy >= it.height) continue;
                const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
                const float v = (dx == 0 && dy == 0) ? yvP.y : it.yvIn[qy * it.width + qx].y;
                num = __fadd_rn(num, __fmul_rn(g, v));
                den = __fadd_rn(den, g);
            }
        }
        const float sd = sqrtf(fmaxf(0.0f, __fdiv_rn(num, den)));
        denomL = __fadd_rn(__fmul_rn(it.sigmaLuminance, sd), 1e-20f);
    }

    float acc[C];
#pragma unroll
    for (int k = 0; k < C; ++k) acc[k] = 0.0f;
    float accV = 0.0f, sumW = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            // x, y < 2^31 and |offset| <= 256: a tap left of or above the image wraps past 2^32 - 257, one right of or below it does not wrap
            const uint32_t qx = x + (uint32_t)(dx * (int)it.step), qy = y + (uint32_t)(dy * (int)it.step);
            if (qx >= it.width || qy >= it.height) continue;
            const uint32_t q = qy * it.width + qx;
            const float hx = dx == 0 ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f;
            const float hy = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
            float w = hx * hy;                             // exact: a constant of the unrolled loop
            float2 yvQ = yvP;
            if (dx != 0 || dy != 0) {
                if (guides) {
                    const float4 gQ = it.guides[q];
                    if (guideHit(gQ) != hitP) continue;
                    if (stopN) {
                        float t = fmaxf(0.0f, __fadd_rn(__fadd_rn(__fmul_rn(gP.x, gQ.x), __fmul_rn(gP.y, gQ.y)), __fmul_rn(gP.z, gQ.z)));
                        for (uint32_t k = 0; k < it.normalPowerLog2; ++k) t = __fmul_rn(t, t);
                        w = __fmul_rn(w, t);
                    }
                    if (stopZ) {
                        const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
                        const float d = (float)(it.step * (uint32_t)(ax > ay ? ax : ay));
                        const float xz = __fdiv_rn(fabsf(__fsub_rn(gP.w, gQ.w)), __fmul_rn(__fmul_rn(it.sigmaDistance, d), gP.w));
                        const float t = fmaxf(0.0f, __fsub_rn(1.0f, xz));
                        w = __fmul_rn(w, __fmul_rn(t, t));
                    }
                }
                yvQ = it.yvIn[q];
                if (stopL) {
                    const float xl = __fdiv_rn(fabsf(__fsub_rn(yvP.x, yvQ.x)), denomL);
                    const float t = fmaxf(0.0f, __fsub_rn(1.0f, xl));
                    w = __fmul_rn(w, __fmul_rn(t, t));
                }
            }
            if (w != 0.0f) {                               // (a NaN weight is added, and spreads)
                float c[C];
                denoiseLoadColor<C, kFirst>(it.colorIn, it.planeIn, q, c);
#pragma unroll
                for (int k = 0; k < C; ++k) acc[k] = __fadd_rn(acc[k], __fmul_rn(w, c[k]));
                accV = __fadd_rn(accV, __fmul_rn(__fmul_rn(w, w), yvQ.y));
                sumW = __fadd_rn(sumW, w);
            }
        }
    }

    float out[C];
#pragma unroll
    for (int k = 0; k < C; ++k) out[k] = __fdiv_rn(acc[k], sumW);
    const float vOut = __fdiv_rn(accV, __fmul_rn(sumW, sumW));
    if (kLast) {
        float* o = it.output + (size_t)p * C;
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = out[k];
        if (it.outputVariance) it.outputVariance[p] = vOut;
    }
    else {
        if (C == 3) it.planeOut[p] = make_float4(out[0], out[1], out[2], 0.0f);
        else {
#pragma unroll
            for (int j = 0; j < C / 4; ++j) it.planeOut[(size_t)p * (C / 4) + j] = make_float4(out[4 * j], out[4 * j + 1], out[4 * j + 2], out[4 * j + 3]);
        }
        it.yvOut[p] = make_float2(denoiseLuminance<C>(out), vOut);
    }
}

template <int C>
void launchIteration(const DenoiseIteration& it, bool first, bool last, dim3 grid, hipStream_t stream) {
    const dim3 block(kDenoiseTileX * kDenoiseTileY);
    if (first && last) hipLaunchKernelGGL((k_denoise_iteration<C, true, true>), grid, block, 0, stream, it);
    else if (first) hipLaunchKernelGGL((k_denoise_iteration<C, true, false>), grid, block, 0, stream, it);
    else if (last) hipLaunchKernelGGL((k_denoise_iteration<C, false, true>), grid, block, 0, stream, it);
    else hipLaunchKernelGGL((k_denoise_iteration<C, false, false>), grid, block, 0, stream, it);
}

} // namespace

void launchDenoise(const DenoiseParams& dp, hipStream_t stream) {
    const uint32_t numPixels = dp.width * dp.height;       // < 2^31 (checked by the caller)
    const DenoisePrepare prep{numPixels, dp.color, dp.variance, dp.normal, dp.distance, dp.coverage, dp.guides, dp.yv[0]};
    const dim3 prepGrid((numPixels + 255u) / 256u), prepBlock(256);
    if (dp.components == 3) hipLaunchKernelGGL(k_denoise_prepare<3>, prepGrid, prepBlock, 0, stream, prep);
    else hipLaunchKernelGGL(k_denoise_prepare<16>, prepGrid, prepBlock, 0, stream, prep);

    DenoiseIteration it{};
    it.width = dp.width; it.height = dp.height;
    it.tilesX = (dp.width + kDenoiseTileX - 1) / kDenoiseTileX;
    // tilesX * tilesY < 2^23 + 2^25 + 2^29 + 1 for width * height < 2^31: one grid dimension holds it
    const dim3 grid(it.tilesX * ((dp.height + kDenoiseTileY - 1) / kDenoiseTileY));
    it.flags = (dp.coverage ? kDenoiseGuides : 0u) | (dp.coverage && dp.normal ? kDenoiseNormal : 0u) |
               (dp.coverage && dp.distance && dp.sigmaDistance > 0.0f ? kDenoiseDistance : 0u) |
               (dp.variance && dp.sigmaLuminance > 0.0f ? kDenoiseLuminance : 0u);
    it.normalPowerLog2 = dp.normalPowerLog2;
    it.sigmaLuminance = dp.sigmaLuminance; it.sigmaDistance = dp.sigmaDistance;
    it.colorIn = dp.color; it.output = dp.output; it.outputVariance = dp.outputVariance;
    it.guides = dp.guides;
    for (uint32_t i = 0; i < dp.iterations; ++i) {
        it.step = 1u << i;
        it.planeIn = dp.planes[(i + 1u) & 1u];             // what iteration i - 1 wrote
        it.planeOut = dp.planes[i & 1u];
        it.yvIn = dp.yv[i & 1u];
        it.yvOut = dp.yv[(i + 1u) & 1u];
        if (dp.components == 3) launchIteration<3>(it, i == 0, i + 1 == dp.iterations, grid, stream);
        else launchIteration<16>(it, i == 0, i + 1 == dp.iterations, grid, stream);
    }
}

} // namespace slrhip
