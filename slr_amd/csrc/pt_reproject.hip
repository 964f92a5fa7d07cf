// pt_reproject.hip — device code of slrhip_reproject: the temporal reprojection defined in include/slrhip.h.  One launch, one lane per
// pixel: a bandwidth-bound gather of up to four taps of the previous frame.  gfx950, wave64.
//
// A lane first decides the validity of its four taps from the small guide planes (coverage, length, ids, distance, normal: 4 to 12
// bytes per tap) and only then reads the colour of the taps that passed and carry weight — the 12- or 64-byte records that make up
// most of the traffic.  A 16-component pixel stays with ONE lane, which reads its 64 bytes as four float4s where the caller's buffers
// are 16-byte aligned: four lanes per pixel (a wave's tap load 1 KiB of consecutive bytes, the luminance through two quad exchanges)
// gave the same bits and measured 1.6 times slower, because every lane of a quad repeats the guide phase.  Every float operation is rounded on its own (the unit is built with -ffp-contract=off) and each pixel's
// sums are formed by ONE thread in the definition's order (j outer, i inner), so the result does not depend on scheduling.
#include "../../include/slrhip.h"
#include "pt_kernels.h"
#include "pt_luminance.h"

namespace slrhip {

namespace {

// A workgroup is a tile of 64 x 4 pixels, a wave one row of it (the denoiser's shape): with coherent motion the lanes of a wave read
// consecutive records of the previous frame for every tap.
const uint32_t kReprojectTileX = 64, kReprojectTileY = 4;

template <int C>
__device__ __forceinline__ float reprojectLuminance(const float* c) {
    if (C == 3) return sampleLuminanceRGB(c[0], c[1], c[2]);
    float p[4];
#pragma unroll
    for (uint32_t q = 0; q < 4; ++q) p[q] = sampleLuminancePlane(q, c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
    return sampleLuminanceOfPlanes(p[0] + p[1], p[2] + p[3]);
}

// kVec: the frame is 16-byte aligned and C is a multiple of 4
template <int C, bool kVec>
__device__ __forceinline__ void loadPixel(const float* __restrict__ frame, uint32_t q, float* c) {
    if (kVec && C % 4 == 0) {
        const float4* s = reinterpret_cast<const float4*>(frame) + (size_t)q * (C / 4);
#pragma unroll
        for (int j = 0; j < C / 4; ++j) {
            const float4 v = s[j];
            c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
        }
    }
    else {
        const float* s = frame + (size_t)q * C;
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = s[k];
    }
}
template <int C, bool kVec>
__device__ __forceinline__ void storePixel(float* __restrict__ frame, uint32_t q, const float* c) {
    if (kVec && C % 4 == 0) {
        float4* o = reinterpret_cast<float4*>(frame) + (size_t)q * (C / 4);
#pragma unroll
        for (int j = 0; j < C / 4; ++j) o[j] = make_float4(c[4 * j], c[4 * j + 1], c[4 * j + 2], c[4 * j + 3]);
    }
    else {
        float* o = frame + (size_t)q * C;
#pragma unroll
        for (int k = 0; k < C; ++k) o[k] = c[k];
    }
}

// the denoiser's normalisation of a sum of normals: N / len by division if len > 0, else zeros
__device__ __forceinline__ void unitNormal(const float* n, float& x, float& y, float& z) {
    const float nx = n[0], ny = n[1], nz = n[2];
    const float len = sqrtf(nx * nx + ny * ny + nz * nz);
    x = 0.0f; y = 0.0f; z = 0.0f;
    if (len > 0.0f) { x = nx / len; y = ny / len; z = nz / len; }
}

// The four taps of pixel p = (x, y), decided from the guide planes alone (the colour is not touched): weight, history length, index
// and validity so far, tap t = 2 j + i.  Returns false for a pixel that is rejected before any tap is looked at.
struct ReprojectTaps {
    float b[4], len[4];
    uint32_t q[4];
    bool ok[4];
};
__device__ __forceinline__ bool reprojectTaps(const slrhip_reproject_desc& d, uint32_t x, uint32_t y, uint32_t p, ReprojectTaps& taps) {
    const float cov = d.coverage[p];
    const float* mv = d.motion + (size_t)p * 4;
    const float n = mv[3];
    if (cov <= 0.0f || n <= 0.0f) return false;
    const float mx = mv[0] / n, my = mv[1] / n, ze = mv[2] / n;
    const float fx = (float)x + mx, fy = (float)y + my;
    const float x0 = floorf(fx), y0 = floorf(fy);
    const float tx = fx - x0, ty = fy - y0;
    float npx = 0.0f, npy = 0.0f, npz = 0.0f;
    if (d.normal) unitNormal(d.normal + (size_t)p * 3, npx, npy, npz);
    uint32_t instP = 0u, matP = 0u;
    if (d.ids) { instP = d.ids[(size_t)p * 3 + 1]; matP = d.ids[(size_t)p * 3 + 2]; }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int t = 2 * j + i;
            const float qxf = x0 + (float)i, qyf = y0 + (float)j;
            taps.b[t] = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty);
            taps.len[t] = 0.0f; taps.q[t] = 0u;
            // integer-valued floats below 2^31 convert exactly; a NaN fails the first comparison
            bool v = taps.b[t] != 0.0f && qxf >= 0.0f && qxf < 2147483648.0f && qyf >= 0.0f && qyf < 2147483648.0f;
            if (v) {
                const uint32_t qx = (uint32_t)qxf, qy = (uint32_t)qyf;
                v = qx < d.width && qy < d.height;
                if (v) {
                    const uint32_t q = qy * d.width + qx;
                    taps.q[t] = q;
                    const float covQ = d.prev_coverage[q];
                    taps.len[t] = d.prev_length[q];
                    v = covQ > 0.0f && taps.len[t] > 0.0f;
                    if (v && d.ids) v = d.prev_ids[(size_t)q * 3 + 1] == instP && d.prev_ids[(size_t)q * 3 + 2] == matP;
                    if (v && d.sigma_distance > 0.0f) v = fabsf(d.prev_distance[q] / covQ - ze) <= d.sigma_distance * ze;
                    if (v && d.normal) {
                        float nqx, nqy, nqz;
                        unitNormal(d.prev_normal + (size_t)q * 3, nqx, nqy, nqz);
                        v = npx * nqx + npy * nqy + npz * nqz >= d.min_normal_dot;
                    }
                }
            }
            taps.ok[t] = v;
        }
    }
    return true;
}

template <int C, bool kVec>
__global__ __launch_bounds__(256) void k_reproject(slrhip_reproject_desc d, uint32_t tilesX) {
    const uint32_t x = (blockIdx.x % tilesX) * kReprojectTileX + (threadIdx.x & 63u);
    const uint32_t y = (blockIdx.x / tilesX) * kReprojectTileY + (threadIdx.x >> 6);
    if (x >= d.width || y >= d.height) return;
    const uint32_t p = y * d.width + x;

    float out[C];
    loadPixel<C, kVec>(d.color, p, out);
    const float varP = d.variance ? d.variance[p] : 0.0f;
    float outLength = 1.0f, outVariance = varP;
    ReprojectTaps taps;
    if (reprojectTaps(d, x, y, p, taps)) {
        // the colour of the taps that passed; a tap whose luminance is not finite drops out here
        float acc[C];
#pragma unroll
        for (int k = 0; k < C; ++k) acc[k] = 0.0f;
        float B = 0.0f, accLength = 0.0f, accVariance = 0.0f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (!taps.ok[t]) continue;
            float c[C];
            loadPixel<C, kVec>(d.prev_color, taps.q[t], c);
            if (!(fabsf(reprojectLuminance<C>(c)) <= 3.402823466e+38f)) continue;
            B = B + taps.b[t];
#pragma unroll
            for (int k = 0; k < C; ++k) acc[k] = acc[k] + taps.b[t] * c[k];
            accLength = accLength + taps.b[t] * taps.len[t];
            if (d.variance) accVariance = accVariance + taps.b[t] * d.prev_variance[taps.q[t]];
        }
        if (!(B <= 0.0f)) {
            const float N = fminf(accLength / B + 1.0f, d.max_history);
            const float a = fmaxf(1.0f / N, d.min_alpha);
            const float keep = 1.0f - a;
#pragma unroll
            for (int k = 0; k < C; ++k) out[k] = keep * (acc[k] / B) + a * out[k];
            outLength = N;
            outVariance = (a * a) * varP + (keep * keep) * (accVariance / B);
        }
    }
    storePixel<C, kVec>(d.output, p, out);
    d.output_length[p] = outLength;
    if (d.output_variance) d.output_variance[p] = outVariance;
}

} // namespace

void launchReproject(const slrhip_reproject_desc& d, hipStream_t stream) {
    const uint32_t tilesX = (d.width + kReprojectTileX - 1) / kReprojectTileX;
    // tilesX * tilesY < 2^23 + 2^25 + 2^29 + 1 for width * height < 2^31 (checked by the caller): one grid dimension holds it
    const dim3 grid(tilesX * ((d.height + kReprojectTileY - 1) / kReprojectTileY)), block(kReprojectTileX * kReprojectTileY);
    const bool aligned = (((uintptr_t)d.color | (uintptr_t)d.prev_color | (uintptr_t)d.output) & 15u) == 0;
    if (d.components == 3) hipLaunchKernelGGL((k_reproject<3, false>), grid, block, 0, stream, d, tilesX);
    else if (aligned) hipLaunchKernelGGL((k_reproject<16, true>), grid, block, 0, stream, d, tilesX);
    else hipLaunchKernelGGL((k_reproject<16, false>), grid, block, 0, stream, d, tilesX);
}

} // namespace slrhip
