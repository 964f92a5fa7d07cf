// pt_stats.hip — read-out of the per-pixel noise records k_fold keeps when statistics are on (slrhip_statistics_begin):
// one channel as a frame (k_stats_resolve) and the shard's totals (k_stats_summary, two stages); the same two read-outs of the
// clamp records (slrhip_clamp_begin).  gfx950, wave64.
#include "../../include/slrhip.h"
#include "pt_kernels.h"

namespace slrhip {

// The channels of a record {mean, M2, n, max}, in float32.  The sample variance is M2 / (n - 1) and the variance of the mean
// M2 / ((n - 1) n), both 0 while n < 2; the divisor of the latter is the float32 product (float)(n - 1) * (float)n.
struct StatsValues { float mean, variance, varianceOfMean, count, maxSample; };
__device__ __forceinline__ StatsValues statsValues(const float4& r) {
    const uint32_t n = __float_as_uint(r.z);
    StatsValues v;
    v.mean = r.x; v.count = (float)n; v.maxSample = r.w;
    v.variance = n < 2u ? 0.0f : r.y / (float)(n - 1u);
    v.varianceOfMean = n < 2u ? 0.0f : r.y / ((float)(n - 1u) * (float)n);
    return v;
}

__global__ __launch_bounds__(256) void k_stats_resolve(const float4* __restrict__ records, const uint32_t* __restrict__ pixelXY, uint32_t numPixels,
                                                       uint32_t imageWidth, uint32_t channel, float* __restrict__ dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= numPixels) return;
    const uint32_t xy = pixelXY[pix];
    const StatsValues v = statsValues(records[pix]);
    dst[(size_t)(xy >> 16) * imageWidth + (xy & 0xFFFFu)] = channel == SLRHIP_STATISTICS_MEAN ? v.mean
                                                            : channel == SLRHIP_STATISTICS_VARIANCE ? v.variance
                                                            : channel == SLRHIP_STATISTICS_VARIANCE_OF_MEAN ? v.varianceOfMean
                                                            : channel == SLRHIP_STATISTICS_COUNT ? v.count : v.maxSample;
}

// The totals of the shard, deterministic: no floating-point atomics, and a grid that depends on the pixel count alone.
// Stage one: block b takes the pixels [b, b + 1) x kStatsBlock x kStatsPixelsPerThread; thread t adds pixels t, t + 256, ... of
// that range in order, the wave adds its lanes with __shfl_down (a fixed tree), thread 0 adds the waves' sums in wave order (LDS)
// and writes the block's partial.  Stage two: one thread adds the partials in index order.  A pixel past the end adds zeros.
__device__ __forceinline__ void statsAdd(StatsTotals& a, uint64_t samples, double mean, double meanSq, double vom, float mx) {
    a.samples += samples; a.sumMean += mean; a.sumMeanSq += meanSq; a.sumVarianceOfMean += vom; a.maxSample = fmaxf(a.maxSample, mx);
}
__global__ __launch_bounds__(kStatsBlock) void k_stats_summary(const float4* __restrict__ records, uint32_t numPixels, StatsTotals* __restrict__ partials) {
    __shared__ StatsTotals waves[kStatsBlock / 64];
    StatsTotals t{};
    const uint32_t first = blockIdx.x * (kStatsBlock * kStatsPixelsPerThread) + threadIdx.x;
#pragma unroll 4
    for (uint32_t k = 0; k < kStatsPixelsPerThread; ++k) {
        const uint32_t pix = first + k * kStatsBlock;
        if (pix < numPixels) {
            const float4 r = records[pix];
            const StatsValues v = statsValues(r);
            statsAdd(t, __float_as_uint(r.z), (double)v.mean, (double)v.mean * (double)v.mean, (double)v.varianceOfMean, v.maxSample);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        statsAdd(t, __shfl_down((unsigned long long)t.samples, off), __shfl_down(t.sumMean, off), __shfl_down(t.sumMeanSq, off),
                 __shfl_down(t.sumVarianceOfMean, off), __shfl_down(t.maxSample, off));
    if ((threadIdx.x & 63u) == 0u) waves[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kStatsBlock / 64; ++w) statsAdd(t, waves[w].samples, waves[w].sumMean, waves[w].sumMeanSq, waves[w].sumVarianceOfMean, waves[w].maxSample);
        partials[blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(64) void k_stats_summary_final(const StatsTotals* __restrict__ partials, uint32_t numPartials, uint32_t numPixels,
                                                            StatsTotals* __restrict__ out) {
    if (threadIdx.x != 0) return;
    StatsTotals t{};
    for (uint32_t b = 0; b < numPartials; ++b) statsAdd(t, partials[b].samples, partials[b].sumMean, partials[b].sumMeanSq, partials[b].sumVarianceOfMean, partials[b].maxSample);
    t.pixels = numPixels;
    *out = t;
}

// ---- the clamp records {clamped, dropped (uint32 bits), removed, largest} (slrhip_clamp_begin) ----
__global__ __launch_bounds__(256) void k_clamp_resolve(const float4* __restrict__ records, const uint32_t* __restrict__ pixelXY, uint32_t numPixels,
                                                       uint32_t imageWidth, uint32_t channel, float* __restrict__ dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= numPixels) return;
    const uint32_t xy = pixelXY[pix];
    const float4 r = records[pix];
    dst[(size_t)(xy >> 16) * imageWidth + (xy & 0xFFFFu)] = channel == SLRHIP_CLAMP_CLAMPED ? (float)__float_as_uint(r.x)
                                                            : channel == SLRHIP_CLAMP_DROPPED ? (float)__float_as_uint(r.y)
                                                            : channel == SLRHIP_CLAMP_REMOVED ? r.z : r.w;
}

// The totals, in the shape and with the grid of k_stats_summary: the same fixed order of additions.
__device__ __forceinline__ void clampAdd(ClampTotals& a, uint64_t clamped, uint64_t dropped, double removed, float largest) {
    a.clamped += clamped; a.dropped += dropped; a.removed += removed; a.largest = fmaxf(a.largest, largest);
}
__global__ __launch_bounds__(kStatsBlock) void k_clamp_summary(const float4* __restrict__ records, uint32_t numPixels, ClampTotals* __restrict__ partials) {
    __shared__ ClampTotals waves[kStatsBlock / 64];
    ClampTotals t{};
    const uint32_t first = blockIdx.x * (kStatsBlock * kStatsPixelsPerThread) + threadIdx.x;
#pragma unroll 4
    for (uint32_t k = 0; k < kStatsPixelsPerThread; ++k) {
        const uint32_t pix = first + k * kStatsBlock;
        if (pix < numPixels) {
            const float4 r = records[pix];
            clampAdd(t, __float_as_uint(r.x), __float_as_uint(r.y), (double)r.z, r.w);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        clampAdd(t, __shfl_down((unsigned long long)t.clamped, off), __shfl_down((unsigned long long)t.dropped, off), __shfl_down(t.removed, off),
                 __shfl_down(t.largest, off));
    if ((threadIdx.x & 63u) == 0u) waves[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kStatsBlock / 64; ++w) clampAdd(t, waves[w].clamped, waves[w].dropped, waves[w].removed, waves[w].largest);
        partials[blockIdx.x] = t;
    }
}
__global__ __launch_bounds__(64) void k_clamp_summary_final(const ClampTotals* __restrict__ partials, uint32_t numPartials, ClampTotals* __restrict__ out) {
    if (threadIdx.x != 0) return;
    ClampTotals t{};
    for (uint32_t b = 0; b < numPartials; ++b) clampAdd(t, partials[b].clamped, partials[b].dropped, partials[b].removed, partials[b].largest);
    *out = t;
}

void launchClampResolve(const float4* records, const uint32_t* pixelXY, uint32_t numPixels, uint32_t imageWidth, uint32_t channel, float* dst,
                        hipStream_t stream) {
    if (numPixels == 0) return;
    hipLaunchKernelGGL(k_clamp_resolve, dim3((numPixels + 255) / 256), dim3(256), 0, stream, records, pixelXY, numPixels, imageWidth, channel, dst);
}
void launchClampSummary(const float4* records, uint32_t numPixels, ClampTotals* partials, ClampTotals* out, hipStream_t stream) {
    const uint32_t blocks = statsSummaryBlocks(numPixels);
    if (blocks) hipLaunchKernelGGL(k_clamp_summary, dim3(blocks), dim3(kStatsBlock), 0, stream, records, numPixels, partials);
    hipLaunchKernelGGL(k_clamp_summary_final, dim3(1), dim3(64), 0, stream, partials, blocks, out);
}

void launchStatsResolve(const float4* records, const uint32_t* pixelXY, uint32_t numPixels, uint32_t imageWidth, uint32_t channel, float* dst,
                        hipStream_t stream) {
    if (numPixels == 0) return;
    hipLaunchKernelGGL(k_stats_resolve, dim3((numPixels + 255) / 256), dim3(256), 0, stream, records, pixelXY, numPixels, imageWidth, channel, dst);
}
void launchStatsSummary(const float4* records, uint32_t numPixels, StatsTotals* partials, StatsTotals* out, hipStream_t stream) {
    const uint32_t blocks = statsSummaryBlocks(numPixels);
    if (blocks) hipLaunchKernelGGL(k_stats_summary, dim3(blocks), dim3(kStatsBlock), 0, stream, records, numPixels, partials);
    hipLaunchKernelGGL(k_stats_summary_final, dim3(1), dim3(64), 0, stream, partials, blocks, numPixels, out);
}

} // namespace slrhip
