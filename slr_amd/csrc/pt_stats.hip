// pt_stats.hip — read-out of the per-pixel noise records k_fold keeps when statistics are on (slrhip_statistics_begin):
// one channel as a frame (k_record_resolve) and the shard's totals (k_record_summary, two stages); the same two read-outs, from the
// same templates, of the clamp records (slrhip_clamp_begin).  gfx950, wave64.
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

// What the read-outs need to know of a record kind, by its totals struct: one channel's value of a record, a record added to
// totals, totals added to totals (both in the fixed order of the fields), and the __shfl_down of totals field by field.
template <typename Totals> struct RecordTraits;

template <> struct RecordTraits<StatsTotals> {
    static __device__ __forceinline__ float channel(const float4& r, uint32_t channel) {
        const StatsValues v = statsValues(r);
        return channel == SLRHIP_STATISTICS_MEAN ? v.mean
               : channel == SLRHIP_STATISTICS_VARIANCE ? v.variance
               : channel == SLRHIP_STATISTICS_VARIANCE_OF_MEAN ? v.varianceOfMean
               : channel == SLRHIP_STATISTICS_COUNT ? v.count : v.maxSample;
    }
    static __device__ __forceinline__ void add(StatsTotals& a, const StatsTotals& b) {
        a.samples += b.samples; a.sumMean += b.sumMean; a.sumMeanSq += b.sumMeanSq; a.sumVarianceOfMean += b.sumVarianceOfMean;
        a.maxSample = fmaxf(a.maxSample, b.maxSample);
    }
    static __device__ __forceinline__ void addRecord(StatsTotals& a, const float4& r) {
        const StatsValues v = statsValues(r);
        StatsTotals b{};
        b.samples = __float_as_uint(r.z); b.sumMean = (double)v.mean; b.sumMeanSq = (double)v.mean * (double)v.mean;
        b.sumVarianceOfMean = (double)v.varianceOfMean; b.maxSample = v.maxSample;
        add(a, b);
    }
    static __device__ __forceinline__ StatsTotals shflDown(const StatsTotals& t, int off) {
        StatsTotals b{};
        b.samples = __shfl_down((unsigned long long)t.samples, off); b.sumMean = __shfl_down(t.sumMean, off); b.sumMeanSq = __shfl_down(t.sumMeanSq, off);
        b.sumVarianceOfMean = __shfl_down(t.sumVarianceOfMean, off); b.maxSample = __shfl_down(t.maxSample, off);
        return b;
    }
    static __device__ __forceinline__ void finish(StatsTotals& t, uint32_t numPixels) { t.pixels = numPixels; }
};

// the clamp records {clamped, dropped (uint32 bits), removed, largest} (slrhip_clamp_begin)
template <> struct RecordTraits<ClampTotals> {
    static __device__ __forceinline__ float channel(const float4& r, uint32_t channel) {
        return channel == SLRHIP_CLAMP_CLAMPED ? (float)__float_as_uint(r.x)
               : channel == SLRHIP_CLAMP_DROPPED ? (float)__float_as_uint(r.y)
               : channel == SLRHIP_CLAMP_REMOVED ? r.z : r.w;
    }
    static __device__ __forceinline__ void add(ClampTotals& a, const ClampTotals& b) {
        a.clamped += b.clamped; a.dropped += b.dropped; a.removed += b.removed; a.largest = fmaxf(a.largest, b.largest);
    }
    static __device__ __forceinline__ void addRecord(ClampTotals& a, const float4& r) {
        ClampTotals b{};
        b.clamped = __float_as_uint(r.x); b.dropped = __float_as_uint(r.y); b.removed = (double)r.z; b.largest = r.w;
        add(a, b);
    }
    static __device__ __forceinline__ ClampTotals shflDown(const ClampTotals& t, int off) {
        ClampTotals b{};
        b.clamped = __shfl_down((unsigned long long)t.clamped, off); b.dropped = __shfl_down((unsigned long long)t.dropped, off);
        b.removed = __shfl_down(t.removed, off); b.largest = __shfl_down(t.largest, off);
        return b;
    }
    static __device__ __forceinline__ void finish(ClampTotals&, uint32_t) {}
};

template <typename Totals>
__global__ __launch_bounds__(256) void k_record_resolve(const float4* __restrict__ records, const uint32_t* __restrict__ pixelXY, uint32_t numPixels,
                                                        uint32_t imageWidth, uint32_t channel, float* __restrict__ dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= numPixels) return;
    const uint32_t xy = pixelXY[pix];
    dst[(size_t)(xy >> 16) * imageWidth + (xy & 0xFFFFu)] = RecordTraits<Totals>::channel(records[pix], channel);
}

// The totals of the shard, deterministic: no floating-point atomics, and a grid that depends on the pixel count alone.
// Stage one: block b takes the pixels [b, b + 1) x kStatsBlock x kStatsPixelsPerThread; thread t adds pixels t, t + 256, ... of
// that range in order, the wave adds its lanes with __shfl_down (a fixed tree), thread 0 adds the waves' sums in wave order (LDS)
// and writes the block's partial.  Stage two: one thread adds the partials in index order.  A pixel past the end adds nothing.
template <typename Totals>
__global__ __launch_bounds__(kStatsBlock) void k_record_summary(const float4* __restrict__ records, uint32_t numPixels, Totals* __restrict__ partials) {
    using Traits = RecordTraits<Totals>;
    __shared__ Totals waves[kStatsBlock / 64];
    Totals t{};
    const uint32_t first = blockIdx.x * (kStatsBlock * kStatsPixelsPerThread) + threadIdx.x;
#pragma unroll 4
    for (uint32_t k = 0; k < kStatsPixelsPerThread; ++k) {
        const uint32_t pix = first + k * kStatsBlock;
        if (pix < numPixels) Traits::addRecord(t, records[pix]);
    }
    for (int off = 32; off > 0; off >>= 1) Traits::add(t, Traits::shflDown(t, off));
    if ((threadIdx.x & 63u) == 0u) waves[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kStatsBlock / 64; ++w) Traits::add(t, waves[w]);
        partials[blockIdx.x] = t;
    }
}
template <typename Totals>
__global__ __launch_bounds__(64) void k_record_summary_final(const Totals* __restrict__ partials, uint32_t numPartials, uint32_t numPixels,
                                                             Totals* __restrict__ out) {
    if (threadIdx.x != 0) return;
    Totals t{};
    for (uint32_t b = 0; b < numPartials; ++b) RecordTraits<Totals>::add(t, partials[b]);
    RecordTraits<Totals>::finish(t, numPixels);          // the statistics' pixel count; the clamp's totals have none
    *out = t;
}

template <typename Totals>
void launchRecordResolve(const float4* records, const uint32_t* pixelXY, uint32_t numPixels, uint32_t imageWidth, uint32_t channel, float* dst,
                         hipStream_t stream) {
    if (numPixels == 0) return;
    hipLaunchKernelGGL(k_record_resolve<Totals>, dim3((numPixels + 255) / 256), dim3(256), 0, stream, records, pixelXY, numPixels, imageWidth, channel, dst);
}
template <typename Totals>
void launchRecordSummary(const float4* records, uint32_t numPixels, Totals* partials, Totals* out, hipStream_t stream) {
    const uint32_t blocks = statsSummaryBlocks(numPixels);
    if (blocks) hipLaunchKernelGGL(k_record_summary<Totals>, dim3(blocks), dim3(kStatsBlock), 0, stream, records, numPixels, partials);
    hipLaunchKernelGGL(k_record_summary_final<Totals>, dim3(1), dim3(64), 0, stream, partials, blocks, numPixels, out);
}
template void launchRecordResolve<StatsTotals>(const float4*, const uint32_t*, uint32_t, uint32_t, uint32_t, float*, hipStream_t);
template void launchRecordResolve<ClampTotals>(const float4*, const uint32_t*, uint32_t, uint32_t, uint32_t, float*, hipStream_t);
template void launchRecordSummary<StatsTotals>(const float4*, uint32_t, StatsTotals*, StatsTotals*, hipStream_t);
template void launchRecordSummary<ClampTotals>(const float4*, uint32_t, ClampTotals*, ClampTotals*, hipStream_t);

} // namespace slrhip
