// pt_adaptive.hip — device code of slrhip_render_adaptive: the retirement check on the noise records with the compaction of the
// pixels that stay active (k_adaptive_count / _scan / _scatter), the fold of a window over the compact list back into the
// pixels of the shard (k_fold_indexed), and the mean resolve (k_resolve_mean).  gfx950, wave64.
#include "../../include/slrhip.h"
#include "pt_fold.h"

namespace slrhip {

// The contract of include/slrhip.h, one IEEE-rounded float32 operation per step (no fused multiply-add: __fmul_rn / __fdiv_rn).
// A NaN anywhere makes the last comparison false: such a pixel never retires.
__device__ __forceinline__ bool adaptiveRetires(const float4& r, float threshold, float floor) {
    const uint32_t n = __float_as_uint(r.z);
    if (n < 2u) return false;
    const float vom = __fdiv_rn(r.y, __fmul_rn((float)(n - 1u), (float)n));
    const float m = fmaxf(r.x, floor);
    const float a = __fmul_rn(threshold, m);
    return !(r.x != r.x) && vom <= __fmul_rn(a, a);
}

// Entry i (< prevCount) of the previous active list: the pixel of the shard and whether it stays active.  prevIndex == nullptr
// is the identity list (every pixel of the shard, before the first check).
__device__ __forceinline__ bool adaptiveStays(const AdaptiveSelect& a, uint32_t i, uint32_t& pixel) {
    pixel = 0u;
    if (i >= a.prevCount) return false;
    pixel = a.prevIndex ? a.prevIndex[i] : i;
    return !adaptiveRetires(a.records[pixel], a.threshold, a.floor);
}

// Stage one: workgroup b counts the entries [b, b + 1) x kAdaptiveBlock of the previous list that stay (a ballot and a population
// count per wave, the four wave counts added in wave order).
__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_count(AdaptiveSelect a) {
    __shared__ uint32_t waves[kAdaptiveBlock / 64];
    uint32_t pixel;
    const bool stays = adaptiveStays(a, blockIdx.x * kAdaptiveBlock + threadIdx.x, pixel);
    const uint64_t m = __ballot(stays);
    if ((threadIdx.x & 63u) == 0u) waves[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kAdaptiveBlock / 64; ++w) t += waves[w];
        a.blockOffsets[blockIdx.x] = t;
    }
}

// Stage two: the exclusive scan of the workgroup counts, in place, by one workgroup: chunks of kAdaptiveBlock counts, each scanned
// in LDS (Hillis-Steele: log2(256) = 8 steps) on top of the carry of the chunks before it.  The total is the new active count.
__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_scan(uint32_t* __restrict__ blockOffsets, uint32_t numBlocks, uint32_t* __restrict__ countWord) {
    __shared__ uint32_t buf[2][kAdaptiveBlock];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < numBlocks; base += kAdaptiveBlock) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t own = b < numBlocks ? blockOffsets[b] : 0u;
        uint32_t cur = 0;
        buf[0][threadIdx.x] = own;
        __syncthreads();
        for (uint32_t off = 1; off < kAdaptiveBlock; off <<= 1) {
            const uint32_t v = buf[cur][threadIdx.x] + (threadIdx.x >= off ? buf[cur][threadIdx.x - off] : 0u);
            buf[cur ^ 1u][threadIdx.x] = v;
            cur ^= 1u;
            __syncthreads();
        }
        const uint32_t inclusive = buf[cur][threadIdx.x];
        const uint32_t chunkTotal = buf[cur][kAdaptiveBlock - 1];
        if (b < numBlocks) blockOffsets[b] = carry + inclusive - own;
        carry += chunkTotal;
        __syncthreads();                       // buf is rewritten by the next chunk
    }
    if (threadIdx.x == 0) *countWord = carry;
}

// Stage three: the same decision again (the records have not changed), the entry's place = the workgroup's offset + the waves
// before it + the lanes before it in the ballot: a stable compaction, so the new list is in ascending shard-pixel order like the
// old one.  No atomics anywhere.
__global__ __launch_bounds__(kAdaptiveBlock) void k_adaptive_scatter(AdaptiveSelect a) {
    __shared__ uint32_t waves[kAdaptiveBlock / 64];
    uint32_t pixel;
    const bool stays = adaptiveStays(a, blockIdx.x * kAdaptiveBlock + threadIdx.x, pixel);
    const uint64_t m = __ballot(stays);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) waves[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (!stays) return;
    uint32_t at = a.blockOffsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) at += waves[w];
    at += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    a.nextXY[at] = a.shardXY[pixel];
    a.nextIndex[at] = pixel;
}

void launchAdaptiveSelect(const AdaptiveSelect& a, hipStream_t stream) {
    const uint32_t blocks = adaptiveSelectBlocks(a.prevCount);
    if (blocks) hipLaunchKernelGGL(k_adaptive_count, dim3(blocks), dim3(kAdaptiveBlock), 0, stream, a);
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), dim3(kAdaptiveBlock), 0, stream, a.blockOffsets, blocks, a.countWord);
    if (blocks) hipLaunchKernelGGL(k_adaptive_scatter, dim3(blocks), dim3(kAdaptiveBlock), 0, stream, a);
}

// k_fold over a compact window: element e of the window adds into the pixel indexMap[compact pixel of e] of the shard (pt_fold.h).
// Only with statistics: the adaptive render needs the records.  kClamp: as in k_fold.
template <bool kClamp, bool kSpectral>
__global__ __launch_bounds__(256) void k_fold_indexed(PathBuffers pb, uint32_t elems, uint32_t passes, float4* statRecords,
                                                      const uint32_t* __restrict__ indexMap, FoldClampArgs<kClamp> clamp) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= elems) return;
    foldElement<kClamp, true, kSpectral, true>(pb, e, elems, passes, statRecords, indexMap, clamp);
}

void launchFoldIndexed(const PathBuffers& pb, const RenderParams& rp, float4* statRecords, const uint32_t* indexMap, const ClampParams& clamp,
                       hipStream_t stream) {
    const uint32_t elems = rp.numPixels * (rp.spectral ? 4u : 1u);
    if (elems == 0 || rp.sppCount == 0) return;
    const dim3 grid((elems + 255) / 256), block(256);
    if (clamp.records) {
        FoldClampArgs<true> on;
        static_cast<ClampParams&>(on) = clamp;
        if (rp.spectral) hipLaunchKernelGGL((k_fold_indexed<true, true>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, indexMap, on);
        else hipLaunchKernelGGL((k_fold_indexed<true, false>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, indexMap, on);
        return;
    }
    const FoldClampArgs<false> off;
    if (rp.spectral) hipLaunchKernelGGL((k_fold_indexed<false, true>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, indexMap, off);
    else hipLaunchKernelGGL((k_fold_indexed<false, false>), grid, block, 0, stream, pb, elems, rp.sppCount, statRecords, indexMap, off);
}

// The mean frame: [H][W][N] = sum / (float)n with n from the pixel's noise record, 0 where n == 0 (dst cleared by the caller:
// pixels outside the shard stay 0).
__global__ __launch_bounds__(256) void k_resolve_mean(const float4* __restrict__ fbSum, const float4* __restrict__ records,
                                                      const uint32_t* __restrict__ pixelXY, uint32_t numPixels, uint32_t imageWidth, uint32_t planes,
                                                      float* __restrict__ dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= numPixels) return;
    const uint32_t xy = pixelXY[pix];
    const uint32_t n = __float_as_uint(records[pix].z);
    const float fn = (float)n;
    if (planes == 1u) {
        float* o = dst + ((size_t)(xy >> 16) * imageWidth + (xy & 0xFFFFu)) * 3u;
        const float4 v = fbSum[pix];
        o[0] = n ? __fdiv_rn(v.x, fn) : 0.0f; o[1] = n ? __fdiv_rn(v.y, fn) : 0.0f; o[2] = n ? __fdiv_rn(v.z, fn) : 0.0f;
    }
    else {
        float* o = dst + ((size_t)(xy >> 16) * imageWidth + (xy & 0xFFFFu)) * 16u;
        for (uint32_t k = 0; k < 4u; ++k) {
            const float4 v = fbSum[(size_t)pix * 4u + k];
            o[4 * k] = n ? __fdiv_rn(v.x, fn) : 0.0f; o[4 * k + 1] = n ? __fdiv_rn(v.y, fn) : 0.0f;
            o[4 * k + 2] = n ? __fdiv_rn(v.z, fn) : 0.0f; o[4 * k + 3] = n ? __fdiv_rn(v.w, fn) : 0.0f;
        }
    }
}

void launchResolveMean(const PathBuffers& pb, const RenderParams& rp, const float4* records, float* dst, hipStream_t stream) {
    if (rp.numPixels == 0) return;
    hipLaunchKernelGGL(k_resolve_mean, dim3((rp.numPixels + 255) / 256), dim3(256), 0, stream, pb.fbSum, records, pb.pixelXY, rp.numPixels,
                       rp.imageWidth, rp.spectral ? 4u : 1u, dst);
}

} // namespace slrhip
