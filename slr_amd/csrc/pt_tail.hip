// pt_tail.hip — launcher of the tail kernel (pt_tail_kernels.h): the twin of the window's k_shade variant, from the table of built
// kernels (pt_shade.hip); the instantiations are in pt_tail_{rgb,spec16}.hip and pt_tail_{multi,tex}_{rgb,spec}.hip.
#include <algorithm>

#include "pt_shade_variants.h"
#include "pt_slot_state.h"
#include "render_plan.h"

namespace slrhip {

// Live slots -> pb.tailList (numSlots entries).
__global__ __launch_bounds__(kShadeBlock) void k_tail_collect(PathBuffers pb, RenderParams rp) {
    __shared__ uint32_t waveCount[kShadeBlock / 64];
    __shared__ uint32_t base;
    if (pb.blockDead[blockIdx.x]) return;
    const uint32_t slot = blockIdx.x * kShadeBlock + threadIdx.x;
    const bool live = F_STATE(pb.flags[slot]) != ST_IDLE;
    const uint64_t m = __ballot(live);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) waveCount[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = waveCount[0] + waveCount[1] + waveCount[2] + waveCount[3];
        base = total ? atomicAdd(&pb.tailWords[0], total) : 0u;
    }
    __syncthreads();
    if (live) {
        uint32_t off = base;
        for (uint32_t w = 0; w < wave; ++w) off += waveCount[w];
        pb.tailList[off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = slot;
    }
}

bool launchTail(const ShadeVariant& v, const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t liveSlots, int numCUs, hipStream_t stream) {
    if (rp.numSlots == 0 || liveSlots == 0) return true;
    const TailKernel kernel = findTailKernel(tailVariant(v));
    if (!kernel) return false;
    hipLaunchKernelGGL(k_tail_collect, dim3(rp.numSlots / kShadeBlock), dim3(kShadeBlock), 0, stream, pb, rp);
    // one lane per listed slot; lanes take further slots from the list when theirs goes idle, so a grid smaller than the list is fine
    const uint32_t blocks = std::min<uint32_t>((liveSlots + kShadeBlock - 1) / kShadeBlock, (uint32_t)numCUs * 4u);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kShadeBlock), 0, stream, sc, pb, rp);
    return true;
}

} // namespace slrhip
