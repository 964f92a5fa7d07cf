// pt_shade_multi_rgb_primary_seeded.hip — one k_shade instantiation with the fused start (PRIMARY, see pt_shade_kernels.h), seeding its own stream; one per file
#include "pt_shade_kernels.h"

namespace slrhip {

void launchShadeMultiRGBPrimarySeeded(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, hipStream_t stream) {
    const dim3 grid(rp.numSlots / kShadeBlock), block(kShadeBlock);
    hipLaunchKernelGGL((k_shade<RGB, false, true, true, false, true>), grid, block, 0, stream, sc, pb, rp, parity);
}

} // namespace slrhip
