// pt_shade_tex_rgb_primary.hip — one k_shade instantiation with the fused start (PRIMARY, see pt_shade_kernels.h); one per file
#include "pt_shade_kernels.h"

namespace slrhip {

void launchShadeTexRGBPrimarySeeded(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, hipStream_t stream);      // pt_shade_tex_rgb_primary_seeded.hip

void launchShadeTexRGBPrimary(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, hipStream_t stream) {
    if (!pb.primaryRng) { launchShadeTexRGBPrimarySeeded(sc, pb, rp, parity, stream); return; }      // no stream plane in this window (render_plan.h, planPrimary)
    const dim3 grid(rp.numSlots / kShadeBlock), block(kShadeBlock);
    hipLaunchKernelGGL((k_shade<RGB, false, true, true, true, true, true>), grid, block, 0, stream, sc, pb, rp, parity);
}

} // namespace slrhip
