// pt_shade_rgb_primary.hip — the k_shade<RGB> instantiations with the fused start (PRIMARY, see pt_shade_kernels.h): windows with a primary pass
#include "pt_shade_kernels.h"

namespace slrhip {

void launchShadeRGBPrimarySeeded(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, bool lds, bool glossy, hipStream_t stream);      // pt_shade_rgb_primary_seeded.hip

void launchShadeRGBPrimary(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, bool lds, bool glossy, hipStream_t stream) {
    if (!pb.primaryRng) { launchShadeRGBPrimarySeeded(sc, pb, rp, parity, lds, glossy, stream); return; }      // no stream plane in this window (render_plan.h, planPrimary)
    const dim3 grid(rp.numSlots / kShadeBlock), block(kShadeBlock);
    if (lds && !glossy) hipLaunchKernelGGL((k_shade<RGB, true, false, false, false, true, true>), grid, block, 0, stream, sc, pb, rp, parity);
    else if (lds) hipLaunchKernelGGL((k_shade<RGB, true, true, false, false, true, true>), grid, block, 0, stream, sc, pb, rp, parity);
    else if (!glossy) hipLaunchKernelGGL((k_shade<RGB, false, false, false, false, true, true>), grid, block, 0, stream, sc, pb, rp, parity);
    else hipLaunchKernelGGL((k_shade<RGB, false, true, false, false, true, true>), grid, block, 0, stream, sc, pb, rp, parity);
}

} // namespace slrhip
