// pt_shade_multi_rgb_primary_seeded.hip — the all-lobes k_shade<RGB> of MultiBSDF scenes with the fused start, seeding its stream (PRIMARY); one per file
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, false, true, true, false, true>();

} // namespace slrhip
