// pt_shade_rgb_primary_seeded.hip — k_shade<RGB> with the fused start seeding its own stream (PRIMARY): windows without a stream plane
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, true, false, false, false, true>();
template ShadeKernel shadeKernel<RGB, true, true, false, false, true>();
template ShadeKernel shadeKernel<RGB, false, false, false, false, true>();
template ShadeKernel shadeKernel<RGB, false, true, false, false, true>();

} // namespace slrhip
