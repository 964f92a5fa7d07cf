// pt_shade_rgb_primary.hip — k_shade<RGB> with the fused start resuming the primary pass's stream (PRIMARY, RESUME)
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, true, false, false, false, true, true>();
template ShadeKernel shadeKernel<RGB, true, true, false, false, true, true>();
template ShadeKernel shadeKernel<RGB, false, false, false, false, true, true>();
template ShadeKernel shadeKernel<RGB, false, true, false, false, true, true>();

} // namespace slrhip
