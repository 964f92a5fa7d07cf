// pt_shade_rgb.hip — k_shade<RGB> without the fused start (the table: pt_shade.hip)
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, true, false>();
template ShadeKernel shadeKernel<RGB, true, true>();
template ShadeKernel shadeKernel<RGB, false, false>();
template ShadeKernel shadeKernel<RGB, false, true>();

} // namespace slrhip
