// pt_shade_spec16.hip — k_shade<Spec16> (the table: pt_shade.hip)
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<Spec16, true, false>();
template ShadeKernel shadeKernel<Spec16, true, true>();
template ShadeKernel shadeKernel<Spec16, false, false>();
template ShadeKernel shadeKernel<Spec16, false, true>();

} // namespace slrhip
