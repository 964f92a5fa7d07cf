// pt_shade_multi_spec.hip — the all-lobes k_shade<Spec16> of MultiBSDF scenes; one per file
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<Spec16, false, true, true>();

} // namespace slrhip
