// pt_shade_tex_spec.hip — the all-lobes k_shade<Spec16> of textured scenes; one per file
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<Spec16, false, true, true, true>();

} // namespace slrhip
