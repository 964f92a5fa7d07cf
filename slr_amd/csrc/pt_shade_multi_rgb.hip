// pt_shade_multi_rgb.hip — the all-lobes k_shade<RGB> of MultiBSDF scenes; one per file: each takes a minute or more to compile
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, false, true, true>();

} // namespace slrhip
