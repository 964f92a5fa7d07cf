// pt_shade_tex_rgb_primary.hip — the all-lobes k_shade<RGB> of textured scenes with the fused start, resuming (PRIMARY, RESUME); one per file
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, false, true, true, true, true, true>();

} // namespace slrhip
