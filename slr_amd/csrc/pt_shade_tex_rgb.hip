// pt_shade_tex_rgb.hip — the all-lobes k_shade<RGB> of textured scenes; one per file: each takes a minute or more to compile
#include "pt_shade_kernels.h"

namespace slrhip {

template ShadeKernel shadeKernel<RGB, false, true, true, true>();

} // namespace slrhip
