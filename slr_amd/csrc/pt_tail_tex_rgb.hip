// pt_tail_tex_rgb.hip — the all-lobes k_tail<RGB> of textured scenes; one per file: each takes minutes to compile
#include "pt_tail_kernels.h"

namespace slrhip {

template TailKernel tailKernel<RGB, false, true, true, true>();

} // namespace slrhip
