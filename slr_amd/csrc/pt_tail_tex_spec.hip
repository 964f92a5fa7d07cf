// pt_tail_tex_spec.hip — the all-lobes k_tail<Spec16> of textured scenes; one per file
#include "pt_tail_kernels.h"

namespace slrhip {

template TailKernel tailKernel<Spec16, false, true, true, true>();

} // namespace slrhip
