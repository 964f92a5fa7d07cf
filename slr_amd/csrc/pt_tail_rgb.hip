// pt_tail_rgb.hip — k_tail<RGB> (the table: pt_shade.hip)
#include "pt_tail_kernels.h"

namespace slrhip {

template TailKernel tailKernel<RGB, true, false>();
template TailKernel tailKernel<RGB, true, true>();
template TailKernel tailKernel<RGB, false, false>();
template TailKernel tailKernel<RGB, false, true>();

} // namespace slrhip
