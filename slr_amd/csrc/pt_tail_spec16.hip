// pt_tail_spec16.hip — k_tail<Spec16> (the table: pt_shade.hip)
#include "pt_tail_kernels.h"

namespace slrhip {

template TailKernel tailKernel<Spec16, true, false>();
template TailKernel tailKernel<Spec16, true, true>();
template TailKernel tailKernel<Spec16, false, false>();
template TailKernel tailKernel<Spec16, false, true>();

} // namespace slrhip
