// pt_shade_variants.h — how the table of built k_shade / k_tail kernels (pt_shade.hip) names an instantiation without seeing the
// kernel templates: shadeKernel<...>() / tailKernel<...>() return the kernel's address.  They are defined next to the kernels
// (pt_shade_kernels.h, pt_tail_kernels.h) and explicitly instantiated in the translation unit that builds the kernel
// (pt_shade_*.hip, pt_tail_*.hip), so a row of the table whose kernel no file builds is a link error.
#pragma once
#include "pt_kernels.h"

namespace slrhip {

struct RGB;
struct Spec16;

using ShadeKernel = void (*)(DevScene, PathBuffers, RenderParams, uint32_t parity);
using TailKernel = void (*)(DevScene, PathBuffers, RenderParams);

template <class S, bool LDS_TABLES, bool MF, bool MULTI = false, bool TEX = false, bool PRIMARY = false, bool RESUME = false>
ShadeKernel shadeKernel();
template <class S, bool LDS_TABLES, bool MF, bool MULTI = false, bool TEX = false>
TailKernel tailKernel();

// The row of the table for `v`, nullptr if no such kernel is built (findTailKernel: for tailVariant(v), render_plan.h)
ShadeKernel findShadeKernel(const ShadeVariant& v);
TailKernel findTailKernel(const ShadeVariant& v);

} // namespace slrhip
