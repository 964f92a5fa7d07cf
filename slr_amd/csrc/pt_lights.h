// pt_lights.h — what slrhip_set_materials and slrhip_set_texture_texels hand their device code (pt_lights.hip): the light list of the
// scene in place rebuilt over the kept index array, the closed form of the light distribution, the texel store.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/slrhip.h"
#include "device_types.h"

namespace slrhip {

const uint32_t kLightsBlock = 256;                         // triangles per workgroup of the count and the scatter
const uint32_t kLightsMaskLds = 1024;                      // mask words a workgroup stages in LDS (32 Ki materials); beyond: read from memory

inline uint32_t lightsBlocks(uint32_t numTriangles) { return (numTriangles + kLightsBlock - 1u) / kLightsBlock; }

// The distribution over n lights of importance 1 (RegularConstantDiscrete1D, Core/distributions.cpp:76-95, as prepareTriangles builds
// it): the Kahan sum of i ones is the integer i exactly, with compensation 0, while i <= 2^24, so PMF[i] = 1 / n and CDF[i] = i / n,
// one IEEE division each (k_light_tables).  n == 0: CDF = {0}.

struct LightsUpdate {
    uint32_t numTriangles, numMaterials, numLights, maskWords;
    const slrhip_triangle* triangles;                      // the kept index array (rebuild only)
    const uint32_t* emitMask;                              // one bit per material
    uint32_t* offsets;                                     // lightsBlocks(numTriangles) + 1 words: workgroup counts -> offsets; the total
    float4* shadeTris;                                     // ShadeTri as 6 x float4: word [1].w = light
    float4* lightTris;                                     // LightTri as 9 x float4: words [0].w = triangle, [1].w = material
    float *pmf, *cdf;                                      // numLights, numLights + 1 floats
    float *stagedPmf, *stagedCdf;                          // the same segments of the staged shade tables, or nullptr
    bool rebuild;                                          // the emitting set changed: count, scan, scatter
};

// The launches before the light records are filled (count, scan, scatter when u.rebuild) ...
uint32_t launchLightsRebuild(const LightsUpdate& u, hipStream_t stream);
// ... and the tables, always.  Each returns its launches.
uint32_t launchLightTables(const LightsUpdate& u, hipStream_t stream);

// `count` texels of three floats from src to dst, each float through binary16 first when `half`.
void launchTexelsStore(const float* src, float* dst, uint32_t count, bool half, hipStream_t stream);

} // namespace slrhip
