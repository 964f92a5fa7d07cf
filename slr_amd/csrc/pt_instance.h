// pt_instance.h — a placement of an instanced mesh: the checks on its two matrices and the world box the top-level tree holds for it.
// ONE definition for the host (buildInstancedQBVH: bvh.cpp; slrhip_instance_world_box: host_util.cpp) and the kernels of
// slrhip_set_instance_transforms (pt_instances.hip).  float32 operations in the order written (both sides are built with
// -ffp-contract=off) and no library call beyond min / max / abs, so host and device agree bit for bit.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>

#include "pt_refit.h"            // kRefitGroupNodes, kMaxTreeLevels: the refit's child rule, shared with slrhip_set_vertices
#endif

#include <cmath>
#include <cstdint>

#include "pt_luminance.h"          // SLR_HOST_DEV

namespace slrhip {

// Matrix4x4 x Point3D (Matrix4x4.h:75-81), column-major m
SLR_HOST_DEV void instMulPoint(const float* m, const float* p, float* o) {
    float x = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12] * 1.0f;
    float y = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13] * 1.0f;
    float z = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14] * 1.0f;
    float w = m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15] * 1.0f;
    if (w != 1.0f) { float r = 1.0f / w; x *= r; y *= r; z *= r; }
    o[0] = x; o[1] = y; o[2] = z;
}

// What the traversal needs of a transform: 0 = fine, 1 = the bottom row is not 0 0 0 1, 2 = an entry is not finite.
SLR_HOST_DEV int instMatrixRefusal(const float* m) {
    if (m[3] != 0.0f || m[7] != 0.0f || m[11] != 0.0f || m[15] != 1.0f) return 1;
    for (int i = 0; i < 16; ++i)
        if (!(fabsf(m[i]) <= 3.402823466e+38f)) return 2;
    return 0;
}

// bounds() of a TransformedSurfaceObject = StaticTransform x BoundingBox3D (Transform.h:54-65): the box of the eight transformed
// corners of the mesh's box; a hair of slack because the local-space traversal rounds differently from a world-space box test.
SLR_HOST_DEV void instanceWorldBox(const float* meshLo, const float* meshHi, const float* localToWorld, float* lo, float* hi) {
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (int c = 0; c < 8; ++c) {
        const float p[3] = {(c & 4) ? meshHi[0] : meshLo[0], (c & 2) ? meshHi[1] : meshLo[1], (c & 1) ? meshHi[2] : meshLo[2]};
        float q[3];
        instMulPoint(localToWorld, p, q);
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], q[a]); hi[a] = fmaxf(hi[a], q[a]); }
    }
    for (int a = 0; a < 3; ++a) {
        const float pad = 1e-5f * fmaxf(1.0f, fmaxf(fabsf(lo[a]), fabsf(hi[a])));
        lo[a] -= pad; hi[a] += pad;
    }
}

#ifdef __HIP__
// slrhip_set_instance_transforms' device work (pt_instances.hip): place the records, then refit the top-level tree's child boxes
// level by level from the deepest level to the root, all on `stream`.  The range has passed instanceUpdateRefusal (render_plan.h).
static const uint32_t kMaxTopLevels = kMaxTreeLevels;
struct InstanceUpdate {
    const float4* src;                                     // the caller's records, 8 x float4 each: local_to_world, world_to_local
    uint32_t first, count;                                 // instances [first, first + count)
    uint32_t numInstances, numMeshes, topNodes, numLevels;
    float4* instances;                                     // DevInstance as 9 x float4
    const float4* meshBoxes;                               // 2 x float4 per mesh: lo, hi
    float4* instBoxes;                                     // 2 x float4 per instance: lo, hi
    const float4* leafBoxes;                               // 2 x float4 per LeafTri record, or nullptr: the loose-triangle packets keep their boxes
    uint32_t numLeafBoxes;                                 //   (slrhip_set_vertices on a scene with instances gives them: the packets' triangles moved)
    float4* nodes;                                         // the scene's QNodes as 8 x float4; the first topNodes are the top level
    uint32_t* status;                                      // SLRHIP_INSTANCE_* bits
    uint32_t levelFirst[kMaxTopLevels + 1];                // first node of each top-level level; [numLevels] = topNodes
};
void launchInstanceUpdate(const InstanceUpdate& u, hipStream_t stream);
// The refit alone (src, first, count, instances, meshBoxes and status are not read): what slrhip_rebuild_top_level runs after it has
// seated the leaves (pt_toplevel.hip), and slrhip_set_vertices after it has refitted the meshes (pt_geometry.hip; with leafBoxes).
// Returns the number of launches.
uint32_t launchTopRefit(const InstanceUpdate& u, hipStream_t stream);
#endif

} // namespace slrhip
