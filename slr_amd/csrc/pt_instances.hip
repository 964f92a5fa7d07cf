// pt_instances.hip — device code of slrhip_set_instance_transforms: new placements for instances of the uploaded scene, and the
// top-level tree's child boxes refitted to them where they are.  gfx950, wave64.  Launches in stream order:
//
//   k_instance_place  one lane per updated instance.  Eight 16-byte loads of the caller's record; the checks of buildInstancedQBVH
//                     (pt_instance.h, instMatrixRefusal).  A record that fails them leaves its instance as it was and sets
//                     SLRHIP_INSTANCE_BAD_TRANSFORM with one atomic OR on a word of its own.  A good record goes into DevInstance
//                     (eight 16-byte stores; the ninth float4 — root, range, mesh — stays) and its world box (pt_instance.h,
//                     instanceWorldBox: the host's arithmetic, same bits) into the instance boxes, two 16-byte stores.
//   k_top_refit       the child boxes of the top-level nodes, bottom-up (the child rule is pt_refit.h's, shared with
//                     slrhip_set_vertices).  One lane per (node, child): an instance child takes its
//                     instance's world box, an inner child the exact min / max union of the valid child boxes of the node it names
//                     (six 16-byte loads of that node's planes + one of its references, a horizontal min / max over the valid
//                     children), a triangle packet keeps its bytes (or, for slrhip_set_vertices, takes the union of its triangles' boxes:
//                     InstanceUpdate::leafBoxes) and an empty slot keeps its bytes.  Six 4-byte stores per lane; the four lanes
//                     of a node fill one 16-byte group of each plane.  The named node is on the NEXT level, so a level needs the
//                     levels below it complete: a level wider than kRefitGroupNodes is a launch of its own, and a run of
//                     consecutive levels that each fit one workgroup is ONE launch of one workgroup with a barrier between levels
//                     (stores and loads of one workgroup go through the same vector L1; __syncthreads orders them).
//
// No atomics but the status bit, no parent pointers, no flags between workgroups: the order comes from the launches.  Only the
// first topNodes nodes are written; a mesh's tree lives in its local space and does not change when a placement moves.
// The refit's launches are a function of their own (launchTopRefit): slrhip_rebuild_top_level runs them after it has seated the
// leaves (pt_toplevel.hip).
#include <hip/hip_runtime.h>

#include "../../include/slrhip.h"
#include "device_types.h"
#include "pt_instance.h"

namespace slrhip {

namespace {

__global__ __launch_bounds__(256) void k_instance_place(InstanceUpdate u) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= u.count) return;                                                 // count records at src; first + count <= numInstances
    const uint32_t k = u.first + t;
    float m[32];                                                              // local_to_world, world_to_local
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const float4 v = u.src[(size_t)t * 8u + q];
        m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w;
    }
    if (instMatrixRefusal(m) != 0 || instMatrixRefusal(m + 16) != 0) {
        atomicOr(u.status, (uint32_t)SLRHIP_INSTANCE_BAD_TRANSFORM);
        return;
    }
    float4* rec = u.instances + (size_t)k * 9u;
    const uint4 tail = *reinterpret_cast<const uint4*>(rec + 8);              // rootNode, firstTriangle, numTriangles, mesh
#pragma unroll
    for (int q = 0; q < 8; ++q) rec[q] = make_float4(m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]);
    const uint32_t mesh = tail.w < u.numMeshes ? tail.w : 0u;                 // (always in range: written by the upload)
    const float4 mlo = u.meshBoxes[2u * mesh], mhi = u.meshBoxes[2u * mesh + 1u];
    const float meshLo[3] = {mlo.x, mlo.y, mlo.z}, meshHi[3] = {mhi.x, mhi.y, mhi.z};
    float lo[3], hi[3];
    instanceWorldBox(meshLo, meshHi, m, lo, hi);
    u.instBoxes[2u * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    u.instBoxes[2u * (size_t)k + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
}

// One level of more than kRefitGroupNodes nodes: nodes [first, first + count), four lanes each.
__global__ __launch_bounds__(kRefitBlock) void k_top_refit(float4* nodes, const float4* instBoxes, const float4* leafBoxes, uint32_t first, uint32_t count,
                                                           uint32_t topNodes, uint32_t numInstances, uint32_t numLeafBoxes) {
    const uint32_t t = blockIdx.x * kRefitBlock + threadIdx.x;
    if (t >= 4u * count) return;
    refitChild(nodes, instBoxes, leafBoxes, first + (t >> 2), t & 3u, topNodes, numInstances, numLeafBoxes);
}

// Levels levelHi, levelHi - 1, .. levelLo, each of at most kRefitGroupNodes nodes: one workgroup, a barrier between levels.
__global__ __launch_bounds__(kRefitBlock) void k_top_refit_levels(InstanceUpdate u, uint32_t levelHi, uint32_t levelLo) {
    const uint32_t t = threadIdx.x;
    for (uint32_t level = levelHi + 1u; level-- > levelLo;) {                 // uniform over the workgroup: every lane reaches every barrier
        const uint32_t first = u.levelFirst[level], count = u.levelFirst[level + 1u] - first;
        if (t < 4u * count) refitChild(u.nodes, u.instBoxes, u.leafBoxes, first + (t >> 2), t & 3u, u.topNodes, u.numInstances, u.numLeafBoxes);
        __syncthreads();
    }
}

} // namespace

void launchInstanceUpdate(const InstanceUpdate& u, hipStream_t stream) {
    hipLaunchKernelGGL(k_instance_place, dim3((u.count + 255u) / 256u), dim3(256), 0, stream, u);
    launchTopRefit(u, stream);
}

uint32_t launchTopRefit(const InstanceUpdate& u, hipStream_t stream) {
    uint32_t launches = 0;
    // from the deepest level to the root; consecutive levels that fit one workgroup share a launch
    for (uint32_t level = u.numLevels; level-- > 0u;) {
        ++launches;
        const uint32_t first = u.levelFirst[level], count = u.levelFirst[level + 1u] - first;
        if (count > kRefitGroupNodes) {
            hipLaunchKernelGGL(k_top_refit, dim3((4u * count + kRefitBlock - 1u) / kRefitBlock), dim3(kRefitBlock), 0, stream, u.nodes, u.instBoxes, u.leafBoxes,
                               first, count, u.topNodes, u.numInstances, u.numLeafBoxes);
            continue;
        }
        uint32_t lo = level;
        while (lo > 0u && u.levelFirst[lo] - u.levelFirst[lo - 1u] <= kRefitGroupNodes) --lo;
        hipLaunchKernelGGL(k_top_refit_levels, dim3(1), dim3(kRefitBlock), 0, stream, u, level, lo);
        level = lo;
    }
    return launches;
}

} // namespace slrhip
