// pt_refit.h — the child rule of the bottom-up refits: what one child box of a 4-wide node becomes when what lies below it has
// moved.  ONE definition for slrhip_set_instance_transforms (pt_instances.hip: the top-level tree over instances) and
// slrhip_set_vertices (pt_geometry.hip: the whole tree of a flat scene).  One lane per (node, child):
//   an inner child      the exact min / max union of the valid child boxes of the node it names (six 16-byte loads of that node's
//                       planes + one of its references, a horizontal min / max over the valid children)
//   an instance child   its instance's world box (instBoxes; without them it keeps its bytes)
//   a triangle packet   the exact min / max union of its `count` triangle boxes (leafBoxes: two float4 per LeafTri record; without
//                       them it keeps its bytes — a placement does not move loose triangles)
//   an empty slot       keeps its bytes
// Six 4-byte stores per lane; the four lanes of a node fill one 16-byte group of each plane.  The named node is on the NEXT level, so
// a level needs the levels below it complete: the callers order levels by launches, or by a barrier inside one workgroup.  No
// padding is added anywhere: min and max are exact, so the unions do not depend on the order they are taken in.
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace slrhip {

static const uint32_t kMaxTreeLevels = 21;                 // 3 x depth + 1 <= 64 (checkTreeLimits)
static const uint32_t kRefitGroupNodes = 64;               // a level of at most this many nodes fits one workgroup of a refit kernel (4 lanes per node)
static const uint32_t kRefitBlock = 4u * kRefitGroupNodes; // 256 lanes: four per node

__device__ __forceinline__ float pick(const float4& v, uint32_t c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }
__device__ __forceinline__ uint32_t pick(const uint4& v, uint32_t c) { return c == 0 ? v.x : c == 1 ? v.y : c == 2 ? v.z : v.w; }

// min / max of a plane over the children whose reference is valid; an empty slot's bytes take no part
__device__ __forceinline__ float unionMin(const float4& v, const uint4& ref) {
    float r = INFINITY;
    if (ref.x != kInvalidChild) r = fminf(r, v.x);
    if (ref.y != kInvalidChild) r = fminf(r, v.y);
    if (ref.z != kInvalidChild) r = fminf(r, v.z);
    if (ref.w != kInvalidChild) r = fminf(r, v.w);
    return r;
}
__device__ __forceinline__ float unionMax(const float4& v, const uint4& ref) {
    float r = -INFINITY;
    if (ref.x != kInvalidChild) r = fmaxf(r, v.x);
    if (ref.y != kInvalidChild) r = fmaxf(r, v.y);
    if (ref.z != kInvalidChild) r = fmaxf(r, v.z);
    if (ref.w != kInvalidChild) r = fmaxf(r, v.w);
    return r;
}

// Child c of node `node`.  nodes: not restrict, not const — a level reads what the level below it stored.  Inner references below
// numNodes, instance indices below numInstances, packets inside numLeafBoxes: anything else keeps its bytes (never: the upload wrote
// the references).
__device__ __forceinline__ void refitChild(float4* nodes, const float4* instBoxes, const float4* leafBoxes, uint32_t node, uint32_t c, uint32_t numNodes,
                                           uint32_t numInstances, uint32_t numLeafBoxes) {
    float4* self = nodes + (size_t)node * 8u;
    const uint32_t ref = pick(*reinterpret_cast<const uint4*>(self + 6), c);
    if (ref == kInvalidChild) return;
    float lo[3], hi[3];
    if (ref & kLeafFlag) {
        const uint32_t count = (ref >> kLeafCountShift) & 0xFu, k = ref & kLeafIndexMask;
        if (count != 0u) {
            if (!leafBoxes || count > kMaxLeafTris || (uint64_t)k + count > numLeafBoxes) return;      // a triangle packet keeps its box
            float4 a = leafBoxes[2u * (size_t)k], b = leafBoxes[2u * (size_t)k + 1u];
            for (uint32_t j = 1; j < count; ++j) {
                const float4 a2 = leafBoxes[2u * (size_t)(k + j)], b2 = leafBoxes[2u * (size_t)(k + j) + 1u];
                a.x = fminf(a.x, a2.x); a.y = fminf(a.y, a2.y); a.z = fminf(a.z, a2.z);
                b.x = fmaxf(b.x, b2.x); b.y = fmaxf(b.y, b2.y); b.z = fmaxf(b.z, b2.z);
            }
            lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
        }
        else {
            if (!instBoxes || k >= numInstances) return;
            const float4 a = instBoxes[2u * (size_t)k], b = instBoxes[2u * (size_t)k + 1u];
            lo[0] = a.x; lo[1] = a.y; lo[2] = a.z; hi[0] = b.x; hi[1] = b.y; hi[2] = b.z;
        }
    }
    else {
        if (ref >= numNodes) return;
        const float4* kid = nodes + (size_t)ref * 8u;
        const float4 p0 = kid[0], p1 = kid[1], p2 = kid[2], p3 = kid[3], p4 = kid[4], p5 = kid[5];
        const uint4 refs = *reinterpret_cast<const uint4*>(kid + 6);
        lo[0] = unionMin(p0, refs); lo[1] = unionMin(p1, refs); lo[2] = unionMin(p2, refs);
        hi[0] = unionMax(p3, refs); hi[1] = unionMax(p4, refs); hi[2] = unionMax(p5, refs);
    }
    float* planes = reinterpret_cast<float*>(self);                            // minx[4] miny[4] minz[4] maxx[4] maxy[4] maxz[4]
    planes[c] = lo[0]; planes[4u + c] = lo[1]; planes[8u + c] = lo[2];
    planes[12u + c] = hi[0]; planes[16u + c] = hi[1]; planes[20u + c] = hi[2];
}

} // namespace slrhip
