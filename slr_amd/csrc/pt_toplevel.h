// pt_toplevel.h — re-seating the top-level tree of an instanced scene (slrhip_rebuild_top_level): the sort key of a top-level
// primitive, the limit between the two device paths, and the launch description.  ONE definition of the key for the host export
// (slrhip_top_level_key), the host twin (slrhip_debug_top_level_reseat: top_level.cpp) and the kernels (pt_toplevel.hip).  float32
// operations in the order written, each rounded on its own (both sides are built with -ffp-contract=off), IEEE division and no
// library call beyond floor / min, so host and device agree bit for bit.
//
// The tree keeps its SHAPE.  Its leaf slots, taken depth-first from node 0 (child slots 0 .. 3 in order, an inner child's whole
// subtree before the next slot), receive the primitives — instance leaves and loose-triangle packets — in the order of the Morton
// code of their box centres; the refit of pt_refit.h then gives every inner child its box.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "device_types.h"
#include "pt_luminance.h"          // SLR_HOST_DEV

namespace slrhip {

// At most this many primitives: one launch of ONE workgroup sorts (key, index) pairs in LDS (12 bytes a pair: 48 KiB).  More: keys,
// a device radix sort and the seat are launches of their own.
static const uint32_t kTopSeatGroup = 4096;
static const uint32_t kTopSeatBlock = 1024;                // lanes of that workgroup
static const uint32_t kTopKeyBits = 21;                    // per axis: a 63-bit key

// One axis of the key: where the box centre lies in the scene box, in 2^21 steps.  A NaN gives 0.
SLR_HOST_DEV uint32_t topLevelAxis(float lo, float hi, float sceneLo, float sceneHi) {
    const float c = (lo + hi) * 0.5f;
    const float e = sceneHi - sceneLo;
    const float x = e > 0.0f ? (c - sceneLo) / e : 0.0f;
    return x >= 0.0f ? (uint32_t)fminf(floorf(x * 2097152.0f), 2097151.0f) : 0u;
}

// bit i of v -> bit 3 i
SLR_HOST_DEV uint64_t topLevelSpread(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x001F00000000FFFFull;
    x = (x | (x << 16)) & 0x001F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}

// The key of a box [lo, hi] in the scene box: bit 3 i + 2 is bit i of q.x, bit 3 i + 1 bit i of q.y, bit 3 i bit i of q.z.
SLR_HOST_DEV uint64_t topLevelKey(const float* lo, const float* hi, const float* sceneLo, const float* sceneHi) {
    const uint32_t qx = topLevelAxis(lo[0], hi[0], sceneLo[0], sceneHi[0]);
    const uint32_t qy = topLevelAxis(lo[1], hi[1], sceneLo[1], sceneHi[1]);
    const uint32_t qz = topLevelAxis(lo[2], hi[2], sceneLo[2], sceneHi[2]);
    return (topLevelSpread(qx) << 2) | (topLevelSpread(qy) << 1) | topLevelSpread(qz);
}

#ifdef __HIP__
// slrhip_rebuild_top_level's device work (pt_toplevel.hip), all on `stream`: keys, order and seat (one launch, or keys + a device
// radix sort + seat), then the refit of pt_instances.hip from the deepest level to the root.  The tables are the first call's
// (slrhip_toplevel.hip): every slot names a child of one of the first topNodes nodes, every instance reference an instance.
struct TopSeat {
    float4* nodes;                                         // the scene's QNodes as 8 x float4; the first topNodes are the top level
    const float4* instBoxes;                               // 2 x float4 per instance: lo, hi
    const float4* packetBoxes;                             // 2 x float4 per packet, in canonical order
    const uint32_t* refs;                                  // the primitives' child words, ascending: instances 0 .. n - 1, then the packets
    const uint32_t* slots;                                 // node * 4 + child of the leaf slots, depth-first
    uint64_t* keys;                                        // by primitive
    uint64_t* sortedKeys;                                  // the large path's sort output (unused by the small one)
    uint32_t* identity;                                    // 0 .. count - 1 (the large path's sort input)
    uint32_t* order;                                       // slot i receives primitive order[i]
    void* sortTemp;                                        // the device radix sort's temporary storage
    size_t sortTempBytes;
    uint32_t count, numInstances, topNodes;
};
// bytes of temporary storage the large path's sort needs for `count` primitives
size_t topSeatSortBytes(uint32_t count);
// returns the launches made before the refit (the radix sort counts as one), 0 and *err on a failure of the sort's enqueue
uint32_t launchTopSeat(const TopSeat& s, hipStream_t stream, hipError_t* err);
#endif

// ---- the host twin (top_level.cpp): the plan the first call builds and the whole operation on a host copy of the nodes ----
// The leaf slots (node * 4 + child) of the first topNodes nodes depth-first, and the child words of those slots ascending.  Returns
// the number of primitives and in *numInstances how many of them are instances, or 0 if the nodes are no top level: an inner child
// not inside (its node, topNodes), more than `capacity` leaves (4 x topNodes always suffice), or references that do not begin with
// the instances 0 .. *numInstances - 1 in order, each once.
uint32_t topLevelPlan(const QNode* nodes, uint32_t topNodes, uint32_t* slots, uint32_t* refs, uint32_t capacity, uint32_t* numInstances);
// Keys, order, seat and refit on `nodes` in place; instBoxes: lo[3], 0, hi[3], 0 per instance.  keys / order: room for every
// primitive, or null.  Returns the number of primitives, 0 as topLevelPlan.
uint32_t topLevelReseat(QNode* nodes, uint32_t topNodes, const float* instBoxes, uint32_t numInstances, uint64_t* keys, uint32_t* order);
// 1 + (sum of the surface areas of all inner-child boxes) / (area of the union of the root's valid children), in double.
double topLevelCost(const QNode* nodes, uint32_t topNodes);

} // namespace slrhip
