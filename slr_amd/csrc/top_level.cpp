// top_level.cpp — the host side of slrhip_rebuild_top_level (pt_toplevel.h): the plan its first call builds from a read-back of the
// top-level nodes, the whole operation on a host copy of a node array (the twin the tests hold the device against) and the cost
// read-out.  No GPU is touched here.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/slrhip_debug.h"
#include "pt_toplevel.h"

namespace slrhip {

namespace {

inline bool isInner(uint32_t ref) { return ref != kInvalidChild && !(ref & kLeafFlag); }
inline bool isLeaf(uint32_t ref) { return ref != kInvalidChild && (ref & kLeafFlag); }
inline bool isInstance(uint32_t ref) { return isLeaf(ref) && ((ref >> kLeafCountShift) & 0xFu) == 0u; }

struct Box6 { float lo[3], hi[3]; };

inline Box6 childBox(const QNode& n, uint32_t c) { return Box6{{n.minx[c], n.miny[c], n.minz[c]}, {n.maxx[c], n.maxy[c], n.maxz[c]}}; }
inline void setChildBox(QNode& n, uint32_t c, const Box6& b) {
    n.minx[c] = b.lo[0]; n.miny[c] = b.lo[1]; n.minz[c] = b.lo[2];
    n.maxx[c] = b.hi[0]; n.maxy[c] = b.hi[1]; n.maxz[c] = b.hi[2];
}
// the exact min / max union of a node's valid child boxes (pt_refit.h, unionMin / unionMax)
inline Box6 unionOfChildren(const QNode& n) {
    Box6 u{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
    for (uint32_t c = 0; c < 4; ++c) {
        if (n.child[c] == kInvalidChild) continue;
        const Box6 b = childBox(n, c);
        for (int a = 0; a < 3; ++a) { u.lo[a] = fminf(u.lo[a], b.lo[a]); u.hi[a] = fmaxf(u.hi[a], b.hi[a]); }
    }
    return u;
}

} // namespace

uint32_t topLevelPlan(const QNode* nodes, uint32_t topNodes, uint32_t* slots, uint32_t* refs, uint32_t capacity, uint32_t* numInstances) {
    *numInstances = 0;
    if (topNodes == 0 || topNodes > (kLeafFlag >> 2)) return 0;
    uint32_t count = 0;
    std::vector<uint32_t> stack{0u};                                          // node * 4 + the next child slot to look at
    while (!stack.empty()) {
        const uint32_t at = stack.back(), node = at >> 2, c = at & 3u;
        if (c == 3u) stack.pop_back(); else stack.back() = at + 1u;
        const uint32_t ref = nodes[node].child[c];
        if (isLeaf(ref)) {
            if (count == capacity) return 0;
            slots[count] = at; refs[count] = ref; ++count;
        }
        else if (isInner(ref)) {
            if (ref <= node || ref >= topNodes || stack.size() > 64u) return 0;
            stack.push_back(ref << 2);
        }
    }
    if (count == 0) return 0;
    std::sort(refs, refs + count);
    uint32_t n = 0;
    while (n < count && isInstance(refs[n])) ++n;                             // count 0 sorts below every packet
    for (uint32_t k = 0; k < n; ++k)
        if ((refs[k] & kLeafIndexMask) != k) return 0;
    *numInstances = n;
    return count;
}

uint32_t topLevelReseat(QNode* nodes, uint32_t topNodes, const float* instBoxes, uint32_t numInstances, uint64_t* keys, uint32_t* order) {
    if (topNodes == 0) return 0;
    std::vector<uint32_t> slots(4u * (size_t)topNodes), refs(4u * (size_t)topNodes);
    uint32_t planInstances = 0;
    const uint32_t count = topLevelPlan(nodes, topNodes, slots.data(), refs.data(), (uint32_t)slots.size(), &planInstances);
    if (count == 0 || planInstances != numInstances) return 0;
    // the primitives' boxes in canonical order: an instance's world box; a packet's is the box of the slot that holds it
    std::vector<Box6> box(count);
    for (uint32_t k = 0; k < numInstances; ++k) {
        const float* b = instBoxes + 8u * (size_t)k;
        box[k] = Box6{{b[0], b[1], b[2]}, {b[4], b[5], b[6]}};
    }
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t ref = nodes[slots[i] >> 2].child[slots[i] & 3u];
        if (isInstance(ref)) continue;
        const uint32_t p = (uint32_t)(std::lower_bound(refs.begin(), refs.begin() + count, ref) - refs.begin());
        box[p] = childBox(nodes[slots[i] >> 2], slots[i] & 3u);
    }
    Box6 scene{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
    for (const Box6& b : box)
        for (int a = 0; a < 3; ++a) { scene.lo[a] = fminf(scene.lo[a], b.lo[a]); scene.hi[a] = fmaxf(scene.hi[a], b.hi[a]); }
    std::vector<uint64_t> key(count);
    for (uint32_t p = 0; p < count; ++p) key[p] = topLevelKey(box[p].lo, box[p].hi, scene.lo, scene.hi);
    std::vector<uint32_t> ord(count);
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    for (uint32_t i = 0; i < count; ++i) {                                    // the seat
        QNode& n = nodes[slots[i] >> 2];
        n.child[slots[i] & 3u] = refs[ord[i]];
        setChildBox(n, slots[i] & 3u, box[ord[i]]);
    }
    for (uint32_t node = topNodes; node-- > 0u;)                              // the refit: an inner child names a later node
        for (uint32_t c = 0; c < 4; ++c)
            if (isInner(nodes[node].child[c])) setChildBox(nodes[node], c, unionOfChildren(nodes[nodes[node].child[c]]));
    if (keys) std::copy(key.begin(), key.end(), keys);
    if (order) std::copy(ord.begin(), ord.end(), order);
    return count;
}

double topLevelCost(const QNode* nodes, uint32_t topNodes) {
    const auto area = [](const Box6& b) {
        const double dx = std::max((double)b.hi[0] - (double)b.lo[0], 0.0), dy = std::max((double)b.hi[1] - (double)b.lo[1], 0.0),
                     dz = std::max((double)b.hi[2] - (double)b.lo[2], 0.0);
        return 2.0 * ((dx * dy + dy * dz) + dz * dx);
    };
    if (topNodes == 0) return 1.0;
    const double rootArea = area(unionOfChildren(nodes[0]));
    if (!(rootArea > 0.0)) return 1.0;
    double sum = 0.0;
    for (uint32_t node = 0; node < topNodes; ++node)
        for (uint32_t c = 0; c < 4; ++c)
            if (isInner(nodes[node].child[c])) sum += area(childBox(nodes[node], c));
    return 1.0 + sum / rootArea;
}

} // namespace slrhip

extern "C" {

int slrhip_top_level_key(const float* lo, const float* hi, const float* sceneLo, const float* sceneHi, uint64_t* key) {
    if (!lo || !hi || !sceneLo || !sceneHi || !key) return SLRHIP_ERR_INVALID_ARGUMENT;
    *key = slrhip::topLevelKey(lo, hi, sceneLo, sceneHi);
    return SLRHIP_OK;
}

int slrhip_debug_top_level_plan(const void* nodes, uint32_t topNodes, uint32_t* slots, uint32_t* refs, uint32_t capacity, uint32_t* count) {
    if (!nodes || !slots || !refs || !count) return SLRHIP_ERR_INVALID_ARGUMENT;
    uint32_t numInstances = 0;
    *count = slrhip::topLevelPlan(static_cast<const slrhip::QNode*>(nodes), topNodes, slots, refs, capacity, &numInstances);
    return *count ? SLRHIP_OK : SLRHIP_ERR_INVALID_ARGUMENT;
}

int slrhip_debug_top_level_reseat(void* nodes, uint32_t topNodes, const float* instanceBoxes, uint32_t numInstances, uint64_t* keysOut, uint32_t* orderOut) {
    if (!nodes || !instanceBoxes) return SLRHIP_ERR_INVALID_ARGUMENT;
    return slrhip::topLevelReseat(static_cast<slrhip::QNode*>(nodes), topNodes, instanceBoxes, numInstances, keysOut, orderOut) ? SLRHIP_OK
                                                                                                                                  : SLRHIP_ERR_INVALID_ARGUMENT;
}

int slrhip_debug_top_level_cost(const void* nodes, uint32_t topNodes, double* cost) {
    if (!nodes || !cost || topNodes == 0) return SLRHIP_ERR_INVALID_ARGUMENT;
    *cost = slrhip::topLevelCost(static_cast<const slrhip::QNode*>(nodes), topNodes);
    return SLRHIP_OK;
}

} // extern "C"
