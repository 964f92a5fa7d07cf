// pt_trace_ws.h — wave-specialised BVH traversal: the LDS ray ring, the consumer and the launch geometry (gfx950, wave64).
//
// Same results as pt_traverse.h (Scene::intersect / testVisibility, Core/SurfaceObject.cpp:408-430; QBVH::intersect,
// Accelerator/QBVH.h:295-339; Triangle::intersect, Surface/TriangleMesh.cpp:131-178) — the same slab, triangle, tie-rule and
// instance functions — on a different schedule.
//
// Why: PMC on the batch kernels showed 19-21 % VALU lane utilisation (SQ_THREAD_CYCLES_VALU / (64 x SQ_ACTIVE_INST_VALU)):
// a wave of 64 rays runs until its LONGEST ray is done, and in this scene most rays need 3-4 nodes while a few need 20+.
// Refilling idle lanes needs new rays without stalling the lanes that are still traversing, and loads return in order
// per wave (vmcnt), so a wave cannot prefetch from HBM behind its own node fetches.  Hence two roles per workgroup:
//
//   wave 0      PRODUCER: makes or streams the rays of the launch and appends them to a ring of rays in LDS (wsProduce,
//               pt_trace_ws.hip: the render's slots and shadow queue; wsProduceIndexed: rays numbered 0 .. n-1).
//   waves 1..NC CONSUMERS (NC = 7; 15 on large trees): one lane = one ray; whenever `refill` or more lanes are idle the wave
//               reserves that many ring entries (one LDS compare-and-swap by lane 0) and the idle lanes start on them, while the
//               other lanes carry on mid-traversal.  A traversal step is one node (four slab tests) or ONE triangle, so lanes in
//               different phases interleave at fine grain.
//
// All hand-offs are LDS atomics at workgroup scope; no global atomics, no inter-workgroup communication.  Every spin is
// bounded (kSpinLimit) so a logic error ends the kernel instead of hanging the GPU.
//
// Nothing here names a client: who feeds the ring and where the results go is the including file's business
// (pt_trace_ws.hip: the render; pt_trace_indexed.hip: ray queries, the feature trace, the primary pass).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "pt_traverse.h"

namespace slrhip {

// NC = consumer waves per workgroup (3 -> 256 threads, 7 -> 512, 15 -> 1 024); the ring holds 64 x (NC + 1) rays (512 for NC = 15)
static const int kWsLdsStack = 11;          // + 1 trash row = 12 rows of 64 lanes = 3 KiB per consumer wave
static const int kWsSpill = 53;            // 11 + 53 = the reference's 64-entry stack (QBVH.h:299)
static const int kSub = 2;                 // 64-slot sub-chunks the producer keeps in flight
static const uint32_t kSpinLimit = 1u << 22;
static const uint32_t kIdle = 0xFFFFFFFFu;
static const uint32_t kShadowBit = 0x80000000u;   // ring slot word: bit 31 = shadow (any-hit) ray, bits 30..0 = slot

template <int NC>
struct WsLds {
    static constexpr uint32_t kRing = NC == 15 ? 512u : 64u * (NC + 1);      // ray ring entries (power of two)
    float4 org[kRing];                     // xyz + tmin
    float4 dir[kRing];                     // xyz + tmax
    uint32_t slot[kRing];
    uint32_t stack[NC][(kWsLdsStack + 1) * 64];
    uint32_t tail;                         // entries published by the producer
    uint32_t reserved;                     // entries claimed by consumers
    uint32_t released;                     // entries consumers have finished reading (ring space)
    uint32_t done;                         // producer has published its last entry
    uint32_t red[NC + 1];
};

// ---- launch geometry ---------------------------------------------------------------------------------------------------------
// The measurement overrides, read once (tuning builds only: tuningEnv): idle lanes that trigger a refill (SLRHIP_WS_REFILL,
// 1 .. 64), consumer waves per workgroup (SLRHIP_WS_NC: 3, 7 or 15; 0 = by tree size) and workgroups per CU
// (SLRHIP_WS_BLOCKS_PER_CU: 1 .. 8; 0 = by NC).  Defined in pt_trace_ws.hip.
struct WsTuning {
    uint32_t refill = 20;
    int consumers = 0;
    int blocksPerCU = 0;
};
const WsTuning& wsTuning();
// consumer waves of the render's traversal: 15 on quantized (large) trees, else 7
inline int wsConsumers(bool quantized) { return wsTuning().consumers ? wsTuning().consumers : (quantized ? 15 : 7); }
// resident workgroups per CU: 32 waves per CU (<= 64 VGPR) at 64.5 / 39.5 / 18.5 KiB of LDS per workgroup
static_assert(2 * sizeof(WsLds<15>) <= 163840 && 4 * sizeof(WsLds<7>) <= 163840 && 8 * sizeof(WsLds<3>) <= 163840, "LDS per CU");
inline int wsBlocksPerCU(int nc) { return wsTuning().blocksPerCU ? wsTuning().blocksPerCU : nc == 15 ? 2 : nc == 7 ? 4 : 8; }
// f(std::integral_constant<int, NC>) for the NC of a launch
template <class F>
void dispatchNc(int nc, F&& f) {
    if (nc == 15) f(std::integral_constant<int, 15>());
    else if (nc == 7) f(std::integral_constant<int, 7>());
    else f(std::integral_constant<int, 3>());
}

// streamed once per launch: keep them out of the vector L1 so that it stays with the BVH nodes
typedef float wsFloat4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ntLoad4(const float4* p) {
    const wsFloat4 v = __builtin_nontemporal_load(reinterpret_cast<const wsFloat4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void ntStore4(float4* p, float4 q) {
    wsFloat4 v = {q.x, q.y, q.z, q.w};
    __builtin_nontemporal_store(v, reinterpret_cast<wsFloat4*>(p));
}

#define WS_LOAD(p, order) __hip_atomic_load((p), order, __HIP_MEMORY_SCOPE_WORKGROUP)
#define WS_STORE(p, v, order) __hip_atomic_store((p), (v), order, __HIP_MEMORY_SCOPE_WORKGROUP)

template <class LDS>
__device__ __forceinline__ void wsResetRing(LDS& lds) {
    if (threadIdx.x == 0) { lds.tail = 0; lds.reserved = 0; lds.released = 0; lds.done = 0; }
    __syncthreads();
}

// Append the rays of one 64-lane sub-chunk that are live; returns how many were appended (wave-uniform).
template <class LDS>
__device__ __forceinline__ uint32_t wsAppend(LDS& lds, uint32_t tailLocal, bool live, uint32_t slot, float4 o, float4 d) {
    const uint64_t mask = __ballot(live);
    if (live) {
        const uint32_t lane = threadIdx.x & 63u;
        const uint32_t pos = (tailLocal + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))) & (LDS::kRing - 1);
        lds.org[pos] = o;
        lds.dir[pos] = d;
        lds.slot[pos] = slot;
    }
    return (uint32_t)__popcll(mask);
}

// Wait until the ring can take `need` more entries.  Returns false if the bound was hit (never expected).
template <class LDS>
__device__ __forceinline__ bool wsWaitSpace(LDS& lds, uint32_t tailLocal, uint32_t need, uint32_t* waits) {
    for (uint32_t spin = 0; spin < kSpinLimit; ++spin) {
        const uint32_t rel = WS_LOAD(&lds.released, __ATOMIC_ACQUIRE);
        if (tailLocal + need - rel <= LDS::kRing) return true;
        ++*waits;
        __builtin_amdgcn_s_sleep(8);
    }
    return false;
}

// schedule diagnostics and traversal counts of the counting instantiations (COUNT)
struct WsDebug {
    uint32_t steps = 0, idleSpins = 0, refills = 0, producerWaits = 0, nodeBlocks = 0, triBlocks = 0, activeLanes = 0;
    uint64_t cycles = 0, idleCycles = 0;
};
struct WsCounts {
    uint32_t nodes[2] = {0, 0}, tris[2] = {0, 0};   // [0] closest, [1] shadow
};

// The consumer side: closest hit and any hit (kShadowBit of the ring's slot word), lane by lane.
// INST: the scene has instanced meshes (DevScene::instances).  A child reference that names an instance (leaf flag, count 0) takes
// the lane's ray to the mesh's local space (enterInstance, pt_traverse.h), pushes kPopInstance and goes on at the root of the
// mesh's tree (same node and leaf arrays).  When kPopInstance comes off the stack the mesh is done and the world ray comes back
// from six registers of its own (they fit under the 64-VGPR cap without more scratch; reading it again from the slot's record —
// two 16-byte loads that miss the caches, the producer streamed them — was 8 % slower).
// IO: where the consumer sends its results (finish<INST>) and its error bits (errorWord()).  The rays themselves always come
// through the LDS ring.
template <bool COUNT, int NC, bool QUANT, bool INST, class IO>
__device__ __forceinline__ void wsConsume(const DevScene& sc, const IO& io, WsLds<NC>& lds, uint32_t refill, WsCounts& cnt, WsDebug& dbg) {
    const uint64_t tStart = COUNT ? __builtin_readcyclecounter() : 0;
    constexpr uint32_t kRing = WsLds<NC>::kRing;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t* stack = lds.stack[(threadIdx.x >> 6) - 1] + lane;          // [entry][lane]
    const float4* __restrict__ nodes4 = sc.nodes;
    const float4* __restrict__ tris4 = sc.leafTris;

    uint32_t slot = kIdle;
    float ox = 0, oy = 0, oz = 0, dx = 0, dy = 0, dz = 0, idx = 0, idy = 0, idz = 0, tmin = 0, tmax = 0;
    uint32_t cur = 0;
    int sp = 0;
    uint32_t hitTri = 0xFFFFFFFFu;
    float hitT = INFINITY, hitB1 = 0.0f, hitB2 = 0.0f;
    int32_t inst = -1, hitInst = -1;           // INST: the instance the lane is inside / the one its closest hit went through
    float wox = 0, woy = 0, woz = 0, wdx = 0, wdy = 0, wdz = 0;      // the world ray while the lane is inside an instance
    // a reference that is a packet of triangles (INST: not an instance reference, not kPopInstance)
    const auto isTriLeaf = [](uint32_t ref) -> bool {
        if (!INST) return (ref & kLeafFlag) != 0;
        const uint32_t n = (ref >> kLeafCountShift) & 0xFu;
        return (ref & kLeafFlag) != 0 && n != 0u && n != 15u;
    };
    // The lane's stack: kWsLdsStack entries in its LDS column, then kWsSpill in scratch.  The host rejects trees that could overflow it.
    uint32_t spill[kWsSpill];
    const auto wsPush = [&](uint32_t ref) {
        if (sp < kWsLdsStack) { stack[sp * 64] = ref; ++sp; }
        else if (sp < kWsLdsStack + kWsSpill) { spill[sp - kWsLdsStack] = ref; ++sp; }
        else atomicOr(io.errorWord(), ERR_STACK_OVERFLOW);
    };
    // the next reference to visit comes off the stack — or the stack is empty and the ray is finished
    const auto wsPop = [&](bool& finished) {
        if (sp == 0) finished = true;
        else {
            --sp;
            if (sp < kWsLdsStack) cur = stack[sp * 64];
            else cur = spill[sp - kWsLdsStack];
        }
    };
    uint32_t idleSpins = 0;

    for (;;) {
        const uint64_t idleMask = __ballot(slot == kIdle);
        const uint32_t nIdle = (uint32_t)__popcll(idleMask);
        if (nIdle >= refill) {
            uint32_t start = 0, take = 0;
            if (lane == 0) {
                // reserved <= tail at all times and tail only grows: reading reserved FIRST makes tail - reserved >= 0
                for (int attempt = 0; attempt < 64; ++attempt) {
                    uint32_t r = WS_LOAD(&lds.reserved, __ATOMIC_RELAXED);
                    const uint32_t t = WS_LOAD(&lds.tail, __ATOMIC_ACQUIRE);
                    take = min(t - r, nIdle);
                    if (take == 0) break;
                    if (__hip_atomic_compare_exchange_strong(&lds.reserved, &r, r + take, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_WORKGROUP)) { start = r; break; }
                    take = 0;
                }
            }
            start = __builtin_amdgcn_readfirstlane(start);
            take = __builtin_amdgcn_readfirstlane(take);
            if (take) {
                idleSpins = 0;
                if (COUNT) ++dbg.refills;
                const uint32_t rank = (uint32_t)__popcll(idleMask & below);
                if (slot == kIdle && rank < take) {
                    const uint32_t pos = (start + rank) & (kRing - 1);
                    const float4 o = lds.org[pos], d = lds.dir[pos];
                    slot = lds.slot[pos];
                    ox = o.x; oy = o.y; oz = o.z; tmin = o.w;
                    dx = d.x; dy = d.y; dz = d.z; tmax = d.w;
                    idx = 1.0f / dx; idy = 1.0f / dy; idz = 1.0f / dz;          // Vector3.h:60 reciprocal()
                    cur = 0; sp = 0;
                    hitTri = 0xFFFFFFFFu; hitT = INFINITY; hitB1 = 0.0f; hitB2 = 0.0f;
                    inst = -1; hitInst = -1;
                }
                // Ring space is handed back IN RESERVATION ORDER: `released` is a watermark, the producer overwrites
                // everything below it, so this wave may only move it past its own entries once every earlier
                // reservation (another wave, possibly still reading) has been released.  The wait is a few hundred
                // cycles at most: the earlier wave is between its compare-and-swap and the end of its own ring reads.
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");           // the ring reads above are complete
                if (lane == 0) {
                    uint32_t spin = 0;
                    for (; spin < kSpinLimit && WS_LOAD(&lds.released, __ATOMIC_ACQUIRE) != start; ++spin)
                        __builtin_amdgcn_s_sleep(1);
                    if (spin == kSpinLimit) atomicOr(io.errorWord(), ERR_RING_RELEASE);     // never expected; the launch fails loudly
                    WS_STORE(&lds.released, start + take, __ATOMIC_RELEASE);
                }
            }
            else if (nIdle == 64) {
                // nothing in flight and nothing to take: finished, or the producer is behind
                if (WS_LOAD(&lds.done, __ATOMIC_ACQUIRE) && WS_LOAD(&lds.tail, __ATOMIC_ACQUIRE) == WS_LOAD(&lds.reserved, __ATOMIC_RELAXED)) break;
                if (++idleSpins > kSpinLimit) { if (lane == 0) atomicOr(io.errorWord(), ERR_CONSUMER_IDLE); break; }
                if (COUNT) {
                    const uint64_t t0 = __builtin_readcyclecounter();
                    __builtin_amdgcn_s_sleep(4);
                    dbg.idleCycles += __builtin_readcyclecounter() - t0;
                    ++dbg.idleSpins;
                }
                else __builtin_amdgcn_s_sleep(4);
                continue;
            }
        }

        if (COUNT) {
            ++dbg.steps;
            const uint64_t act = __ballot(slot != kIdle);
            dbg.activeLanes += (uint32_t)__popcll(act);
            if (__ballot(slot != kIdle && !(cur & kLeafFlag))) ++dbg.nodeBlocks;
        }
        if (INST && slot != kIdle && (cur & kLeafFlag) != 0 && !isTriLeaf(cur)) {
            // one step = entering or leaving an instance
            bool finished = false;
            if (cur == kPopInstance) {
                ox = wox; oy = woy; oz = woz;
                dx = wdx; dy = wdy; dz = wdz;
                inst = -1;
                wsPop(finished);
            }
            else {
                const uint32_t k = cur & kLeafIndexMask;
                V3 lo, ld;
                const uint32_t root = enterInstance(sc, k, V3(ox, oy, oz), V3(dx, dy, dz), lo, ld);
                wox = ox; woy = oy; woz = oz; wdx = dx; wdy = dy; wdz = dz;
                ox = lo.x; oy = lo.y; oz = lo.z;
                dx = ld.x; dy = ld.y; dz = ld.z;
                wsPush(kPopInstance);
                cur = root;
                inst = (int32_t)k;
            }
            idx = 1.0f / dx; idy = 1.0f / dy; idz = 1.0f / dz;          // Vector3.h:60 reciprocal()
            if (finished) {
                io.template finish<INST>(slot, hitTri, hitT, hitB1, hitB2, hitInst);
                slot = kIdle;
            }
        }
        // (not `else`: a lane that has just entered or left an instance goes on with its node or triangle step in the same turn)
        if (slot != kIdle && !(INST && (cur & kLeafFlag) != 0 && !isTriLeaf(cur))) {
            bool finished = false;
            // Two schedules of the same steps, by tree class (measured per class, as the consumer count is):
            //  * float nodes without instances (kOneTrip): the kind of this turn's step — a node, or ONE triangle of the leaf packet
            //    the lane stands at — is fixed here, before any load, and one round trip serves both kinds.  A lane needs the three
            //    16-byte pieces of its triangle record OR the near planes of its node, never both, so the same three loads fetch
            //    either into the same twelve registers (their base differs from lane to lane: a 64-bit address each); the far planes
            //    and the children are loaded by the node lanes alone.  The loads of the lanes at a leaf are on their way while the
            //    node lanes do their slab test and stack work.  A lane whose node step ends on a leaf tests that leaf's first
            //    triangle in its NEXT turn.
            //  * quantized nodes, instanced scenes: the node block with its loads, then the triangle block with its own loads for
            //    every lane that stands at a leaf now — a lane whose node step ended on a leaf tests the first triangle in the same turn.
            // Either way a ray visits the same nodes and tests the same triangles in the same order.
            constexpr bool kOneTrip = !QUANT && !INST;
            const bool atLeaf = isTriLeaf(cur);
            const char* nb = QUANT ? reinterpret_cast<const char*>(sc.nodesQ) : reinterpret_cast<const char*>(nodes4);
            const char* tb = reinterpret_cast<const char*>(tris4);
            const uint32_t nOff = cur * (QUANT ? 64u : 128u);
            // float4 index inside a 128-byte node: 0..2 = min xyz, 3..5 = max xyz, 6 = children (QBVH.h:66-71 folded into offsets)
            const uint32_t nx = idx > 0.0f ? 0u : 48u, ny = idy > 0.0f ? 16u : 64u, nz = idz > 0.0f ? 32u : 80u;
            float4 s0, s1, s2;
            if (kOneTrip) {
                const char* row = (atLeaf ? tb : nb) + (atLeaf ? (cur & kLeafIndexMask) * 48u : nOff);
                s0 = *reinterpret_cast<const float4*>(row + (atLeaf ? 0u : nx));
                s1 = *reinterpret_cast<const float4*>(row + (atLeaf ? 16u : ny));
                s2 = *reinterpret_cast<const float4*>(row + (atLeaf ? 32u : nz));
            }
            // dbg.triBlocks = triangle blocks executed: counted by the first active lane, summed over lanes at the end
            const auto countTriBlock = [&](bool lanes) {
                if (__ballot(lanes) && (threadIdx.x & 63u) == (uint32_t)__ffsll((long long)__ballot(true)) - 1u) ++dbg.triBlocks;
            };
            if (COUNT && kOneTrip) countTriBlock(atLeaf);
            if (!atLeaf) {
                if (COUNT) { const bool sh = (slot & kShadowBit) != 0; cnt.nodes[0] += sh ? 0u : 1u; cnt.nodes[1] += sh ? 1u : 0u; }
                float4 nX, nY, nZ, fX, fY, fZ, ch;
                if (QUANT) {
                    // 64-byte node, 8-bit child boxes (device_types.h QNodeQ): plane = fma(byte, scale, origin), rounded outwards by
                    // the host, so the boxes are supersets of the float boxes and the set of hits is unchanged
                    const float4 v0 = *reinterpret_cast<const float4*>(nb + nOff);
                    const float4 v1 = *reinterpret_cast<const float4*>(nb + (nOff + 16u));
                    const float4 v2 = *reinterpret_cast<const float4*>(nb + (nOff + 32u));
                    ch = *reinterpret_cast<const float4*>(nb + (nOff + 48u));
                    const uint32_t qlox = __float_as_uint(v1.z), qloy = __float_as_uint(v1.w), qloz = __float_as_uint(v2.x);
                    const uint32_t qhix = __float_as_uint(v2.y), qhiy = __float_as_uint(v2.z), qhiz = __float_as_uint(v2.w);
                    const uint32_t nqx = idx > 0.0f ? qlox : qhix, fqx = idx > 0.0f ? qhix : qlox;      // QBVH.h:66-71
                    const uint32_t nqy = idy > 0.0f ? qloy : qhiy, fqy = idy > 0.0f ? qhiy : qloy;
                    const uint32_t nqz = idz > 0.0f ? qloz : qhiz, fqz = idz > 0.0f ? qhiz : qloz;
#define WS_DEQ(q, sh, scale, org) __builtin_fmaf((float)(((q) >> (sh)) & 0xFFu), scale, org)
#define WS_DEQ4(q, scale, org) make_float4(WS_DEQ(q, 0, scale, org), WS_DEQ(q, 8, scale, org), WS_DEQ(q, 16, scale, org), WS_DEQ(q, 24, scale, org))
                    nX = WS_DEQ4(nqx, v0.w, v0.x); fX = WS_DEQ4(fqx, v0.w, v0.x);
                    nY = WS_DEQ4(nqy, v1.x, v0.y); fY = WS_DEQ4(fqy, v1.x, v0.y);
                    nZ = WS_DEQ4(nqz, v1.y, v0.z); fZ = WS_DEQ4(fqz, v1.y, v0.z);
#undef WS_DEQ4
#undef WS_DEQ
                }
                else {
                    // 32-bit byte offsets from the (uniform) array base: SGPR-base + VGPR-offset addressing, one VALU op per load
                    // instead of a 64-bit address computation (node array < 4 GiB: checked at upload)
                    if (kOneTrip) { nX = s0; nY = s1; nZ = s2; }
                    else {
                        nX = *reinterpret_cast<const float4*>(nb + (nOff + nx));
                        nY = *reinterpret_cast<const float4*>(nb + (nOff + ny));
                        nZ = *reinterpret_cast<const float4*>(nb + (nOff + nz));
                    }
                    fX = *reinterpret_cast<const float4*>(nb + (nOff + (48u - nx)));
                    fY = *reinterpret_cast<const float4*>(nb + (nOff + (80u - ny)));
                    fZ = *reinterpret_cast<const float4*>(nb + (nOff + (112u - nz)));
                    ch = *reinterpret_cast<const float4*>(nb + (nOff + 96u));
                }
                const uint32_t c[4] = {__float_as_uint(ch.x), __float_as_uint(ch.y), __float_as_uint(ch.z), __float_as_uint(ch.w)};
                float tn[4];
                bool h[4];
                // nearest hit child is visited next; the rest go on the stack
                const uint32_t next = slabTest4(nX, nY, nZ, fX, fY, fZ, V3(ox, oy, oz), idx, idy, idz, tmin, tmax, c, tn, h);
                // the hit children other than `next` go on the stack in child order.  Fast path (all of them fit in the LDS
                // part): branch-free, a child that is not pushed writes the trash row kWsLdsStack of this lane's column.
                const bool v0 = h[0] && c[0] != next, v1 = h[1] && c[1] != next, v2 = h[2] && c[2] != next, v3 = h[3] && c[3] != next;
                const int nPush = (int)v0 + (int)v1 + (int)v2 + (int)v3;
                if (sp + nPush <= kWsLdsStack) {
                    int p = sp;
                    stack[(v0 ? p : kWsLdsStack) * 64] = c[0]; p += (int)v0;
                    stack[(v1 ? p : kWsLdsStack) * 64] = c[1]; p += (int)v1;
                    stack[(v2 ? p : kWsLdsStack) * 64] = c[2]; p += (int)v2;
                    stack[(v3 ? p : kWsLdsStack) * 64] = c[3]; p += (int)v3;
                    sp = p;
                }
                else {
                    if (v0) wsPush(c[0]);
                    if (v1) wsPush(c[1]);
                    if (v2) wsPush(c[2]);
                    if (v3) wsPush(c[3]);
                }
                if (next != kInvalidChild) cur = next;
                else wsPop(finished);
            }
            const bool triStep = kOneTrip ? atLeaf : !finished && isTriLeaf(cur);
            if (COUNT && !kOneTrip) countTriBlock(triStep);
            if (triStep) {
                // ONE triangle of the leaf packet per step; the reference tests them in order (QBVH.h:322-327)
                float4 a, b, c;
                if (kOneTrip) { a = s0; b = s1; c = s2; }
                else {
                    const uint32_t tOff = (cur & kLeafIndexMask) * 48u;
                    a = *reinterpret_cast<const float4*>(tb + tOff);
                    b = *reinterpret_cast<const float4*>(tb + (tOff + 16u));
                    c = *reinterpret_cast<const float4*>(tb + (tOff + 32u));
                }
                const uint32_t first = cur & kLeafIndexMask;
                const uint32_t count = (cur >> kLeafCountShift) & 0xF;
                const uint32_t triIdx = __float_as_uint(a.w);
                const bool anyHit = (slot & kShadowBit) != 0;
                if (COUNT) { cnt.tris[0] += anyHit ? 0u : 1u; cnt.tris[1] += anyHit ? 1u : 0u; }
                const TriHit th = triangleTest(sc, a, b, c, V3(ox, oy, oz), V3(dx, dy, dz), tmin, tmax);
                // One trip: the triangle test reads no fourth word of the record's last piece, the node block reads all four of its
                // plane.  Left to itself the compiler loads three words for every lane and the fourth in the node block: an eighth
                // request per node visit into the vector L1, the unit this kernel is bound by (measured: +12 % tag look-ups, the gain
                // gone).  Naming the word here (no instruction) keeps the shared load whole.
                if (kOneTrip) asm volatile("" :: "v"(c.w));
                if (th.accept) {
                    if (anyHit) {
                        hitTri = triIdx;
                        finished = true;
                    }
                    else if (closerHit<INST>(th.t, tmax, hitTri != 0xFFFFFFFFu, inst, triIdx, hitInst, hitTri)) {
                        tmax = th.t;                                // ray.distMax = isect->dist (QBVH.h:335)
                        hitTri = triIdx;
                        if (INST) hitInst = inst;
                        hitT = th.t;
                        hitB1 = th.b1;                              // Intersection::u = 1 - b1 - b2, ::v = b1 (TriangleMesh.cpp:159,172-173)
                        hitB2 = th.b2;
                    }
                }
                if (!finished) {
                    if (count > 1) cur = kLeafFlag | ((count - 1) << kLeafCountShift) | (first + 1);
                    else wsPop(finished);
                }
            }
            if (finished) {
                io.template finish<INST>(slot, hitTri, hitT, hitB1, hitB2, hitInst);
                slot = kIdle;
            }
        }
    }
    if (COUNT) dbg.cycles = __builtin_readcyclecounter() - tStart;
}

// The producer of a launch whose rays are numbered 0 .. n-1 (ray queries: indices into the caller's array; feature and primary
// passes: samples of the window): workgroup b takes the 128-ray chunks b, b + gridDim, ... (the grid is at most the resident grid,
// so every workgroup is resident and the chunks of one workgroup are its share).  makeRay(i, o, d) loads or computes ray i; a
// chunk's rays are made before the wait for ring space, so that their loads overlap it.  Every index is a ray: no state flags, no
// queue.  tag = kShadowBit for visibility queries.  Returns the rays appended (wave-uniform).
template <class LDS, class MakeRay>
__device__ __forceinline__ uint32_t wsProduceIndexed(uint32_t n, uint32_t tag, uint32_t* errorWord, LDS& lds, WsDebug& dbg, const MakeRay& makeRay) {
    const uint32_t lane = threadIdx.x;
    const uint32_t chunk = kSub * 64;
    const uint32_t numChunks = (n + chunk - 1) / chunk;           // n < 2^31: c * chunk + 127 stays inside 32 bits
    uint32_t tailLocal = 0;
    for (uint32_t c = blockIdx.x; c < numChunks; c += gridDim.x) {
        float4 o[kSub], d[kSub];
        bool live[kSub];
#pragma unroll
        for (int j = 0; j < kSub; ++j) {
            const uint32_t i = c * chunk + j * 64 + lane;
            live[j] = i < n;
            o[j] = make_float4(0, 0, 0, 0); d[j] = make_float4(0, 0, 0, 0);
            if (live[j]) makeRay(i, o[j], d[j]);
        }
        if (!wsWaitSpace(lds, tailLocal, chunk, &dbg.producerWaits)) { if (lane == 0) atomicOr(errorWord, ERR_RING_SPACE); break; }
#pragma unroll
        for (int j = 0; j < kSub; ++j) tailLocal += wsAppend(lds, tailLocal, live[j], (c * chunk + j * 64 + lane) | tag, o[j], d[j]);
        WS_STORE(&lds.tail, tailLocal, __ATOMIC_RELEASE);
    }
    WS_STORE(&lds.done, 1u, __ATOMIC_RELEASE);
    return tailLocal;
}

} // namespace slrhip
