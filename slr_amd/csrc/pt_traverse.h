// pt_traverse.h — the arithmetic of a traversal step, stated once, and the one-lane-one-ray traversal built on it (gfx950, wave64).
//
// slabTest4, triangleTest, closerHit and enterInstance are what every traversal of the library computes: the wave-specialised
// consumer (wsConsume, pt_trace_ws.h) and traverse() below call the same functions, so the two schedules cannot drift apart.
// traverse() is the closest-hit / any-hit traversal as a device function, used by the 64-ray-batch kernel of pt_trace.hip and by
// the tail kernel of pt_tail_kernels.h.  Same semantics as Scene::intersect / testVisibility (Core/SurfaceObject.cpp:408-430),
// QBVH::intersect (Accelerator/QBVH.h:295-339) and Triangle::intersect (Surface/TriangleMesh.cpp:131-178).
#pragma once
#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_kernels.h"
#include "pt_tex.h"

namespace slrhip {

static const int kTraceBlock = 256;
static const int kLdsStack = 8;
static const int kSpillStack = 56;     // 8 + 56 = the reference's 64-entry stack (QBVH.h:299)
static const int kTopNodes = 128;      // levels 0-3 of the 4-wide tree (1 + 4 + 16 + 64 = 85) and a bit
static const int kTopStride = 9;       // float4 per staged node: 8 + 1 pad -> 144 B, spreads nodes over the LDS banks

struct HitRec {
    uint32_t tri;
    float t, b1, b2;       // Moller-Trumbore's own barycentrics: b0 = 1 - b1 - b2 is re-derived where it is needed (logicSlot, pt_shade_visit.h)
    int32_t inst;          // INST: the instance the hit went through, -1 = a loose triangle
};
struct TravCount {
    uint32_t nodes, tris;
};

// The four children of a node against one ray: the slab test of QBVH::Node::intersect (QBVH.h:55-76), tNear <= tFar, on the near
// and far planes the caller picked by the sign of the reciprocal direction (QBVH.h:66-71).  Yields the entry distances, which
// children are hit, and returns the nearest hit child (kInvalidChild: none) — the one to visit next; the others go on the stack.
// The operand order of the fmaxf / fminf chains and -fno-fast-math are load-bearing: a NaN product (0 * inf) must be ignored
// (tests/test_traversal_edges.py).
// (Tried: fma(plane, id, -(o * id)) on padded boxes, half the arithmetic — but for rays that start ON a surface the cancellation
// noise near t = 0 admits the boxes around the origin: 3x the triangle tests for shadow rays, 4x slower on the 10 M grid.)
// (Tried: the 24 subtractions + 24 multiplications as packed fp32, v_pk_add_f32 / v_pk_mul_f32 — same roundings, 110 -> 87 VALU
// in this block — measured 23 % SLOWER per k_trace_ws launch: 1.55 -> 1.90 ms at 22 M slots.)
SLR_DEV uint32_t slabTest4(float4 nX, float4 nY, float4 nZ, float4 fX, float4 fY, float4 fZ, V3 org, float idx, float idy, float idz,
                           float tmin, float tmax, const uint32_t (&child)[4], float (&tn)[4], bool (&hit)[4]) {
    tn[0] = fmaxf(fmaxf((nX.x - org.x) * idx, (nY.x - org.y) * idy), fmaxf((nZ.x - org.z) * idz, tmin));
    tn[1] = fmaxf(fmaxf((nX.y - org.x) * idx, (nY.y - org.y) * idy), fmaxf((nZ.y - org.z) * idz, tmin));
    tn[2] = fmaxf(fmaxf((nX.z - org.x) * idx, (nY.z - org.y) * idy), fmaxf((nZ.z - org.z) * idz, tmin));
    tn[3] = fmaxf(fmaxf((nX.w - org.x) * idx, (nY.w - org.y) * idy), fmaxf((nZ.w - org.z) * idz, tmin));
    const float tf0 = fminf(fminf((fX.x - org.x) * idx, (fY.x - org.y) * idy), fminf((fZ.x - org.z) * idz, tmax));
    const float tf1 = fminf(fminf((fX.y - org.x) * idx, (fY.y - org.y) * idy), fminf((fZ.y - org.z) * idz, tmax));
    const float tf2 = fminf(fminf((fX.z - org.x) * idx, (fY.z - org.y) * idy), fminf((fZ.z - org.z) * idz, tmax));
    const float tf3 = fminf(fminf((fX.w - org.x) * idx, (fY.w - org.y) * idy), fminf((fZ.w - org.z) * idz, tmax));
    hit[0] = tn[0] <= tf0 && child[0] != kInvalidChild;
    hit[1] = tn[1] <= tf1 && child[1] != kInvalidChild;
    hit[2] = tn[2] <= tf2 && child[2] != kInvalidChild;
    hit[3] = tn[3] <= tf3 && child[3] != kInvalidChild;
    float best = INFINITY;
    uint32_t next = kInvalidChild;
    if (hit[0]) { best = tn[0]; next = child[0]; }
    if (hit[1] && tn[1] < best) { best = tn[1]; next = child[1]; }
    if (hit[2] && tn[2] < best) { best = tn[2]; next = child[2]; }
    if (hit[3] && tn[3] < best) { best = tn[3]; next = child[3]; }
    return next;
}

// One triangle (LeafTri as three float4: v0 | index, e1 | alpha record, e2) against one ray: Moller-Trumbore exactly as
// TriangleMesh.cpp:139-160, then the alpha texture of the triangle (TriangleMesh.cpp:162-167; LeafTri::alpha rides in e1's fourth
// word).  accept: the ray hits at t with Moller-Trumbore's own barycentrics b1, b2.  The arithmetic is the four expressions below;
// the two forms of the test differ only in when they look at the conditions: triangleTest evaluates all of them, traverse() leaves
// at the first that fails and spells that out in its loop (as a function of its own, whichever way it was written, the early-out
// form cost k_tail<RGB, true> a register: DESIGN.md 7.22).
struct TriHit { bool accept; float t, b1, b2; };
SLR_DEV float triDet(V3 dir, V3 e1, V3 e2, V3& p) { p = cross(dir, e2); return dot(e1, p); }
SLR_DEV float triB1(V3 d, V3 p, float invDet) { return dot(d, p) * invDet; }
SLR_DEV float triB2(V3 dir, V3 d, V3 e1, float invDet, V3& q) { q = cross(d, e1); return dot(dir, q) * invDet; }
SLR_DEV float triT(V3 e2, V3 q, float invDet) { return dot(e2, q) * invDet; }
// every condition evaluated and combined: wsConsume tests one triangle per step with its lanes in lock-step
SLR_DEV TriHit triangleTest(const DevScene& sc, float4 a, float4 b, float4 c, V3 org, V3 dir, float tmin, float tmax) {
    const V3 v0(a.x, a.y, a.z), e1(b.x, b.y, b.z), e2(c.x, c.y, c.z);
    TriHit r;
    V3 p, q;
    const float det = triDet(dir, e1, e2, p);
    r.accept = det != 0.0f;
    const float invDet = 1.0f / det;
    const V3 d = org - v0;
    r.b1 = triB1(d, p, invDet);
    r.accept = r.accept && !(r.b1 < 0.0f || r.b1 > 1.0f);
    r.b2 = triB2(dir, d, e1, invDet, q);
    r.accept = r.accept && !(r.b2 < 0.0f || r.b1 + r.b2 > 1.0f);
    r.t = triT(e2, q, invDet);
    r.accept = r.accept && !(r.t < tmin || r.t > tmax);
    if (r.accept && __float_as_uint(b.w) != kNoAlpha) r.accept = alphaPasses(sc.alphaTris, sc.textures, __float_as_uint(b.w), r.b1, r.b2);
    return r;
}

// Does an accepted hit at distance t replace the closest hit so far?  tmax is that hit's distance once there is one (haveHit), so
// only t == tmax needs a rule: at equal distance the larger scene index wins — the larger (instance, triangle) pair in instanced
// scenes (tree-independent tie rule).
template <bool INST>
SLR_DEV bool closerHit(float t, float tmax, bool haveHit, int32_t inst, uint32_t tri, int32_t hitInst, uint32_t hitTri) {
    return !(t == tmax && haveHit && (INST ? (inst < hitInst || (inst == hitInst && tri < hitTri)) : tri < hitTri));
}

// A ray enters instance k: TransformedSurfaceObject::intersect (Core/SurfaceObject.cpp:307-317), invert(sampledTF) * ray — the
// origin as a point (Matrix4x4 x Point3D, Matrix4x4.h:75-81; the bottom row is 0 0 0 1, so w == 1 and there is no division), the
// direction as a vector (:71-73) and NOT renormalised, so distances stay world distances and tmin / tmax carry over.
// DevInstance::worldToLocal is 3 x 4, column-major.  Returns the root of the mesh's tree.
SLR_DEV uint32_t enterInstance(const DevScene& sc, uint32_t k, V3 worldOrg, V3 worldDir, V3& org, V3& dir) {
    const float4* rec = sc.instances + (size_t)k * 9u + 4u;
    const float4 c0 = rec[0], c1 = rec[1], c2 = rec[2], c3 = rec[3], meta = rec[4];
    org = V3(c0.x * worldOrg.x + c1.x * worldOrg.y + c2.x * worldOrg.z + c3.x * 1.0f,
             c0.y * worldOrg.x + c1.y * worldOrg.y + c2.y * worldOrg.z + c3.y * 1.0f,
             c0.z * worldOrg.x + c1.z * worldOrg.y + c2.z * worldOrg.z + c3.z * 1.0f);
    dir = V3(c0.x * worldDir.x + c1.x * worldDir.y + c2.x * worldDir.z, c0.y * worldDir.x + c1.y * worldDir.y + c2.y * worldDir.z,
             c0.z * worldDir.x + c1.z * worldDir.y + c2.z * worldDir.z);
    return __float_as_uint(meta.x);
}

// INST: scenes with instanced meshes (DevScene::instances; see wsConsume in pt_trace_ws.h for the scheme).  Here too the world ray
// stays in registers while the lane is inside an instance.  The stack is this function's own: kLdsStack entries in LDS, the rest
// in scratch.
template <bool ANY_HIT, bool COUNT, bool INST = false>
__device__ __forceinline__ bool traverse(const DevScene& sc, const float4* __restrict__ nodes4, const float4* __restrict__ tris4, const float4* topNodes,
                                         uint32_t numTop, V3 org, V3 dir, float tmin, float tmax, HitRec* hit,
                                         uint32_t* ldsStack /* [kLdsStack][blockDim], this lane's column */, TravCount* cnt,
                                         uint32_t* errorWord = nullptr) {
    float idx = 1.0f / dir.x, idy = 1.0f / dir.y, idz = 1.0f / dir.z;      // Vector3.h:60 reciprocal()
    // float4 index inside a node: 0..2 = min xyz, 3..5 = max xyz, 6 = children
    int nx = idx > 0.0f ? 0 : 3, fx = 3 - nx;
    int ny = idy > 0.0f ? 1 : 4, fy = 5 - ny;
    int nz = idz > 0.0f ? 2 : 5, fz = 7 - nz;
    const V3 worldOrg = org, worldDir = dir;
    int32_t inst = -1;
    hit->inst = -1;

    uint32_t spill[kSpillStack];
    int sp = 0;
    uint32_t cur = 0;                      // root
    bool found = false;
    hit->tri = 0xFFFFFFFFu; hit->t = INFINITY; hit->b1 = 0.0f; hit->b2 = 0.0f;

    for (;;) {
        if (INST && (cur & kLeafFlag) && (((cur >> kLeafCountShift) & 0xFu) == 0u || cur == kPopInstance)) {
            const bool leaving = cur == kPopInstance;
            if (leaving) { org = worldOrg; dir = worldDir; inst = -1; }
            else {
                const uint32_t k = cur & kLeafIndexMask;
                const uint32_t root = enterInstance(sc, k, worldOrg, worldDir, org, dir);
                inst = (int32_t)k;
                if (sp < kLdsStack) ldsStack[sp * kTraceBlock] = kPopInstance;
                else if (sp < kLdsStack + kSpillStack) spill[sp - kLdsStack] = kPopInstance;
                else { if (errorWord) atomicOr(errorWord, ERR_STACK_OVERFLOW); --sp; }
                ++sp;
                cur = root;
            }
            idx = 1.0f / dir.x; idy = 1.0f / dir.y; idz = 1.0f / dir.z;
            nx = idx > 0.0f ? 0 : 3; fx = 3 - nx;
            ny = idy > 0.0f ? 1 : 4; fy = 5 - ny;
            nz = idz > 0.0f ? 2 : 5; fz = 7 - nz;
            if (!leaving) continue;
            if (sp == 0) break;
            --sp;
            cur = sp < kLdsStack ? ldsStack[sp * kTraceBlock] : spill[sp - kLdsStack];
            continue;
        }
        if (cur & kLeafFlag) {
            const uint32_t first = cur & kLeafIndexMask;
            const uint32_t count = (cur >> kLeafCountShift) & 0xF;
            for (uint32_t k = 0; k < count; ++k) {
                const float4* tp = tris4 + (size_t)(first + k) * 3;
                const float4 a = tp[0], b = tp[1], c = tp[2];
                const uint32_t triIdx = __float_as_uint(a.w);
                if (COUNT) ++cnt->tris;
                // triangleTest's conditions one at a time: the lane leaves at the first that fails
                const V3 v0(a.x, a.y, a.z), e1(b.x, b.y, b.z), e2(c.x, c.y, c.z);
                V3 p, q;
                const float det = triDet(dir, e1, e2, p);
                if (det == 0.0f) continue;
                const float invDet = 1.0f / det;
                const V3 d = org - v0;
                const float b1 = triB1(d, p, invDet);
                if (b1 < 0.0f || b1 > 1.0f) continue;
                const float b2 = triB2(dir, d, e1, invDet, q);
                if (b2 < 0.0f || b1 + b2 > 1.0f) continue;
                const float tt = triT(e2, q, invDet);
                if (tt < tmin || tt > tmax) continue;
                if (__float_as_uint(b.w) != kNoAlpha && !alphaPasses(sc.alphaTris, sc.textures, __float_as_uint(b.w), b1, b2)) continue;
                if (ANY_HIT) return true;
                if (!closerHit<INST>(tt, tmax, found, inst, triIdx, hit->inst, hit->tri)) continue;
                found = true;
                tmax = tt;                                  // ray.distMax = isect->dist (QBVH.h:335)
                hit->tri = triIdx;
                hit->inst = inst;
                hit->t = tt;
                hit->b1 = b1;                               // Intersection::u = 1 - b1 - b2, ::v = b1 (TriangleMesh.cpp:159,172-173)
                hit->b2 = b2;
            }
            if (sp == 0) break;
            --sp;
            cur = sp < kLdsStack ? ldsStack[sp * kTraceBlock] : spill[sp - kLdsStack];
            continue;
        }

        if (COUNT) ++cnt->nodes;
        float4 nX, nY, nZ, fX, fY, fZ, ch;
        if (cur < numTop) {
            const float4* n = topNodes + cur * kTopStride;
            nX = n[nx]; nY = n[ny]; nZ = n[nz]; fX = n[fx]; fY = n[fy]; fZ = n[fz]; ch = n[6];
        }
        else {
            const float4* n = nodes4 + (size_t)cur * 8;
            nX = n[nx]; nY = n[ny]; nZ = n[nz]; fX = n[fx]; fY = n[fy]; fZ = n[fz]; ch = n[6];
        }
        const uint32_t child[4] = {__float_as_uint(ch.x), __float_as_uint(ch.y), __float_as_uint(ch.z), __float_as_uint(ch.w)};
        float tn[4];
        bool h[4];
        // nearest hit child is visited next; the rest go on the stack
        const uint32_t next = slabTest4(nX, nY, nZ, fX, fY, fZ, org, idx, idy, idz, tmin, tmax, child, tn, h);
#define SLR_PUSH(cond, ref)                                                              \
        if ((cond) && (ref) != next) {                                                   \
            if (sp < kLdsStack) ldsStack[sp * kTraceBlock] = (ref);                      \
            else if (sp < kLdsStack + kSpillStack) spill[sp - kLdsStack] = (ref);        \
            else { if (errorWord) atomicOr(errorWord, ERR_STACK_OVERFLOW); --sp; }       \
            ++sp;                                                                        \
        }
        SLR_PUSH(h[0], child[0])
        SLR_PUSH(h[1], child[1])
        SLR_PUSH(h[2], child[2])
        SLR_PUSH(h[3], child[3])
#undef SLR_PUSH
        if (next != kInvalidChild) { cur = next; continue; }
        if (sp == 0) break;
        --sp;
        cur = sp < kLdsStack ? ldsStack[sp * kTraceBlock] : spill[sp - kLdsStack];
    }
    return found;
}

struct TraceLds {
    float4 top[kTopNodes * kTopStride];
    uint32_t stack[kLdsStack * kTraceBlock];
};

// Stage the top of the tree: coalesced 16-byte loads, padded rows in LDS.
__device__ __forceinline__ uint32_t stageTopNodes(const DevScene& sc, TraceLds& lds) {
    const uint32_t numTop = min(sc.numNodes, (uint32_t)kTopNodes);
    for (uint32_t i = threadIdx.x; i < numTop * 8; i += kTraceBlock) lds.top[(i >> 3) * kTopStride + (i & 7)] = sc.nodes[i];
    __syncthreads();
    return numTop;
}

} // namespace slrhip
