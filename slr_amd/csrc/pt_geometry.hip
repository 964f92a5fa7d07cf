// pt_geometry.hip — device code of slrhip_set_vertices: new vertices for the uploaded scene (flat, or with instances), and everything that depends on
// vertices rebuilt in place from the kept vertex array — the tree keeps its shape and gets exact boxes.  gfx950, wave64.  Launches
// in stream order (a launch reads what earlier launches stored; nothing is handed between workgroups inside one):
//
//   k_vertices_store      one lane per caller's record: eleven 4-byte loads (the record is 44 bytes, 4-byte aligned), the finite check,
//                         eleven stores into the kept array.  A record with a non-finite float leaves its vertex as it was and sets
//                         SLRHIP_GEOMETRY_BAD_VERTEX with one atomic OR on a word of its own.
//   k_geometry_leaves     one lane per LeafTri record: its `tri` word, the index triple, three positions; v0 / e1 / e2 (pt_triangle.h:
//                         the upload's arithmetic) with the record's w words kept; the triangle's exact box (min / max over the
//                         positions) into the box scratch; the texture coordinates of its alpha record where it has one.
//   k_geometry_triangles  one lane per scene triangle: ShadeTri (`material` and `light` kept) and, with textures, triUV.
//   k_geometry_lights     one lane per light: LightTri::tri names the triangle; both copies (lightTris and the shade tables' segment).
//   k_geometry_refit      the child boxes of every node, bottom-up, one lane per (node, child), pt_refit.h's rule: a packet takes the
//                         union of its triangles' scratch boxes, an inner child the union of the valid child boxes of the node it
//                         names, an empty slot keeps its bytes.  A level wider than kRefitGroupNodes is a launch of its own; a run of
//                         consecutive narrower levels is ONE workgroup with a barrier between levels (k_geometry_refit_levels).
//   k_geometry_quantize   one lane per node: QNodeQ from the refitted float node (pt_quantize.h), when the quantized nodes are in use.
//
//
// A scene with instances (SLRHIP_FLAG_DYNAMIC_INSTANCED as well) runs the same four record kernels — LeafTri records of the top
// level's loose packets and of every mesh share one array, and a mesh's triangles stay in its local space — and then, instead of
// k_geometry_refit over one tree:
//   k_geometry_mesh_refit    ALL mesh trees at once, by the merged level list (level d of every mesh is one run of node indices): the
//                            same child rule and the same grouping by width, so the launches are bounded by the deepest mesh.
//   k_geometry_instance_boxes  one lane per instance: its mesh's box = the union of the valid child boxes of the mesh's root, its
//                            world box = instanceWorldBox of that (pt_instance.h); lanes below the number of meshes store the mesh boxes.
//   the top-level refit      pt_instances.hip's launchTopRefit, here with the leaf boxes: instance children take the new world boxes,
//                            loose packets the union of their triangles' boxes.
//   k_geometry_packet_boxes  where slrhip_rebuild_top_level has built its tables: the loose packets' boxes in its canonical order.
//
// No atomics but the status bit, no parent pointers, no flags between workgroups: the order comes from the launches.
#include <hip/hip_runtime.h>

#include "pt_geometry.h"
#include "pt_instance.h"
#include "pt_quantize.h"
#include "pt_triangle.h"

namespace slrhip {

namespace {

const uint32_t kVertexFloats = 11;
static_assert(sizeof(slrhip_vertex) == kVertexFloats * sizeof(float), "slrhip_vertex is eleven floats");

__global__ __launch_bounds__(256) void k_vertices_store(GeometryUpdate u) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= u.count) return;                                                 // count records at src; first + count <= numVertices
    const float* src = u.src + (size_t)t * kVertexFloats;
    float v[kVertexFloats];
    bool finite = true;
#pragma unroll
    for (uint32_t k = 0; k < kVertexFloats; ++k) {
        v[k] = src[k];
        finite = finite && fabsf(v[k]) <= 3.402823466e+38f;
    }
    if (!finite) {
        atomicOr(u.status, (uint32_t)SLRHIP_GEOMETRY_BAD_VERTEX);
        return;
    }
    float* dst = u.vertices + (size_t)(u.first + t) * kVertexFloats;
#pragma unroll
    for (uint32_t k = 0; k < kVertexFloats; ++k) dst[k] = v[k];
}

__device__ __forceinline__ slrhip_vertex loadVertex(const float* vertices, uint32_t i) {
    const float* p = vertices + (size_t)i * kVertexFloats;
    slrhip_vertex v;
    v.position[0] = p[0]; v.position[1] = p[1]; v.position[2] = p[2];
    v.normal[0] = p[3]; v.normal[1] = p[4]; v.normal[2] = p[5];
    v.tangent[0] = p[6]; v.tangent[1] = p[7]; v.tangent[2] = p[8];
    v.texcoord[0] = p[9]; v.texcoord[1] = p[10];
    return v;
}

// the index triple of triangle `tri`, or false for an index outside the kept arrays (never: the upload checked them)
__device__ __forceinline__ bool loadTriangle(const GeometryUpdate& u, uint32_t tri, uint32_t* v) {
    if (tri >= u.numTriangles) return false;
    const uint4 t = *reinterpret_cast<const uint4*>(u.triangles + tri);      // v[3], material
    v[0] = t.x; v[1] = t.y; v[2] = t.z;
    return t.x < u.numVertices && t.y < u.numVertices && t.z < u.numVertices;
}

__global__ __launch_bounds__(256) void k_geometry_leaves(GeometryUpdate u) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= u.numLeafTris) return;
    float4* rec = u.leafTris + (size_t)k * 3u;
    const float4 r0 = rec[0], r1 = rec[1], r2 = rec[2];
    uint32_t vi[3];
    if (!loadTriangle(u, __float_as_uint(r0.w), vi)) return;
    float p[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float* q = u.vertices + (size_t)vi[j] * kVertexFloats;
        p[j][0] = q[0]; p[j][1] = q[1]; p[j][2] = q[2];
    }
    LeafTri lt;
    leafTriEdges(p[0], p[1], p[2], lt);
    rec[0] = make_float4(lt.v0[0], lt.v0[1], lt.v0[2], r0.w);                 // tri
    rec[1] = make_float4(lt.e1[0], lt.e1[1], lt.e1[2], r1.w);                 // alpha
    rec[2] = make_float4(lt.e2[0], lt.e2[1], lt.e2[2], r2.w);
    float lo[3], hi[3];
    triangleBox(p[0], p[1], p[2], lo, hi);
    u.leafBoxes[2u * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
    u.leafBoxes[2u * (size_t)k + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    const uint32_t alpha = __float_as_uint(r1.w);
    if (alpha == kNoAlpha || alpha >= u.numAlphaRecords) return;
    float uv[6];
    triangleTexcoords(loadVertex(u.vertices, vi[0]), loadVertex(u.vertices, vi[1]), loadVertex(u.vertices, vi[2]), uv);
    float4* a = u.alphaTris + 2u * (size_t)alpha;
    const float4 tail = a[1];                                                 // .z: the texture's index, .w: 0
    a[0] = make_float4(uv[0], uv[1], uv[2], uv[3]);
    a[1] = make_float4(uv[4], uv[5], tail.z, tail.w);
}

__global__ __launch_bounds__(256) void k_geometry_triangles(GeometryUpdate u) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= u.numTriangles) return;
    uint32_t vi[3];
    if (!loadTriangle(u, i, vi)) return;
    const slrhip_vertex v0 = loadVertex(u.vertices, vi[0]), v1 = loadVertex(u.vertices, vi[1]), v2 = loadVertex(u.vertices, vi[2]);
    float4* rec = u.shadeTris + (size_t)i * 6u;
    const float material = rec[0].w, light = rec[1].w;                        // kept, as bits
    ShadeTri s;
    shadeTriGeometry(v0, v1, v2, s);
    rec[0] = make_float4(s.n0[0], s.n0[1], s.n0[2], material);
    rec[1] = make_float4(s.n1[0], s.n1[1], s.n1[2], light);
    rec[2] = make_float4(s.n2[0], s.n2[1], s.n2[2], s.areaPDF);
    rec[3] = make_float4(s.t0[0], s.t0[1], s.t0[2], s.gnx);
    rec[4] = make_float4(s.t1[0], s.t1[1], s.t1[2], s.gny);
    rec[5] = make_float4(s.t2[0], s.t2[1], s.t2[2], s.gnz);
    if (!u.triUV) return;
    float uv[6];
    triangleTexcoords(v0, v1, v2, uv);
    u.triUV[2u * (size_t)i] = make_float4(uv[0], uv[1], uv[2], uv[3]);
    u.triUV[2u * (size_t)i + 1u] = make_float4(uv[4], uv[5], 0.0f, 0.0f);
}

__global__ __launch_bounds__(256) void k_geometry_lights(GeometryUpdate u) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= u.numLights) return;
    float4* rec = u.lightTris + (size_t)i * 9u;
    const float tri = rec[0].w, material = rec[1].w;                          // kept, as bits
    uint32_t vi[3];
    if (!loadTriangle(u, __float_as_uint(tri), vi)) return;
    const slrhip_vertex v0 = loadVertex(u.vertices, vi[0]), v1 = loadVertex(u.vertices, vi[1]), v2 = loadVertex(u.vertices, vi[2]);
    ShadeTri s;
    shadeTriGeometry(v0, v1, v2, s);
    LightTri l;
    lightTriGeometry(v0, v1, v2, s, l);
    float4 out[9];
    out[0] = make_float4(l.p0[0], l.p0[1], l.p0[2], tri);
    out[1] = make_float4(l.p1[0], l.p1[1], l.p1[2], material);
    out[2] = make_float4(l.p2[0], l.p2[1], l.p2[2], l.areaPDF);
    out[3] = make_float4(l.n0[0], l.n0[1], l.n0[2], l.gnx);
    out[4] = make_float4(l.n1[0], l.n1[1], l.n1[2], l.gny);
    out[5] = make_float4(l.n2[0], l.n2[1], l.n2[2], l.gnz);
    out[6] = make_float4(l.t0[0], l.t0[1], l.t0[2], 0.0f);
    out[7] = make_float4(l.t1[0], l.t1[1], l.t1[2], 0.0f);
    out[8] = make_float4(l.t2[0], l.t2[1], l.t2[2], 0.0f);
#pragma unroll
    for (int q = 0; q < 9; ++q) rec[q] = out[q];
    if (!u.stagedLights) return;
    float4* staged = u.stagedLights + (size_t)i * 9u;
#pragma unroll
    for (int q = 0; q < 9; ++q) staged[q] = out[q];
}

// One level of more than kRefitGroupNodes nodes: nodes [first, first + count), four lanes each.
__global__ __launch_bounds__(kRefitBlock) void k_geometry_refit(float4* nodes, const float4* leafBoxes, uint32_t first, uint32_t count, uint32_t numNodes,
                                                                uint32_t numLeafTris) {
    const uint32_t t = blockIdx.x * kRefitBlock + threadIdx.x;
    if (t >= 4u * count) return;
    refitChild(nodes, nullptr, leafBoxes, first + (t >> 2), t & 3u, numNodes, 0u, numLeafTris);
}

// Levels levelHi, levelHi - 1, .. levelLo, each of at most kRefitGroupNodes nodes: one workgroup, a barrier between levels.
__global__ __launch_bounds__(kRefitBlock) void k_geometry_refit_levels(GeometryUpdate u, uint32_t levelHi, uint32_t levelLo) {
    const uint32_t t = threadIdx.x;
    for (uint32_t level = levelHi + 1u; level-- > levelLo;) {                 // uniform over the workgroup: every lane reaches every barrier
        const uint32_t first = u.levelFirst[level], count = u.levelFirst[level + 1u] - first;
        if (t < 4u * count) refitChild(u.nodes, nullptr, u.leafBoxes, first + (t >> 2), t & 3u, u.numNodes, 0u, u.numLeafTris);
        __syncthreads();
    }
}

// ---- a scene with instances: the mesh trees lie behind the top level, and their levels are the merged list's ----

// One merged level of more than kRefitGroupNodes entries: entries [first, first + count) of the list, four lanes each.
__global__ __launch_bounds__(kRefitBlock) void k_geometry_mesh_refit(float4* nodes, const float4* leafBoxes, const uint32_t* __restrict__ list, uint32_t first,
                                                                     uint32_t count, uint32_t numNodes, uint32_t numLeafTris) {
    const uint32_t t = blockIdx.x * kRefitBlock + threadIdx.x;
    if (t >= 4u * count) return;
    const uint32_t node = list[first + (t >> 2)];
    if (node < numNodes) refitChild(nodes, nullptr, leafBoxes, node, t & 3u, numNodes, 0u, numLeafTris);      // (always: the upload wrote the list)
}

// Merged levels levelHi, levelHi - 1, .. levelLo, each of at most kRefitGroupNodes entries: one workgroup, a barrier between levels.
__global__ __launch_bounds__(kRefitBlock) void k_geometry_mesh_refit_levels(GeometryUpdate u, uint32_t levelHi, uint32_t levelLo) {
    const uint32_t t = threadIdx.x;
    for (uint32_t level = levelHi + 1u; level-- > levelLo;) {                 // uniform over the workgroup: every lane reaches every barrier
        const uint32_t first = u.meshLevelFirst[level], count = u.meshLevelFirst[level + 1u] - first;
        if (t < 4u * count) {
            const uint32_t node = u.meshLevelNodes[first + (t >> 2)];
            if (node < u.numNodes) refitChild(u.nodes, nullptr, u.leafBoxes, node, t & 3u, u.numNodes, 0u, u.numLeafTris);
        }
        __syncthreads();
    }
}

// the exact union of the valid child boxes of node `root`: a mesh's local box
__device__ __forceinline__ void rootBox(const float4* nodes, uint32_t root, float* lo, float* hi) {
    const float4* n = nodes + (size_t)root * 8u;
    const float4 p0 = n[0], p1 = n[1], p2 = n[2], p3 = n[3], p4 = n[4], p5 = n[5];
    const uint4 refs = *reinterpret_cast<const uint4*>(n + 6);
    lo[0] = unionMin(p0, refs); lo[1] = unionMin(p1, refs); lo[2] = unionMin(p2, refs);
    hi[0] = unionMax(p3, refs); hi[1] = unionMax(p4, refs); hi[2] = unionMax(p5, refs);
}

// One lane per instance: its mesh's box from the mesh's refitted root, its world box (pt_instance.h: the upload's arithmetic) from
// that and its localToWorld.  Lanes k < numMeshes also store mesh k's box (numMeshes <= numInstances: every mesh is placed).  Every
// lane takes the union it needs itself; no lane reads what another lane of this launch stores.
__global__ __launch_bounds__(256) void k_geometry_instance_boxes(GeometryUpdate u) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= u.numInstances) return;
    float lo[3], hi[3];
    if (k < u.numMeshes) {
        const uint32_t root = u.meshRoots[k];
        if (root < u.numNodes) {
            rootBox(u.nodes, root, lo, hi);
            u.meshBoxes[2u * (size_t)k] = make_float4(lo[0], lo[1], lo[2], 0.0f);
            u.meshBoxes[2u * (size_t)k + 1u] = make_float4(hi[0], hi[1], hi[2], 0.0f);
        }
    }
    const float4* rec = u.instances + (size_t)k * 9u;
    const uint4 tail = *reinterpret_cast<const uint4*>(rec + 8);              // rootNode, firstTriangle, numTriangles, mesh
    if (tail.x >= u.numNodes) return;                                         // (never: written by the upload)
    rootBox(u.nodes, tail.x, lo, hi);
    float m[16];                                                              // localToWorld
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 v = rec[q];
        m[4 * q] = v.x; m[4 * q + 1] = v.y; m[4 * q + 2] = v.z; m[4 * q + 3] = v.w;
    }
    float wlo[3], whi[3];
    instanceWorldBox(lo, hi, m, wlo, whi);
    u.instBoxes[2u * (size_t)k] = make_float4(wlo[0], wlo[1], wlo[2], 0.0f);
    u.instBoxes[2u * (size_t)k + 1u] = make_float4(whi[0], whi[1], whi[2], 0.0f);
}

// One lane per loose-triangle packet of slrhip_rebuild_top_level's canonical order: the union of its triangles' boxes into the table
// a later rebuild seats the packet with.
__global__ __launch_bounds__(256) void k_geometry_packet_boxes(GeometryUpdate u) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= u.numTopPackets) return;
    const uint32_t ref = u.topPacketRefs[p];
    const uint32_t count = (ref >> kLeafCountShift) & 0xFu, k = ref & kLeafIndexMask;
    if (!(ref & kLeafFlag) || ref == kInvalidChild || count == 0u || count > kMaxLeafTris || (uint64_t)k + count > u.numLeafTris) return;      // (never)
    float4 a = u.leafBoxes[2u * (size_t)k], b = u.leafBoxes[2u * (size_t)k + 1u];
    for (uint32_t j = 1; j < count; ++j) {
        const float4 a2 = u.leafBoxes[2u * (size_t)(k + j)], b2 = u.leafBoxes[2u * (size_t)(k + j) + 1u];
        a.x = fminf(a.x, a2.x); a.y = fminf(a.y, a2.y); a.z = fminf(a.z, a2.z);
        b.x = fmaxf(b.x, b2.x); b.y = fmaxf(b.y, b2.y); b.z = fmaxf(b.z, b2.z);
    }
    u.topPacketBoxes[2u * (size_t)p] = make_float4(a.x, a.y, a.z, 0.0f);
    u.topPacketBoxes[2u * (size_t)p + 1u] = make_float4(b.x, b.y, b.z, 0.0f);
}

__global__ __launch_bounds__(256) void k_geometry_quantize(const QNode* __restrict__ nodes, QNodeQ* __restrict__ nodesQ, uint32_t numNodes) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= numNodes) return;
    const QNode qn = nodes[i];
    nodesQ[i] = quantizeNode(qn);
}

inline dim3 gridOf(uint32_t lanes, uint32_t block) { return dim3((lanes + block - 1u) / block); }

// The refits of a scene with instances, after the records: every mesh tree by merged levels from the deepest to the roots, the meshes'
// and the instances' boxes, the top level (pt_instances.hip, with the leaf boxes: its loose packets moved too), and the packet boxes of
// slrhip_rebuild_top_level where its tables exist.  Returns the launches.
uint32_t launchInstancedRefit(const GeometryUpdate& u, hipStream_t stream) {
    uint32_t launches = 0;
    for (uint32_t level = u.numMeshLevels; level-- > 0u;) {
        const uint32_t first = u.meshLevelFirst[level], count = u.meshLevelFirst[level + 1u] - first;
        ++launches;
        if (count > kRefitGroupNodes) {
            hipLaunchKernelGGL(k_geometry_mesh_refit, gridOf(4u * count, kRefitBlock), dim3(kRefitBlock), 0, stream, u.nodes, u.leafBoxes, u.meshLevelNodes, first,
                               count, u.numNodes, u.numLeafTris);
            continue;
        }
        uint32_t lo = level;
        while (lo > 0u && u.meshLevelFirst[lo] - u.meshLevelFirst[lo - 1u] <= kRefitGroupNodes) --lo;
        hipLaunchKernelGGL(k_geometry_mesh_refit_levels, dim3(1), dim3(kRefitBlock), 0, stream, u, level, lo);
        level = lo;
    }
    hipLaunchKernelGGL(k_geometry_instance_boxes, gridOf(u.numInstances, 256u), dim3(256), 0, stream, u); ++launches;
    InstanceUpdate top{};                                                     // the refit's part of it
    top.numInstances = u.numInstances; top.topNodes = u.levelFirst[u.numLevels]; top.numLevels = u.numLevels;
    top.instBoxes = u.instBoxes; top.leafBoxes = u.leafBoxes; top.numLeafBoxes = u.numLeafTris; top.nodes = u.nodes;
    for (uint32_t l = 0; l <= u.numLevels; ++l) top.levelFirst[l] = u.levelFirst[l];
    launches += launchTopRefit(top, stream);
    if (u.topPacketRefs && u.numTopPackets) { hipLaunchKernelGGL(k_geometry_packet_boxes, gridOf(u.numTopPackets, 256u), dim3(256), 0, stream, u); ++launches; }
    return launches;
}

} // namespace

uint32_t launchGeometryLights(const GeometryUpdate& u, hipStream_t stream) {
    if (!u.numLights) return 0u;
    hipLaunchKernelGGL(k_geometry_lights, gridOf(u.numLights, 256u), dim3(256), 0, stream, u);
    return 1u;
}

uint32_t launchGeometryUpdate(const GeometryUpdate& u, hipStream_t stream) {
    uint32_t launches = 0;
    hipLaunchKernelGGL(k_vertices_store, gridOf(u.count, 256u), dim3(256), 0, stream, u); ++launches;
    hipLaunchKernelGGL(k_geometry_leaves, gridOf(u.numLeafTris, 256u), dim3(256), 0, stream, u); ++launches;
    hipLaunchKernelGGL(k_geometry_triangles, gridOf(u.numTriangles, 256u), dim3(256), 0, stream, u); ++launches;
    launches += launchGeometryLights(u, stream);
    if (u.numInstances) return launches + launchInstancedRefit(u, stream);
    // from the deepest level to the root; consecutive levels that fit one workgroup share a launch (as launchInstanceUpdate does)
    for (uint32_t level = u.numLevels; level-- > 0u;) {
        const uint32_t first = u.levelFirst[level], count = u.levelFirst[level + 1u] - first;
        ++launches;
        if (count > kRefitGroupNodes) {
            hipLaunchKernelGGL(k_geometry_refit, gridOf(4u * count, kRefitBlock), dim3(kRefitBlock), 0, stream, u.nodes, u.leafBoxes, first, count, u.numNodes,
                               u.numLeafTris);
            continue;
        }
        uint32_t lo = level;
        while (lo > 0u && u.levelFirst[lo] - u.levelFirst[lo - 1u] <= kRefitGroupNodes) --lo;
        hipLaunchKernelGGL(k_geometry_refit_levels, dim3(1), dim3(kRefitBlock), 0, stream, u, level, lo);
        level = lo;
    }
    if (u.nodesQ) {
        hipLaunchKernelGGL(k_geometry_quantize, gridOf(u.numNodes, 256u), dim3(256), 0, stream, reinterpret_cast<const QNode*>(u.nodes),
                           reinterpret_cast<QNodeQ*>(u.nodesQ), u.numNodes);
        ++launches;
    }
    return launches;
}

} // namespace slrhip
