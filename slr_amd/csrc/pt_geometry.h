// pt_geometry.h — what slrhip_set_vertices hands its device code (pt_geometry.hip): the kept vertex and index arrays of a context
// created with SLRHIP_FLAG_DYNAMIC_GEOMETRY and every scene array that depends on vertices, all updated in place.  The range has passed
// geometryUpdateRefusal2 (render_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/slrhip.h"
#include "device_types.h"
#include "pt_refit.h"

namespace slrhip {

struct GeometryUpdate {
    const float* src;                                      // the caller's records, 11 floats each (slrhip_vertex), 4-byte aligned
    uint32_t first, count;                                 // vertices [first, first + count)
    uint32_t numVertices, numTriangles, numLeafTris, numNodes, numLights, numLevels;
    float* vertices;                                       // the kept array, 11 floats per vertex
    const slrhip_triangle* triangles;                      // the kept index array
    float4* leafTris;                                      // LeafTri as 3 x float4
    float4* leafBoxes;                                     // scratch: lo, hi of each LeafTri record's triangle
    float4* shadeTris;                                     // ShadeTri as 6 x float4
    float4* lightTris;                                     // LightTri as 9 x float4
    float4* stagedLights;                                  // the lights segment of DevScene::shadeTables, nullptr when the tables are not staged
    float4* triUV;                                         // 2 x float4 per triangle, nullptr for a scene without textures
    float4* alphaTris;                                     // 2 x float4 per alpha record
    uint32_t numAlphaRecords;
    float4* nodes;                                         // QNode as 8 x float4
    float4* nodesQ;                                        // QNodeQ as 4 x float4, nullptr unless the quantized nodes are in use
    uint32_t* status;                                      // SLRHIP_GEOMETRY_* bits
    uint32_t levelFirst[kMaxTreeLevels + 1];               // first node of each level; [numLevels] = numNodes (instanced: the TOP level's; = topNodes)
    // a scene with instances (numInstances != 0): the mesh trees behind the top level, and what slrhip_set_instance_transforms and
    // slrhip_rebuild_top_level work from
    uint32_t numInstances, numMeshes, numMeshLevels, numTopPackets;
    const uint32_t* meshLevelNodes;                        // level d of every mesh tree: entries [meshLevelFirst[d], meshLevelFirst[d + 1])
    const uint32_t* meshRoots;                             // the root node of each mesh
    const float4* instances;                               // DevInstance as 9 x float4 (read only: localToWorld, rootNode, mesh)
    float4* meshBoxes;                                     // 2 x float4 per mesh: lo, hi
    float4* instBoxes;                                     // 2 x float4 per instance: lo, hi
    const uint32_t* topPacketRefs;                         // slrhip_rebuild_top_level's canonical child words of the loose packets, or nullptr: no tables yet
    float4* topPacketBoxes;                                // ... and their boxes, 2 x float4 per packet
    uint32_t meshLevelFirst[kMaxTreeLevels + 1];           // [numMeshLevels] = the number of mesh nodes
};

// The launches of one call, in order on `stream`; returns how many there were.
uint32_t launchGeometryUpdate(const GeometryUpdate& u, hipStream_t stream);

// k_geometry_lights alone: the light records (both copies) of the lights whose `tri` and `material` words stand, from the kept vertices.
// Reads u.numLights, lightTris, stagedLights, triangles, vertices, numTriangles, numVertices.  slrhip_set_materials fills a rebuilt
// light list with it.  Returns the launches (0 without lights).
uint32_t launchGeometryLights(const GeometryUpdate& u, hipStream_t stream);

} // namespace slrhip
