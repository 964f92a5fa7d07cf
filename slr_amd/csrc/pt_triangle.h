// pt_triangle.h — the per-triangle records derived from three vertices: LeafTri (v0, e1, e2), ShadeTri (normals, tangents, face normal,
// 1 / area), LightTri, the texture-coordinate pair of triUV and of the alpha records, and a triangle's box.  ONE definition for the
// host (slrhip_upload_scene: scene_prep.cpp, bvh.cpp), the device build (bvh_device.hip: k_leaf_tris, k_shade_tris) and
// slrhip_set_vertices (pt_geometry.hip).  float32 operations in the order written (every side is built with -ffp-contract=off; divide
// and square root are correctly rounded on both), so host and device agree bit for bit — the NaN normal of a degenerate triangle
// included.  Each function writes only the words that depend on vertices; the index words of a record are its caller's.
#pragma once
#ifdef __HIP__
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>

#include "../../include/slrhip.h"
#include "device_types.h"
#include "pt_luminance.h"          // SLR_HOST_DEV

namespace slrhip {

// v0, e1 = v1 - v0, e2 = v2 - v0: the two subtractions Triangle::intersect does first (TriangleMesh.cpp:136-137)
SLR_HOST_DEV void leafTriEdges(const float* p0, const float* p1, const float* p2, LeafTri& lt) {
    for (int a = 0; a < 3; ++a) {
        lt.v0[a] = p0[a];
        lt.e1[a] = p1[a] - p0[a];      // edge01
        lt.e2[a] = p2[a] - p0[a];      // edge02
    }
}

// The exact box of a triangle: min / max over its vertex positions (never over v0 + e1, which rounds).
SLR_HOST_DEV void triangleBox(const float* p0, const float* p1, const float* p2, float* lo, float* hi) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(fminf(p0[a], p1[a]), p2[a]);
        hi[a] = fmaxf(fmaxf(p0[a], p1[a]), p2[a]);
    }
}

// Triangle::getSurfacePoint's inputs (TriangleMesh.cpp:180-215): everything of a ShadeTri but `material` and `light`.
SLR_HOST_DEV void shadeTriGeometry(const slrhip_vertex& v0, const slrhip_vertex& v1, const slrhip_vertex& v2, ShadeTri& s) {
    float e1[3], e2[3];
    for (int a = 0; a < 3; ++a) {
        s.n0[a] = v0.normal[a]; s.n1[a] = v1.normal[a]; s.n2[a] = v2.normal[a];
        s.t0[a] = v0.tangent[a]; s.t1[a] = v1.tangent[a]; s.t2[a] = v2.tangent[a];
        e1[a] = v1.position[a] - v0.position[a];
        e2[a] = v2.position[a] - v0.position[a];
    }
    // normalize(cross(edge01, edge02)) TriangleMesh.cpp:171 — same float ops as the reference
    const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const float len = sqrtf(cx * cx + cy * cy + cz * cz);
    const float r = 1.0f / len;
    s.gnx = cx * r; s.gny = cy * r; s.gnz = cz * r;
    s.areaPDF = 1.0f / (0.5f * len);                    // 1 / Triangle::area() :217-222
}

// What Triangle::sample needs (TriangleMesh.cpp:224-255): everything of a LightTri but `tri`, `material` and the pad words; `s` is the
// triangle's ShadeTri.
SLR_HOST_DEV void lightTriGeometry(const slrhip_vertex& v0, const slrhip_vertex& v1, const slrhip_vertex& v2, const ShadeTri& s, LightTri& l) {
    for (int a = 0; a < 3; ++a) {
        l.p0[a] = v0.position[a]; l.p1[a] = v1.position[a]; l.p2[a] = v2.position[a];
        l.n0[a] = v0.normal[a]; l.n1[a] = v1.normal[a]; l.n2[a] = v2.normal[a];
        l.t0[a] = v0.tangent[a]; l.t1[a] = v1.tangent[a]; l.t2[a] = v2.tangent[a];
    }
    l.areaPDF = s.areaPDF;
    l.gnx = s.gnx; l.gny = s.gny; l.gnz = s.gnz;
}

// (u0, v0, u1, v1), (u2, v2, ., .) of one triangle: the layout of DevScene::triUV and of the alpha records.  out[0 .. 5]; the last two
// words of the pair are the caller's (0, 0 in triUV; the texture index, 0 in an alpha record).
SLR_HOST_DEV void triangleTexcoords(const slrhip_vertex& v0, const slrhip_vertex& v1, const slrhip_vertex& v2, float* out) {
    out[0] = v0.texcoord[0]; out[1] = v0.texcoord[1]; out[2] = v1.texcoord[0]; out[3] = v1.texcoord[1];
    out[4] = v2.texcoord[0]; out[5] = v2.texcoord[1];
}

} // namespace slrhip
