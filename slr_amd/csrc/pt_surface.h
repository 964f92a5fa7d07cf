// pt_surface.h — the surface point of a triangle hit as device functions: Triangle::getSurfacePoint (Surface/TriangleMesh.cpp:
// 180-215), BumpSingleSurfaceObject::getSurfacePoint (Core/SurfaceObject.cpp:123-134) and TransformedSurfaceObject::
// getSurfacePoint (:329-336).  One statement of the reference's arithmetic, used by the path tracer (logicSlot,
// pt_shade_visit.h) and by the feature pass (k_feature_fold, pt_features.hip).
#pragma once
#include "pt_device.h"
#include "pt_tex.h"

namespace slrhip {

struct SurfPt {       // Core/geometry.h:239-258 (fields the path uses)
    V3 p;
    V3 gNormal;
    Frame frame;
    uint32_t material;
    int32_t light;
    float areaPDF;
};

// The shading frame of Triangle::getSurfacePoint (TriangleMesh.cpp:190-213) from the triangle's shading record (ShadeTri as six
// float4: three normals, three tangents) and the hit record's Moller-Trumbore barycentrics (b1, b2).  Intersection::u = b0 =
// 1 - b1 - b2 as Triangle::intersect computes it (:159), and getSurfacePoint re-derives ITS b2 from (u, v) (:190-191).
SLR_DEV Frame triangleShadingFrame(float4 q0, float4 q1, float4 q2, float4 q3, float4 q4, float4 q5, float b1, float b2hit) {
    const float b0 = 1.0f - b1 - b2hit;
    const float b2 = 1.0f - b0 - b1;
    Frame f;
    f.z = normalize(b0 * xyz(q0) + b1 * xyz(q1) + b2 * xyz(q2));
    f.x = normalize(b0 * xyz(q3) + b1 * xyz(q4) + b2 * xyz(q5));
    const float dotNT = dot(f.z, f.x);
    if (fabsf(dotNT) >= 0.01f) f.x = normalize(f.x - dotNT * f.z);
    f.y = cross(f.z, f.x);
    return f;
}

// BumpSingleSurfaceObject::getSurfacePoint, Core/SurfaceObject.cpp:123-134: the frame tilted by the material's normal map
// (a CheckerBoardNormal3DTexture) at the hit's texture coordinate
SLR_DEV void bumpShadingFrame(const DevTexture* textures, uint32_t normalMap, float texU, float texV, Frame& frame) {
    const DevTexture nt = loadTexture(textures, normalMap);
    float uc, vc;
    checkerNormalComponents(nt, texU, texV, &uc, &vc);
    const V3 nLocal = normalize(V3(uc, vc, 1.0f));
    const V3 tLocal = V3(1.0f, 0.0f, 0.0f) - dot(nLocal, V3(1.0f, 0.0f, 0.0f)) * nLocal;
    const V3 bLocal = V3(0.0f, 1.0f, 0.0f) - dot(nLocal, V3(0.0f, 1.0f, 0.0f)) * nLocal;
    const V3 tt = normalize(frame.fromLocal(tLocal));
    const V3 bb = normalize(frame.fromLocal(bLocal));
    const V3 nn = normalize(frame.fromLocal(nLocal));
    frame.x = tt; frame.y = bb; frame.z = nn;
}

// *surfPt = sampledTF * *surfPt (SurfaceObject.cpp:329-336; SurfacePoint x StaticTransform, geometry.cpp:63-78): p as a point,
// the geometric normal through the inverse transpose (Transform.h:47-52), the frame's axes as vectors, re-normalised.
// instMats: DevInstance::localToWorld, then worldToLocal at + 16.
SLR_DEV V3 instanceNormalToWorld(const float* instMats, V3 n) { return normalize(mulNormal(instMats + 16, n)); }
SLR_DEV V3 instanceAxisToWorld(const float* instMats, V3 v) { return normalize(mulVector(instMats, v)); }
SLR_DEV void instanceSurfaceToWorld(const float* instMats, SurfPt& surf) {
    surf.p = mulPoint(instMats, surf.p);
    surf.gNormal = instanceNormalToWorld(instMats, surf.gNormal);
    surf.frame.x = instanceAxisToWorld(instMats, surf.frame.x);
    surf.frame.y = instanceAxisToWorld(instMats, surf.frame.y);
    surf.frame.z = instanceAxisToWorld(instMats, surf.frame.z);
}

} // namespace slrhip
