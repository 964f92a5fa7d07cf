// pt_motion.h — the motion vector of one sample (slrhip_render_motion / slrhip_render_motion_vertices, include/slrhip.h): where on the
// PREVIOUS frame's image was the material point that this sample's camera ray hits now?  ONE definition for the host exports
// (slrhip_motion_sample, slrhip_motion_sample_vertices: host_util.cpp) and the fold kernel (k_motion_fold, pt_motion.hip).  float32 operations in the order written (both sides are built with
// -ffp-contract=off), IEEE division and square root, no other library call: host and device agree bit for bit.
//
// The point goes through pt_device.h's mulPoint, restated for both sides as instMulPoint (pt_instance.h): per row r of the column-major
// matrix, ((m[r] * p.x + m[4 + r] * p.y) + m[8 + r] * p.z) + m[12 + r] * 1.0f, and a division by w only where w != 1.
#pragma once
#include <cmath>
#include <cstdint>

#include "pt_instance.h"           // instMulPoint, SLR_HOST_DEV

namespace slrhip {

// What the projection needs of a camera: slrhip_motion_camera's 24 floats, in its order.  opWidth, opHeight and objPlaneDistance are
// prepareCamera's (scene_prep.cpp: the upload's host arithmetic), the lens centre is mulPoint(local_to_world, (0, 0, 0)).
struct MotionCamera {
    float matInv[16];              // world -> camera, column-major
    float centre[3];
    float opWidth, opHeight, objPlaneDistance;
    float pad[2];                  // 0
};
static_assert(sizeof(MotionCamera) == 24 * sizeof(float), "MotionCamera is slrhip_motion_camera's 24 floats");

SLR_HOST_DEV MotionCamera makeMotionCamera(const float* localToWorld, const float* worldToLocal, float opWidth, float opHeight, float objPlaneDistance) {
    MotionCamera c;
    for (int i = 0; i < 16; ++i) c.matInv[i] = worldToLocal[i];
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    instMulPoint(localToWorld, zero, c.centre);
    c.opWidth = opWidth; c.opHeight = opHeight; c.objPlaneDistance = objPlaneDistance;
    c.pad[0] = 0.0f; c.pad[1] = 0.0f;
    return c;
}

SLR_HOST_DEV bool motionFinite(float v) { return fabsf(v) <= 3.402823466e+38f; }       // false for a NaN

// proj(cam, Q): the inverse of sampleCameraRay (pt_camera.h) through the lens centre.  A point of the focal plane in camera space is
// (opWidth * (0.5 - X / W), opHeight * (0.5 - Y / H), objPlaneDistance); q is scaled onto that plane and the pixel solved for.
SLR_HOST_DEV bool motionProject(const MotionCamera& c, const float* Q, uint32_t width, uint32_t height, float& X, float& Y) {
    float q[3];
    instMulPoint(c.matInv, Q, q);
    if (!(q[2] > 0.0f) || !motionFinite(q[0]) || !motionFinite(q[1]) || !motionFinite(q[2])) return false;
    X = (0.5f - ((q[0] / q[2]) * c.objPlaneDistance) / c.opWidth) * (float)width;
    Y = (0.5f - ((q[1] / q[2]) * c.objPlaneDistance) / c.opHeight) * (float)height;
    return true;
}

// The tail of a sample, shared by motionSample and motionSampleVertices: the two placed points through the two projections, m and z'.
// out = {m.x, m.y, z', 1} for a valid sample, {0, 0, 0, 0} otherwise; returns the validity.
SLR_HOST_DEV bool motionTail(const MotionCamera& now, const MotionCamera& prev, uint32_t width, uint32_t height, const float* pNow, const float* pPrev,
                             float* out) {
    float xNow = 0.0f, yNow = 0.0f, xPrev = 0.0f, yPrev = 0.0f;
    const bool okNow = motionProject(now, pNow, width, height, xNow, yNow);
    const bool okPrev = motionProject(prev, pPrev, width, height, xPrev, yPrev);
    if (!(okNow && okPrev)) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = 0.0f; return false; }
    const float dx = pPrev[0] - prev.centre[0], dy = pPrev[1] - prev.centre[1], dz = pPrev[2] - prev.centre[2];
    out[0] = xPrev - xNow;
    out[1] = yPrev - yNow;
    out[2] = sqrtf(dx * dx + dy * dy + dz * dz);           // pt_device.h's length: (xx + yy) + zz
    out[3] = 1.0f;
    return true;
}

// One sample.  P: the hit point now, org + dist * dir.  recNow / recPrev: the 32 floats of a slrhip_instance_transform (local_to_world,
// then world_to_local) of the instance that was hit, now and in the previous frame; recNow == nullptr: a loose triangle, which does not
// move (recPrev is not read); recPrev == nullptr with recNow given: the instance did not move (recPrev = recNow).  Both placements go
// through the same arithmetic, so records that are bit-equal give points that are bit-equal, and with equal cameras m is exactly 0.
// out = {m.x, m.y, z', 1} for a valid sample, {0, 0, 0, 0} otherwise; returns the validity.
SLR_HOST_DEV bool motionSample(const MotionCamera& now, const MotionCamera& prev, const float* recNow, const float* recPrev, uint32_t width,
                               uint32_t height, const float* P, float* out) {
    float l[3] = {P[0], P[1], P[2]}, pNow[3], pPrev[3];
    if (recNow) {
        instMulPoint(recNow + 16, P, l);
        instMulPoint(recNow, l, pNow);
        instMulPoint(recPrev ? recPrev : recNow, l, pPrev);
    }
    else for (int a = 0; a < 3; ++a) { pNow[a] = l[a]; pPrev[a] = l[a]; }
    return motionTail(now, prev, width, height, pNow, pPrev, out);
}

// One sample of slrhip_render_motion_vertices: the vertices moved as well.  posNow / posPrev: the positions of the hit triangle's three
// vertices (x, y, z of the first, the second, the third) in the mesh's local space, now and in the previous frame; b1, b2: Moller-
// Trumbore's barycentrics of the hit (b1 on the second vertex, b2 on the third).  The local point of each frame is the same expression
// on its own positions, (b0 p0 + b1 p1) + b2 p2 with b0 = (1 - b1) - b2, so positions that are bit-equal give points that are bit-equal;
// the camera ray is not used.  recNow / recPrev and out as for motionSample; only local_to_world is read of a record.
SLR_HOST_DEV bool motionSampleVertices(const MotionCamera& now, const MotionCamera& prev, const float* recNow, const float* recPrev, uint32_t width,
                                       uint32_t height, const float* posNow, const float* posPrev, float b1, float b2, float* out) {
    const float b0 = (1.0f - b1) - b2;
    float lNow[3], lPrev[3], pNow[3], pPrev[3];
    for (int a = 0; a < 3; ++a) {
        lNow[a] = (b0 * posNow[a] + b1 * posNow[3 + a]) + b2 * posNow[6 + a];
        lPrev[a] = (b0 * posPrev[a] + b1 * posPrev[3 + a]) + b2 * posPrev[6 + a];
    }
    if (recNow) {
        instMulPoint(recNow, lNow, pNow);
        instMulPoint(recPrev ? recPrev : recNow, lPrev, pPrev);
    }
    else for (int a = 0; a < 3; ++a) { pNow[a] = lNow[a]; pPrev[a] = lPrev[a]; }
    return motionTail(now, prev, width, height, pNow, pPrev, out);
}

#ifdef __HIP__
struct FeatureParams;
struct DevCamera;
// slrhip_render_motion's fold (pt_motion.hip): the window's records -> per pixel {sum m.x, sum m.y, sum z', valid samples}.
struct MotionParams {
    MotionCamera now, prev;
    const float4* instances;       // DevInstance as 9 x float4, or nullptr: the scene has no instanced mesh
    const float4* prevTransforms;  // the caller's previous frame, 8 x float4 per instance, or nullptr: no instance moved
    float4* sums;                  // one per pixel of the shard
    // slrhip_render_motion_vertices (prevVertices given; fp.b2 is then the window's second barycentrics): the kept arrays of
    // slrhip_set_vertices and the caller's previous frame, slrhip_vertex records of 11 floats
    const float* vertices;
    const uint4* triangles;        // slrhip_triangle: v[3], material
    const float* prevVertices;     // or nullptr: no vertex moved (the fold of slrhip_render_motion)
    uint32_t numVertices, numTriangles;
};
// mp.prevVertices == nullptr: k_motion_fold<false>, slrhip_render_motion's fold; else k_motion_fold<true>
void launchMotionFold(const DevCamera& cam, const FeatureParams& fp, const MotionParams& mp, hipStream_t stream);
// the sums as [height][width][4] (dst cleared by the caller: pixels outside the shard stay 0)
void launchMotionResolve(const FeatureParams& fp, const float4* sums, float* dst, hipStream_t stream);
#endif

} // namespace slrhip
