// pt_camera.h — the camera half of Job::kernel (Renderers/PathTracingRenderer.cpp:100-120) as device functions: the sample's
// draws and PerspectiveCamera::sample + PerspectiveIDF::sample (Cameras/PerspectiveCamera.cpp:33-74).  One statement of the
// reference's arithmetic, used by the path tracer's startSample (pt_sample_start.h), by the producer waves of the feature trace
// and the primary pass (pt_trace_indexed.hip) and by slrhip_camera_rays (k_camera_rays, pt_features.hip).
#pragma once
#include "pt_device.h"
#include "pt_kernels.h"

namespace slrhip {

// What Job::kernel draws before the camera is sampled, in source (left-to-right) order: time, pixel x, pixel y, wavelength
// offset, wavelength selection, two lens draws.  The stream is left where the path's first bounce goes on.
struct CameraDraws {
    float px, py;               // p.x, p.y: the jittered position on the image, in pixels
    float wlOffset, uLambda;    // WavelengthSamples::createWithEqualOffsets (RGBTypes.h:37-45 / SpectrumTypes.h:54-64)
    float lu0, lu1;             // LensPosSample
};
SLR_DEV CameraDraws drawCameraSample(Rng& rng, int32_t rngSeed, uint32_t px, uint32_t py, uint32_t pass, float timeStart, float timeEnd) {
    rng.seed(sampleSeed(rngSeed, px, py, pass));
    float v = rng.nextFloat();
    float time = timeStart * (1 - v) + timeEnd * v;
    (void)time;
    CameraDraws d;
    d.px = px + rng.nextFloat();
    d.py = py + rng.nextFloat();
    d.wlOffset = rng.nextFloat();
    d.uLambda = rng.nextFloat();
    d.lu0 = rng.nextFloat();
    d.lu1 = rng.nextFloat();
    return d;
}

// The same draws from the stream drawCameraSample leaves behind.  xorshift128's state IS its last four outputs, so the state
// after the seven draws is (o4, o5, o6, o7): the raw words of wlOffset, uLambda, lu0 and lu1.  The two draws before them run the
// recurrence backwards: o_n = A(o_{n-1}) ^ B(o_{n-4}) with A(x) = x ^ (x >> 19) and B(x) = t ^ (t >> 8), t = x ^ (x << 11), so
// B(o3) = o7 ^ A(o6) and B(o2) = o6 ^ A(o5), and both halves of B are xorshifts with closed inverses.  The time draw (o1) is not
// used by the camera.  Integer operations and nextFloat's own conversion: the draws are the forward ones bit for bit.
SLR_DEV uint32_t xorshiftStepBack(uint32_t newer, uint32_t older) {
    const uint32_t y = newer ^ (older ^ (older >> 19));         // B(x)
    const uint32_t t = y ^ (y >> 8) ^ (y >> 16) ^ (y >> 24);    // x ^ (x << 11)
    return t ^ (t << 11) ^ (t << 22);                           // x
}
SLR_DEV CameraDraws recoverCameraDraws(const Rng& after, uint32_t px, uint32_t py) {
    CameraDraws d;
    d.px = px + Rng::toFloat(xorshiftStepBack(after.s2, after.s1));
    d.py = py + Rng::toFloat(xorshiftStepBack(after.s3, after.s2));
    d.wlOffset = Rng::toFloat(after.s0);
    d.uLambda = Rng::toFloat(after.s1);
    d.lu0 = Rng::toFloat(after.s2);
    d.lu1 = Rng::toFloat(after.s3);
    return d;
}

struct CameraRay {
    V3 org, dir;                // world space; the ray is Ray(org, dir, time) with distMin 0 and distMax INFINITY
    V3 lensN;                   // the lens surface's normal in world space
    float dirLocalZ;            // z of the direction in camera space (PerspectiveIDF's dirPDF needs it)
};
// PerspectiveCamera::sample (PerspectiveCamera.cpp:33-57), then PerspectiveIDF::sample (:63-74) with IDFSample(p.x / W, p.y / H)
SLR_DEV CameraRay sampleCameraRay(const DevCamera& cam, uint32_t imageWidth, uint32_t imageHeight, const CameraDraws& d) {
    float lx, ly;
    concentricSampleDisk(d.lu0, d.lu1, &lx, &ly);
    V3 orgLocal(cam.lensRadius * lx, cam.lensRadius * ly, 0.0f);
    CameraRay r;
    r.org = mulPoint(cam.mat, orgLocal);
    r.lensN = mulNormal(cam.matInv, V3(0, 0, 1));
    Frame lf;
    lf.z = r.lensN;
    lf.x = mulVector(cam.mat, V3(1, 0, 0));
    lf.y = cross(lf.z, lf.x);
    float sx = d.px / (float)imageWidth;
    float sy = d.py / (float)imageHeight;
    V3 pFocus(cam.opWidth * (0.5f - sx), cam.opHeight * (0.5f - sy), cam.objPlaneDistance);
    V3 dirLocal = normalize(pFocus - orgLocal);
    r.dirLocalZ = dirLocal.z;
    r.dir = lf.fromLocal(dirLocal);
    return r;
}

// The camera ray of (pixel of the shard, pass of the launch) as a ring entry or a slrhip_ray: {org, distMin 0}, {dir, distMax inf}
// `rng`: the stream as the draws leave it, where the path's first bounce goes on
SLR_DEV void cameraRayOf(const DevCamera& cam, const FeatureParams& fp, uint32_t pix, uint32_t pass, float4& o, float4& d, uint32_t& xy, Rng& rng) {
    xy = fp.pixelXY[pix];
    const CameraDraws draws = drawCameraSample(rng, fp.rngSeed, xy & 0xFFFFu, xy >> 16, fp.passBegin + pass, fp.timeStart, fp.timeEnd);
    const CameraRay r = sampleCameraRay(cam, fp.imageWidth, fp.imageHeight, draws);
    o = make_float4(r.org.x, r.org.y, r.org.z, 0.0f);
    d = make_float4(r.dir.x, r.dir.y, r.dir.z, INFINITY);
}
// the feature passes' numbering: the pixel fastest (their record windows are pass-major, writer and reader alike)
SLR_DEV void featureCameraRay(const DevCamera& cam, const FeatureParams& fp, uint32_t index, float4& o, float4& d, uint32_t& xy) {
    const uint32_t pass = index / fp.numPixels, pix = index - pass * fp.numPixels;
    Rng rng;
    cameraRayOf(cam, fp, pix, pass, o, d, xy, rng);
}
// the primary pass's numbering: the pass fastest (the result window's own order, windowEntry)
SLR_DEV void primaryCameraRay(const DevCamera& cam, const FeatureParams& fp, uint32_t index, float4& o, float4& d, uint32_t& xy, Rng& rng) {
    const uint32_t pix = index / fp.numPasses, pass = index - pix * fp.numPasses;
    cameraRayOf(cam, fp, pix, pass, o, d, xy, rng);
}

} // namespace slrhip
