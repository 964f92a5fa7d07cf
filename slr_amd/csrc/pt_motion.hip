// pt_motion.hip — device code of the motion pass (slrhip_render_motion / slrhip_resolve_motion), as defined in include/slrhip.h.
// gfx950, wave64.
//
// The traversal of a motion pass is the feature pass's (launchFeatureTrace, pt_trace_indexed.hip: camera rays made on the spot, one hit record
// {triangle, instance, dist, b1} per sample).  k_motion_fold turns a window's records into motion vectors: one lane owns a pixel and
// takes its passes in pass order.  The hit point is not in the record: the fold makes the sample's camera ray again from
// (seed, pixel, pass) with the path tracer's own draws and camera arithmetic (pt_camera.h, as featureCameraRay does) and walks `dist`
// along it.  The sample itself is pt_motion.h's motionSample, the function slrhip_motion_sample calls on the host.
#include "pt_camera.h"
#include "pt_kernels.h"
#include "pt_motion.h"

namespace slrhip {

namespace {

// the records are streamed once per launch, the matrices of a pixel's instance are read again by its neighbours
typedef float mvFloat4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ntLoad4(const float4* p) {
    const mvFloat4 v = __builtin_nontemporal_load(reinterpret_cast<const mvFloat4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}

// the two matrices of a placement, 8 x float4 -> the 32 floats motionSample takes
__device__ __forceinline__ void loadTransform(const float4* src, float* m) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float4 v = src[k];
        m[4 * k] = v.x; m[4 * k + 1] = v.y; m[4 * k + 2] = v.z; m[4 * k + 3] = v.w;
    }
}

__global__ __launch_bounds__(256) void k_motion_fold(DevCamera cam, FeatureParams fp, MotionParams mp) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const uint32_t xy = fp.pixelXY[pix];
    float4 acc = mp.sums[pix];
#pragma unroll 1
    for (uint32_t p = 0; p < fp.numPasses; ++p) {
        const float4 r = ntLoad4(fp.records + (size_t)p * fp.numPixels + pix);
        if (__float_as_uint(r.x) == 0xFFFFFFFFu) continue;                 // a miss (the environment sphere included) adds nothing
        Rng rng;
        const CameraDraws draws = drawCameraSample(rng, fp.rngSeed, xy & 0xFFFFu, xy >> 16, fp.passBegin + p, fp.timeStart, fp.timeEnd);
        const CameraRay ray = sampleCameraRay(cam, fp.imageWidth, fp.imageHeight, draws);
        const float P[3] = {ray.org.x + r.z * ray.dir.x, ray.org.y + r.z * ray.dir.y, ray.org.z + r.z * ray.dir.z};
        const int32_t inst = (int32_t)__float_as_uint(r.y);
        float out[4];
        if (mp.instances && inst >= 0) {
            float recNow[32], recPrev[32];
            loadTransform(mp.instances + (size_t)inst * 9u, recNow);
            if (mp.prevTransforms) loadTransform(mp.prevTransforms + (size_t)inst * 8u, recPrev);
            motionSample(mp.now, mp.prev, recNow, mp.prevTransforms ? recPrev : nullptr, fp.imageWidth, fp.imageHeight, P, out);
        }
        else motionSample(mp.now, mp.prev, nullptr, nullptr, fp.imageWidth, fp.imageHeight, P, out);
        if (out[3] != 0.0f) { acc.x += out[0]; acc.y += out[1]; acc.z += out[2]; acc.w += 1.0f; }
    }
    mp.sums[pix] = acc;
}

// slrhip_resolve_motion: the sums scattered into a [height][width][4] image the caller has cleared (4-byte aligned: scalar stores)
__global__ __launch_bounds__(256) void k_motion_resolve(FeatureParams fp, const float4* sums, float* dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const uint32_t xy = fp.pixelXY[pix];
    const float4 v = sums[pix];
    float* o = dst + ((size_t)(xy >> 16) * fp.imageWidth + (xy & 0xFFFFu)) * 4u;
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
}

} // namespace

void launchMotionFold(const DevCamera& cam, const FeatureParams& fp, const MotionParams& mp, hipStream_t stream) {
    hipLaunchKernelGGL(k_motion_fold, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, cam, fp, mp);
}

void launchMotionResolve(const FeatureParams& fp, const float4* sums, float* dst, hipStream_t stream) {
    hipLaunchKernelGGL(k_motion_resolve, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, fp, sums, dst);
}

} // namespace slrhip
