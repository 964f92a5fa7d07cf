// pt_motion.hip — device code of the motion pass (slrhip_render_motion / slrhip_render_motion_vertices / slrhip_resolve_motion), as
// defined in include/slrhip.h.  gfx950, wave64.
//
// The traversal of a motion pass is the feature pass's (launchFeatureTrace, pt_trace_indexed.hip: camera rays made on the spot, one hit record
// {triangle, instance, dist, b1} per sample).  k_motion_fold turns a window's records into motion vectors: one lane owns a pixel and
// takes its passes in pass order.  The hit point is not in the record: the fold makes the sample's camera ray again from
// (seed, pixel, pass) with the path tracer's own draws and camera arithmetic (pt_camera.h, as featureCameraRay does) and walks `dist`
// along it.  The sample itself is pt_motion.h's motionSample, the function slrhip_motion_sample calls on the host.
//
// Where the vertices moved as well (slrhip_render_motion_vertices) the window also holds Moller-Trumbore's b2, and k_motion_fold<true>
// takes the hit point from the hit triangle instead: the index triple from the context's kept index array, the three positions from the
// kept vertex array as it now stands and from the caller's previous frame, weighted by the record's barycentrics (motionSampleVertices,
// the function slrhip_motion_sample_vertices calls on the host).  No camera ray is made on that path.  Per sample: one 16 B record and
// one 4 B b2, streamed; one 16 B index record and six 12 B positions at 44 B stride, gathered and left to the cache.
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

// a placement's local_to_world alone, 4 x float4 -> the 16 floats motionSampleVertices reads
__device__ __forceinline__ void loadMatrix(const float4* src, float* m) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float4 v = src[k];
        m[4 * k] = v.x; m[4 * k + 1] = v.y; m[4 * k + 2] = v.z; m[4 * k + 3] = v.w;
    }
}

// the position of vertex i of an array of slrhip_vertex records (11 floats, 4-byte aligned): three consecutive floats, left to the
// cache (a pixel's neighbours hit the same or adjacent triangles)
__device__ __forceinline__ void loadPosition(const float* vertices, uint32_t i, float* p) {
    const float* v = vertices + (size_t)i * 11u;
    p[0] = v[0]; p[1] = v[1]; p[2] = v[2];
}

// VERTS == false: slrhip_render_motion's fold.  VERTS == true: slrhip_render_motion_vertices' — the hit point comes from the hit
// triangle's vertices now and in the previous frame and the record's barycentrics (motionSampleVertices), not from the camera ray.
template <bool VERTS>
__global__ __launch_bounds__(256) void k_motion_fold(DevCamera cam, FeatureParams fp, MotionParams mp) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const uint32_t xy = fp.pixelXY[pix];
    float4 acc = mp.sums[pix];
#pragma unroll 1
    for (uint32_t p = 0; p < fp.numPasses; ++p) {
        const float4 r = ntLoad4(fp.records + (size_t)p * fp.numPixels + pix);
        if (__float_as_uint(r.x) == 0xFFFFFFFFu) continue;                 // a miss (the environment sphere included) adds nothing
        const int32_t inst = (int32_t)__float_as_uint(r.y);
        float out[4];
        if constexpr (VERTS) {
            const float b2 = __builtin_nontemporal_load(fp.b2 + (size_t)p * fp.numPixels + pix);
            const uint32_t tri = __float_as_uint(r.x);
            if (tri >= mp.numTriangles) continue;                          // never: the record names a triangle of the kept array
            const uint4 t = mp.triangles[tri];
            if (t.x >= mp.numVertices || t.y >= mp.numVertices || t.z >= mp.numVertices) continue;      // never: the upload checked them
            float posNow[9], posPrev[9];
            loadPosition(mp.vertices, t.x, posNow); loadPosition(mp.vertices, t.y, posNow + 3); loadPosition(mp.vertices, t.z, posNow + 6);
            loadPosition(mp.prevVertices, t.x, posPrev); loadPosition(mp.prevVertices, t.y, posPrev + 3); loadPosition(mp.prevVertices, t.z, posPrev + 6);
            if (mp.instances && inst >= 0) {
                // only local_to_world is read of a placement: the first four float4 of a record
                float recNow[16], recPrev[16];
                loadMatrix(mp.instances + (size_t)inst * 9u, recNow);
                // no previous placements: the current record again (an address is chosen, not a register array: no scratch)
                loadMatrix(mp.prevTransforms ? mp.prevTransforms + (size_t)inst * 8u : mp.instances + (size_t)inst * 9u, recPrev);
                motionSampleVertices(mp.now, mp.prev, recNow, recPrev, fp.imageWidth, fp.imageHeight, posNow, posPrev, r.w, b2, out);
            }
            else motionSampleVertices(mp.now, mp.prev, nullptr, nullptr, fp.imageWidth, fp.imageHeight, posNow, posPrev, r.w, b2, out);
        }
        else {
            Rng rng;
            const CameraDraws draws = drawCameraSample(rng, fp.rngSeed, xy & 0xFFFFu, xy >> 16, fp.passBegin + p, fp.timeStart, fp.timeEnd);
            const CameraRay ray = sampleCameraRay(cam, fp.imageWidth, fp.imageHeight, draws);
            const float P[3] = {ray.org.x + r.z * ray.dir.x, ray.org.y + r.z * ray.dir.y, ray.org.z + r.z * ray.dir.z};
            if (mp.instances && inst >= 0) {
                float recNow[32], recPrev[32];
                loadTransform(mp.instances + (size_t)inst * 9u, recNow);
                if (mp.prevTransforms) loadTransform(mp.prevTransforms + (size_t)inst * 8u, recPrev);
                motionSample(mp.now, mp.prev, recNow, mp.prevTransforms ? recPrev : nullptr, fp.imageWidth, fp.imageHeight, P, out);
            }
            else motionSample(mp.now, mp.prev, nullptr, nullptr, fp.imageWidth, fp.imageHeight, P, out);
        }
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
    const dim3 grid((fp.numPixels + 255u) / 256u);
    if (mp.prevVertices) hipLaunchKernelGGL(k_motion_fold<true>, grid, dim3(256), 0, stream, cam, fp, mp);
    else hipLaunchKernelGGL(k_motion_fold<false>, grid, dim3(256), 0, stream, cam, fp, mp);
}

void launchMotionResolve(const FeatureParams& fp, const float4* sums, float* dst, hipStream_t stream) {
    hipLaunchKernelGGL(k_motion_resolve, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, fp, sums, dst);
}

} // namespace slrhip
