// pt_features.hip — the feature buffers' kernels that are not traversal (slrhip_render_features, slrhip_resolve_features,
// slrhip_camera_rays): the fold of a window's hit records into the per-pixel sums, the read-out of a channel, and the camera rays of
// a pass in the public format.  The records come from launchFeatureTrace (pt_trace_indexed.hip, WsFeatureIO).
#include <hip/hip_runtime.h>

#include "pt_camera.h"
#include "pt_surface.h"
#include "pt_trace_ws.h"          // ntLoad4

namespace slrhip {

// The accumulation of a window's records: one lane owns a pixel and takes its passes in pass order — the surface point of the hit
// (pt_surface.h: the triangle's frame, the bump map, the instance transform, as logicSlot does) for the vector channels asked for,
// then plain float32 adds; a miss (the environment sphere included) adds nothing.  idsPass: the pass of the window whose ids
// become the pixel's (the highest pass rendered so far), or 0xFFFFFFFF to leave them.
__global__ __launch_bounds__(256) void k_feature_fold(DevScene sc, FeatureParams fp, FeatureSums sums, uint32_t idsPass) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const bool gn = (fp.channels & SLRHIP_FEATURE_GEOMETRIC_NORMAL) != 0, sn = (fp.channels & SLRHIP_FEATURE_SHADING_NORMAL) != 0,
               tn = (fp.channels & SLRHIP_FEATURE_SHADING_TANGENT) != 0;
    float4 g = sums.geometric[pix], s = sums.shading[pix], t = sums.tangent[pix];      // .w: distance, coverage, unused
    for (uint32_t p = 0; p < fp.numPasses; ++p) {
        const size_t e = (size_t)p * fp.numPixels + pix;
        const float4 r = ntLoad4(fp.records + e);
        const uint32_t tri = __float_as_uint(r.x);
        const bool hit = tri != 0xFFFFFFFFu;
        const float4* st = reinterpret_cast<const float4*>(sc.shadeTris) + (size_t)(hit ? tri : 0u) * 6;
        if (p == idsPass) sums.ids[pix] = make_uint4(tri, hit ? __float_as_uint(r.y) : 0xFFFFFFFFu, hit ? reinterpret_cast<const uint32_t*>(st)[3] : 0xFFFFFFFFu, 0u);
        if (!hit) continue;
        g.w += r.z;
        s.w += 1.0f;
        if (!(gn || sn || tn)) continue;
        const float4 q0 = st[0], q1 = st[1], q2 = st[2], q3 = st[3], q4 = st[4], q5 = st[5];
        const int32_t inst = (int32_t)__float_as_uint(r.y);
        const float* instMats = sc.instances && inst >= 0 ? reinterpret_cast<const float*>(sc.instances + (size_t)inst * 9u) : nullptr;
        if (gn) {
            V3 n(q3.w, q4.w, q5.w);
            if (instMats) n = instanceNormalToWorld(instMats, n);
            g.x += n.x; g.y += n.y; g.z += n.z;
        }
        if (sn || tn) {
            const float b1 = r.w, b2 = __builtin_nontemporal_load(fp.b2 + e);
            Frame frame = triangleShadingFrame(q0, q1, q2, q3, q4, q5, b1, b2);
            if (sc.numTextures) {
                const int32_t normalMap = sc.matTex[__float_as_uint(q0.w)].normalMap;
                if (normalMap >= 0) {
                    // texCoord from the original barycentrics (TriangleMesh.cpp:160-161)
                    const float4 uvA = sc.triUV[(size_t)tri * 2], uvB = sc.triUV[(size_t)tri * 2 + 1];
                    float texU, texV;
                    hitTexCoord(uvA, uvB, b1, b2, &texU, &texV);
                    bumpShadingFrame(sc.textures, (uint32_t)normalMap, texU, texV, frame);
                }
            }
            if (instMats) { frame.x = instanceAxisToWorld(instMats, frame.x); frame.z = instanceAxisToWorld(instMats, frame.z); }
            if (sn) { s.x += frame.z.x; s.y += frame.z.y; s.z += frame.z.z; }
            if (tn) { t.x += frame.x.x; t.y += frame.x.y; t.z += frame.x.z; }
        }
    }
    sums.geometric[pix] = g; sums.shading[pix] = s; sums.tangent[pix] = t;
}

void launchFeatures(const DevScene& sc, const FeatureParams& fp, const FeatureSums& sums, uint32_t idsPass, int numCUs, hipStream_t stream) {
    launchFeatureTrace(sc, fp, numCUs, stream);
    hipLaunchKernelGGL(k_feature_fold, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, sc, fp, sums, idsPass);
}

// slrhip_camera_rays: the feature trace's producer half alone, written out in the public slrhip_ray format; one lane per pixel of the shard
__global__ __launch_bounds__(256) void k_camera_rays(DevCamera cam, FeatureParams fp, float4* rays, uint32_t* pixelXY) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    float4 o, d;
    uint32_t xy;
    featureCameraRay(cam, fp, pix, o, d, xy);
    rays[2 * (size_t)pix] = o;
    rays[2 * (size_t)pix + 1] = d;
    if (pixelXY) pixelXY[pix] = xy;
}
void launchCameraRays(const DevScene& sc, const FeatureParams& fp, float4* rays, uint32_t* pixelXY, hipStream_t stream) {
    hipLaunchKernelGGL(k_camera_rays, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, sc.camera, fp, rays, pixelXY);
}

// slrhip_debug_camera_draws: drawCameraSample forward and recoverCameraDraws from the stream it leaves, one lane per tuple
// (seed, x, y, pass); out: 16 words a tuple — the six forward draws, the stream, the six recovered draws
__global__ __launch_bounds__(256) void k_camera_draws(uint32_t n, const uint4* tuples, uint32_t* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint4 t = tuples[i];
    Rng rng;
    const CameraDraws f = drawCameraSample(rng, (int32_t)t.x, t.y, t.z, t.w, 0.0f, 0.0f);
    const CameraDraws r = recoverCameraDraws(rng, t.y, t.z);
    const uint32_t words[16] = {__float_as_uint(f.px), __float_as_uint(f.py), __float_as_uint(f.wlOffset), __float_as_uint(f.uLambda),
                                __float_as_uint(f.lu0), __float_as_uint(f.lu1), rng.s0, rng.s1, rng.s2, rng.s3,
                                __float_as_uint(r.px), __float_as_uint(r.py), __float_as_uint(r.wlOffset), __float_as_uint(r.uLambda),
                                __float_as_uint(r.lu0), __float_as_uint(r.lu1)};
#pragma unroll
    for (int k = 0; k < 16; ++k) out[(size_t)i * 16 + k] = words[k];
}
void launchCameraDraws(uint32_t n, const uint4* tuples, uint32_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(k_camera_draws, dim3((n + 255u) / 256u), dim3(256), 0, stream, n, tuples, out);
}

// slrhip_resolve_features: one channel scattered into a [height][width][k] image the caller has filled with the value of
// "outside the shard"; channel = one SLRHIP_FEATURE_* bit
__global__ __launch_bounds__(256) void k_feature_resolve(FeatureParams fp, FeatureSums sums, uint32_t channel, uint32_t* dst) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= fp.numPixels) return;
    const uint32_t xy = fp.pixelXY[pix];
    const size_t at = (size_t)(xy >> 16) * fp.imageWidth + (xy & 0xFFFFu);
    if (channel == SLRHIP_FEATURE_IDS) { const uint4 v = sums.ids[pix]; dst[3 * at] = v.x; dst[3 * at + 1] = v.y; dst[3 * at + 2] = v.z; }
    else if (channel == SLRHIP_FEATURE_DISTANCE) dst[at] = __float_as_uint(sums.geometric[pix].w);
    else if (channel == SLRHIP_FEATURE_COVERAGE) dst[at] = __float_as_uint(sums.shading[pix].w);
    else {
        const float4 v = channel == SLRHIP_FEATURE_GEOMETRIC_NORMAL ? sums.geometric[pix] : channel == SLRHIP_FEATURE_SHADING_NORMAL ? sums.shading[pix] : sums.tangent[pix];
        dst[3 * at] = __float_as_uint(v.x); dst[3 * at + 1] = __float_as_uint(v.y); dst[3 * at + 2] = __float_as_uint(v.z);
    }
}
void launchFeatureResolve(const FeatureParams& fp, const FeatureSums& sums, uint32_t channel, void* dst, hipStream_t stream) {
    hipLaunchKernelGGL(k_feature_resolve, dim3((fp.numPixels + 255u) / 256u), dim3(256), 0, stream, fp, sums, channel, static_cast<uint32_t*>(dst));
}

} // namespace slrhip
