// pt_quantize.h — the device quantizer of one node: QNode -> QNodeQ.  ONE definition for the device build (bvh_device.hip,
// k_collapse_emit) and slrhip_set_vertices (pt_geometry.hip, k_geometry_quantize).  It restates quantizeNodes of bvh.cpp statement for
// statement with the device's own fma as the check (rounded outwards: every dequantized box contains the float box); the tests hold the
// two equal bit for bit (test_device_quantizer_equals_the_host_quantizer).
#pragma once
#include <hip/hip_runtime.h>

#include "device_types.h"

namespace slrhip {

// what the traversal kernel computes for a quantized plane
__device__ __forceinline__ float dequantDev(uint32_t q, float scale, float origin) { return __builtin_fmaf((float)q, scale, origin); }

__device__ __forceinline__ QNodeQ quantizeNode(const QNode& qn) {
    QNodeQ d;
    const float* mins[3] = {qn.minx, qn.miny, qn.minz};
    const float* maxs[3] = {qn.maxx, qn.maxy, qn.maxz};
    float org[3], scl[3];
    uint32_t qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        float bmin = INFINITY, bmax = -INFINITY;
        for (int c = 0; c < 4; ++c)
            if (qn.child[c] != kInvalidChild) { bmin = fminf(bmin, mins[a][c]); bmax = fmaxf(bmax, maxs[a][c]); }
        if (!(bmin <= bmax)) { bmin = 0.0f; bmax = 0.0f; }
        org[a] = bmin;
        // quantScale of bvh.cpp, statement for statement: a box with bmax > bmin never gets scale 0 (a subnormal extent whose division
        // rounds to 0 starts at the smallest subnormal), and the same bound on the loop
        float sc = (bmax - bmin) / 255.0f;
        if (sc == 0.0f && bmax > bmin) sc = __uint_as_float(1u);
        for (int guard = 0; guard < 64 && sc > 0.0f && dequantDev(255, sc, bmin) < bmax; ++guard) sc = __uint_as_float(__float_as_uint(sc) + 1u);      // nextafter upwards (sc > 0)
        scl[a] = sc;
        for (int c = 0; c < 4; ++c) {
            uint32_t l = 255, h = 0;                       // empty slot: inverted, never entered
            if (qn.child[c] != kInvalidChild) {
                if (sc > 0.0f) {
                    l = (uint32_t)fminf(255.0f, fmaxf(0.0f, floorf((mins[a][c] - bmin) / sc)));
                    h = (uint32_t)fminf(255.0f, fmaxf(0.0f, ceilf((maxs[a][c] - bmin) / sc)));
                    while (l > 0 && dequantDev(l, sc, bmin) > mins[a][c]) --l;
                    while (h < 255 && dequantDev(h, sc, bmin) < maxs[a][c]) ++h;
                }
                else { l = 0; h = 0; }                    // flat box on this axis: origin is the plane, exactly
            }
            qlo[a] |= l << (8 * c);
            qhi[a] |= h << (8 * c);
        }
    }
    d.ox = org[0]; d.oy = org[1]; d.oz = org[2];
    d.sx = scl[0]; d.sy = scl[1]; d.sz = scl[2];
    d.qlox = qlo[0]; d.qloy = qlo[1]; d.qloz = qlo[2];
    d.qhix = qhi[0]; d.qhiy = qhi[1]; d.qhiz = qhi[2];
    for (int c = 0; c < 4; ++c) d.child[c] = qn.child[c];
    return d;
}

} // namespace slrhip
