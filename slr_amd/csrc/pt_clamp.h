// pt_clamp.h — the sample clamp of slrhip_clamp_begin (include/slrhip.h): what happens to one sample between the result window
// and the sensor.  ONE definition for the host export (slrhip_clamp_sample, host_util.cpp) and the fold kernels (pt_fold.h).
// float32 operations in the order written (both sides are built with -ffp-contract=off), IEEE division: host and device agree
// bit for bit.
#pragma once
#include <cmath>
#include <cstdint>

#include "pt_luminance.h"

namespace slrhip {

static const uint32_t kClampDropNonFinite = 1u;        // SLRHIP_CLAMP_DROP_NONFINITE (checked in slrhip_api.hip)
enum : uint32_t { CLAMP_KEPT = 0u, CLAMP_CLAMPED = 1u, CLAMP_DROPPED = 2u };

// The rule on the N values `v` its caller holds of a sample; lum(values) is the sample's luminance (pt_luminance.h) from N such
// values — on the host N is all of the sample's components, in the spectral fold it is one plane of four bins and lum() ends in
// the quad exchange.  That is why there are no branches: the scaled values and their luminance are evaluated for EVERY sample and
// the outcome is selected afterwards, so the exchange runs in uniform control flow (limit / Y of a sample that is not clamped may
// be anything, infinity and NaN included; it is not used).  yIn: Y of the sample as it came; yOut: of the sample as the sensor
// receives it.  Returns CLAMP_*.
template <int N, class Lum>
SLR_HOST_DEV uint32_t clampSample(float (&v)[N], float limit, uint32_t flags, const Lum& lum, float& yIn, float& yOut) {
    const float Y = lum(v);
    const bool drop = (flags & kClampDropNonFinite) != 0u && !(fabsf(Y) < INFINITY);       // NaN or +-infinity
    const bool clamp = !drop && Y > limit;                                                 // false for a NaN; Y == limit is kept
    const float f = limit / Y;
    float s[N];
    for (int k = 0; k < N; ++k) s[k] = v[k] * f;
    const float Y2 = lum(s);                                                               // the same expression, evaluated again
    for (int k = 0; k < N; ++k) v[k] = drop ? 0.0f : clamp ? s[k] : v[k];
    yIn = Y;
    yOut = drop ? 0.0f : clamp ? Y2 : Y;
    return drop ? CLAMP_DROPPED : clamp ? CLAMP_CLAMPED : CLAMP_KEPT;
}

// the luminance of a whole sample held in one place (the host; N = 3 or 16)
struct LuminanceRGB {
    SLR_HOST_DEV float operator()(const float (&v)[3]) const { return sampleLuminanceRGB(v[0], v[1], v[2]); }
};
struct LuminanceSpec16 {
    SLR_HOST_DEV float operator()(const float (&v)[16]) const {
        float p[4];
        for (uint32_t q = 0; q < 4; ++q) p[q] = sampleLuminancePlane(q, v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        return sampleLuminanceOfPlanes(p[0] + p[1], p[2] + p[3]);
    }
};

} // namespace slrhip
