// pt_slot_state.h — the state of a path slot in HBM and how a visit reads and writes it (gfx950, wave64).
//
// A path SLOT carries one light path at a time through the reference's bounce loop (Renderers/PathTracingRenderer.cpp:137-262);
// it is not bound to a pixel: whenever its path ends it takes the next sample of its wave's work queue (pt_kernels.h WorkItem).
// All path state is SoA in 16-byte records (PathBuffers, pt_kernels.h) so a wave's loads are 1 KiB bursts.  Here: the flags word,
// the spectrum-valued records (SpecIO), the records every visit reads (SlotLoads) and the path's radiance sum (SpAcc).
#pragma once
#include "pt_device.h"
#include "pt_kernels.h"

namespace slrhip {

enum : uint32_t {
    ST_IDLE = 0,            // no more samples for this slot
    ST_REGEN = 1,           // start the next sample: every slot after k_reset_slots; in the tail kernel also "a path just ended" (bit 15)
    ST_FIRST_HIT = 2,       // camera ray in flight        (PathTracingRenderer.cpp:147)
    ST_NEXT_HIT = 3,        // BSDF-sampled ray in flight  (:225)
    ST_FINISH = 4           // path ended while a shadow ray was still pending
};
// flags word: [2:0] state | [9:3] pathLength | [12] wlFlags.LambdaIsSelected | [13] previous direction was delta
//             | [14] shadow ray pending | [15] a finished path awaits accumulation | [19:16] selectedLambda
#define F_STATE(f) ((f) & 7u)
#define F_PATHLEN(f) (((f) >> 3) & 127u)
#define F_WL(f) (((f) >> 16) & 15u)
#define F_WLSEL(f) (((f) >> 12) & 1u)
#define F_DELTA(f) (((f) >> 13) & 1u)
#define F_SHADOW(f) (((f) >> 14) & 1u)
#define F_HASPATH(f) (((f) >> 15) & 1u)
#define F_SPVALID(f) (((f) >> 10) & 1u)      // spectral mode: the path's radiance sum in HBM has been written since the path began
#define F_MAKE(state, len, wl, wlsel, delta, shadow) \
    ((state) | ((len) << 3) | ((wl) << 16) | ((wlsel) << 12) | ((delta) << 13) | ((shadow) << 14))

// Spectrum-valued path state in HBM.  RGB: one float4 per slot, the scalar that travels with it in .w.
// Spectral: four float4 planes per array (plane p of slot i at [p * numSlots + i], so every plane is a coalesced
// stream) and the scalar in an array of its own.
template <class S> struct SpecIO;
template <> struct SpecIO<RGB> {
    static __device__ __forceinline__ void load(const float4* a, const float* /*scalars*/, uint32_t slot, uint32_t /*n*/, RGB& v, float& w) {
        const float4 q = a[slot];
        v = RGB(q.x, q.y, q.z); w = q.w;
    }
    static __device__ __forceinline__ void store(float4* a, float* /*scalars*/, uint32_t slot, uint32_t /*n*/, const RGB& v, float w) {
        a[slot] = make_float4(v.r, v.g, v.b, w);
    }
};
template <> struct SpecIO<Spec16> {
    static __device__ __forceinline__ void load(const float4* a, const float* scalars, uint32_t slot, uint32_t n, Spec16& v, float& w) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const float4 q = a[(size_t)p * n + slot];
            v.c[4 * p] = q.x; v.c[4 * p + 1] = q.y; v.c[4 * p + 2] = q.z; v.c[4 * p + 3] = q.w;
        }
        w = scalars ? scalars[slot] : 0.0f;
    }
    static __device__ __forceinline__ void store(float4* a, float* scalars, uint32_t slot, uint32_t n, const Spec16& v, float w) {
#pragma unroll
        for (int p = 0; p < 4; ++p) a[(size_t)p * n + slot] = make_float4(v.c[4 * p], v.c[4 * p + 1], v.c[4 * p + 2], v.c[4 * p + 3]);
        if (scalars) scalars[slot] = w;
    }
};

// The records of a slot that a visit reads whatever the slot's state is.  k_shade requests them at the very top of the kernel,
// together with the slot's flags and the tables it stages in LDS, so that they travel in ONE memory round trip before the
// workgroup's barrier instead of in three dependent ones (flags -> tables -> state); the tail kernel requests them just before
// its visit.
template <class S>
struct SlotLoads {
    uint4 r4;                  // xorshift128 state
    S alpha;                   // path throughput
    float pdfPrev;
    float4 h, o4, d4;          // hit record, ray origin, ray direction
    int32_t hitInstance;       // instanced scenes: the TransformedSurfaceObject of the hit
    float wlOffset;            // spectral mode: the sample's wavelength offset (sample header)
    __device__ __forceinline__ void issue(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t slot) {
        r4 = pb.rng[(size_t)slot * pb.hdrStride];
        SpecIO<S>::load(pb.alpha, pb.pdfPrev, slot, rp.numSlots, alpha, pdfPrev);
        h = pb.hit[slot];
        hitInstance = sc.instances ? pb.hitInstance[slot] : -1;
        o4 = pb.rayOrg[(size_t)slot * pb.rayStride];
        d4 = pb.rayDir[(size_t)slot * pb.rayStride];
        wlOffset = S::N == 3 ? 0.0f : __uint_as_float(pb.hdr[(size_t)slot * pb.hdrStride].z);
    }
};

// SampledSpectrumSum sp of Job::contribution (PathTracingRenderer.cpp:141): see the note at its use in logicSlot.
template <class S> struct SpAcc;
// A path starts with sp = 0 (and alpha = 1, no previous PDF): startSample does not write those records, the first visit
// (state FIRST_HIT) supplies the values instead of what it loaded.  RGB keeps the pair in registers and always stores it,
// so it is valid from then on; the spectral variants update HBM only when a contribution arrives and track that in `valid`
// (flag bit 10), which writeResult consults before reading the sum.
template <> struct SpAcc<RGB> {
    // The Kahan pair is read only once the path has written it (flag bit 10) and written back only by a visit that added to it;
    // the pending light sample only by a visit that has one (flag bit 14).  Most visits do neither: a first hit adds only on an
    // emitter, a later one when its shadow ray came back visible or the ray found a light.
    RGB r, c, nee;
    bool valid, changed;
    __device__ __forceinline__ void begin(const PathBuffers& pb, uint32_t slot, uint32_t n, uint32_t flags, bool /*resolves*/) {
        float unused;
        valid = F_STATE(flags) != ST_FIRST_HIT && F_SPVALID(flags);
        changed = false;
        r = RGB(); c = RGB(); nee = RGB();
        if (valid) {
            SpecIO<RGB>::load(pb.spR, nullptr, slot * pb.spStride, n * pb.spStride, r, unused);
            SpecIO<RGB>::load(pb.spC, nullptr, slot * pb.spStride, n * pb.spStride, c, unused);
        }
        if (F_SHADOW(flags)) SpecIO<RGB>::load(pb.nee, nullptr, slot, n, nee, unused);
    }
    __device__ __forceinline__ void startPath(bool first, uint32_t) { if (first) { r = RGB(); c = RGB(); } }
    __device__ __forceinline__ uint32_t validBits() const { return (valid || changed) ? 1u << 10 : 0u; }
    __device__ __forceinline__ RGB total() const { return r; }
    __device__ __forceinline__ void addPendingNee(const PathBuffers&, uint32_t, uint32_t) { kahanAdd(r, c, nee); changed = true; }
    __device__ __forceinline__ void add(const PathBuffers&, uint32_t, uint32_t, const RGB& v) { kahanAdd(r, c, v); changed = true; }
    __device__ __forceinline__ void end(const PathBuffers& pb, uint32_t slot, uint32_t n, bool pathContinues) {
        if (!changed) return;
        SpecIO<RGB>::store(pb.spR, nullptr, slot * pb.spStride, n * pb.spStride, r, 0.0f);
        if (pathContinues) SpecIO<RGB>::store(pb.spC, nullptr, slot * pb.spStride, n * pb.spStride, c, 0.0f);       // a finished path only hands over the sum
    }
};
template <> struct SpAcc<Spec16> {
    // The Kahan pair (2 x 64 B) and the pending light sample (64 B) stay in HBM and are updated in place when a contribution
    // arrives.  The one contribution that is known before the visit starts — the pending light sample of a slot whose shadow ray
    // came back visible (flag bit 14 + the visibility word, both read before the state loads are issued) — has its twelve 16-byte
    // operands requested WITH the state loads, so that the resolve costs no memory round trip of its own.
    bool valid;
    float4 pn[4], pr[4], pc[4];
    bool fetched;
    __device__ __forceinline__ void begin(const PathBuffers& pb, uint32_t slot, uint32_t n, uint32_t flags, bool resolves) {
        fetched = false;
        if (resolves) {
            const bool had = F_STATE(flags) != ST_FIRST_HIT && F_SPVALID(flags);
            const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                pn[p] = pb.nee[(size_t)p * n + slot];
                pr[p] = had ? pb.spR[((size_t)p * n + slot) * pb.spStride] : zero;
                pc[p] = had ? pb.spC[((size_t)p * n + slot) * pb.spStride] : zero;
            }
            fetched = true;
        }
    }
    __device__ __forceinline__ void startPath(bool first, uint32_t flags) { valid = !first && F_SPVALID(flags); }
    __device__ __forceinline__ uint32_t validBits() const { return valid ? 1u << 10 : 0u; }
    __device__ __forceinline__ Spec16 total() const { return Spec16(); }      // the sum is in HBM (flag bit 10 says whether it was ever written)
    __device__ __forceinline__ void add(const PathBuffers& pb, uint32_t slot, uint32_t n, const Spec16& v) {
        // plane by plane: 4 components of the Kahan pair in flight at a time
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float4 r = zero, c = zero;
            if (valid) { r = pb.spR[((size_t)p * n + slot) * pb.spStride]; c = pb.spC[((size_t)p * n + slot) * pb.spStride]; }
            kahanAdd(r.x, c.x, v.c[4 * p]); kahanAdd(r.y, c.y, v.c[4 * p + 1]);
            kahanAdd(r.z, c.z, v.c[4 * p + 2]); kahanAdd(r.w, c.w, v.c[4 * p + 3]);
            pb.spR[((size_t)p * n + slot) * pb.spStride] = r;
            pb.spC[((size_t)p * n + slot) * pb.spStride] = c;
        }
        valid = true;
    }
    __device__ __forceinline__ void addPendingNee(const PathBuffers& pb, uint32_t slot, uint32_t n) {
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float4 v, r = zero, c = zero;
            if (fetched) { v = pn[p]; r = pr[p]; c = pc[p]; }
            else {
                v = pb.nee[(size_t)p * n + slot];
                if (valid) { r = pb.spR[((size_t)p * n + slot) * pb.spStride]; c = pb.spC[((size_t)p * n + slot) * pb.spStride]; }
            }
            kahanAdd(r.x, c.x, v.x); kahanAdd(r.y, c.y, v.y); kahanAdd(r.z, c.z, v.z); kahanAdd(r.w, c.w, v.w);
            pb.spR[((size_t)p * n + slot) * pb.spStride] = r;
            pb.spC[((size_t)p * n + slot) * pb.spStride] = c;
        }
        valid = true;
    }
    __device__ __forceinline__ void end(const PathBuffers&, uint32_t, uint32_t, bool) {}
};

} // namespace slrhip
