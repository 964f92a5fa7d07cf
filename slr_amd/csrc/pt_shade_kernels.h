// pt_shade_kernels.h — k_shade, the shading half of the wavefront path tracer (gfx950, wave64), and what only its translation
// units (pt_shade_*.hip) need beyond the visit: the shadow-queue push, the hand-over of the samples to start, the count of the
// light samples not traced, the occupancy floors.
//
// One wavefront iteration is two launches:
//
//   k_shade          every live slot: the visit (logicSlot, pt_shade_visit.h) emits the next extension ray in place and a shadow
//                    ray (slot index into the shadow queue).  A slot whose path ENDS here is finished in the same launch:
//                    weight * C goes to the sample's entry of the result window (writeResult; sensor->add itself, in pass order,
//                    is k_fold's), the wave's queue hands the slot its next (pixel, pass), and the new samples of the workgroup
//                    are started by its FIRST lanes, compacted (Job::kernel's camera half, :100-120: the 50-draw stream seeding
//                    runs on full waves).  With the primary pass (RenderParams::primary; launchPrimary, pt_kernels.h) those
//                    lanes also take the camera ray's hit from the pass's record and shade it in the same launch: the slot
//                    leaves with its first bounce in flight.
//   k_trace_ws       every slot with a ray in flight (state flag) + the shadow-ray queue, one launch (pt_trace_ws.hip)
//
// The shadow queue is a slot-index list in HBM, 16 regions (one per blockIdx % 16), filled by wave ballot + popcount prefix
// with ONE atomic per workgroup on a counter that has its own 128-byte line.  The state loads are issued together at the top,
// the material / light / spectrum tables live in LDS.
#pragma once
#include "pt_kernels.h"
#include "pt_sample_start.h"
#include "pt_shade_tables.h"
#include "pt_shade_variants.h"
#include "pt_shade_visit.h"
#include "pt_slot_state.h"

namespace slrhip {

// Append `slot` to the workgroup's region of the shadow queue: wave ballots + popcount prefixes, the four wave counts meet
// in LDS, ONE atomic per workgroup (on the region's own counter line).
struct PushLds {
    uint32_t count[4];
    uint32_t base;
};
// A lane hands in up to two slots: its own (`emit`, `slot`) and the one whose new sample it started and shaded in the same launch
// (`emitB`, `slotB`; k_shade's fused start) — still one reservation per workgroup.  A slot emits at most one shadow ray per launch
// (a path that ended emitted none), so a region still holds every slot of its blocks.
__device__ __forceinline__ void blockPush(PushLds& pl, bool emit, uint32_t slot, bool emitB, uint32_t slotB, uint32_t* queue,
                                          uint32_t* counters /* set being filled */, uint32_t shardCapacity, uint32_t* errorWord) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t shard = blockIdx.x % kShards;
    const uint64_t m = __ballot(emit), mB = __ballot(emitB);
    if (lane == 0) pl.count[wave] = (uint32_t)__popcll(m) + (uint32_t)__popcll(mB);
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t total = pl.count[0] + pl.count[1] + pl.count[2] + pl.count[3];
        pl.base = total ? atomicAdd(&counters[(Q_SHADOW * kShards + shard) * kCounterStride], total) : 0u;
        if (pl.base + total > shardCapacity) atomicOr(errorWord, ERR_QUEUE_OVERFLOW);     // cannot happen: a region holds every slot of its blocks
    }
    __syncthreads();
    if (emit || emitB) {
        uint32_t off = pl.base;
        for (uint32_t w = 0; w < wave; ++w) off += pl.count[w];
        const uint64_t below = (1ull << lane) - 1ull;
        if (emit) queue[(size_t)shard * shardCapacity + off + (uint32_t)__popcll(m & below)] = slot;
        if (emitB) queue[(size_t)shard * shardCapacity + off + (uint32_t)__popcll(m) + (uint32_t)__popcll(mB & below)] = slotB;
    }
}

// Occupancy floor of k_shade (waves per SIMD): the register allocator spills to scratch to stay under 512 / N registers.
// Measured on the spectral GGX scene: the 330-register allocation (1 wave per SIMD, 63 % of its cycles waiting on memory,
// PMC) ran at 1 393 us per launch; held to 256 registers (300 B of scratch per lane, 2 waves) it runs at 765 us.
// A floor of 3 waves costs the same kernel 988 us (more scratch than the extra wave hides), but pays on the variant
// without the glossy lobes (190 registers: 832 -> 768 us at <= 170).  The RGB variants allocate 116-161 registers
// (3-4 waves) on their own; forcing 5 or 6 waves slows them (220 -> 326 / 505 us), so their floor is left below that.
#ifndef SLR_WAVES_SPECTRAL_GLOSSY
#define SLR_WAVES_SPECTRAL_GLOSSY 2
#endif
#ifndef SLR_WAVES_SPECTRAL
#define SLR_WAVES_SPECTRAL 3
#endif
#ifndef SLR_WAVES_RGB
#define SLR_WAVES_RGB 2
#endif
// Measurement builds only (what a wave is worth): -DSLR_WAVES_RGB_CAP=N also CAPS the RGB kernels of the translation unit
// at N waves per SIMD — the compiler pads the kernel's register allocation so that no more fit.  Never set in the committed build.
#ifdef SLR_WAVES_RGB_CAP
#define SLR_SHADE_WAVES(rgb, mf) (rgb) ? SLR_WAVES_RGB : ((mf) ? SLR_WAVES_SPECTRAL_GLOSSY : SLR_WAVES_SPECTRAL), (rgb) ? SLR_WAVES_RGB_CAP : 8
#else
#define SLR_SHADE_WAVES(rgb, mf) (rgb) ? SLR_WAVES_RGB : ((mf) ? SLR_WAVES_SPECTRAL_GLOSSY : SLR_WAVES_SPECTRAL)
#endif

// What the finishing lanes of a k_shade workgroup hand to its first lanes: the samples to start.
struct StartLds {
    uint32_t lane[kShadeBlock];                 // compacted: slot = workgroup base + lane
    uint32_t pix[kShadeBlock];
    uint32_t pass[kShadeBlock];
    uint32_t waveBase[kShadeBlock / 64 + 1];
    uint32_t wentIdle;                          // lanes of the workgroup that found the queue exhausted in this launch
};
// Light samples of this launch that were not traced (logicSlot, step 3), per wave.  RGB kernels only: an instantiation that never
// names it allocates nothing.
struct DeadLds {
    uint32_t count[kShadeBlock / 64];
};

// The rays the algorithm casts are the reference's whether or not they are traced: the workgroup's untraced light samples go to
// T_SHADOW_RAYS (k_trace_ws counts the traced ones) and to T_SHADOW_SKIPPED, one atomic each (no return) per workgroup and launch on the
// workgroup's shard line, and none where the count is zero.  Called by every thread behind a barrier that follows the waves' writes.
__device__ __forceinline__ void countDeadShadows(const PathBuffers& pb, const DeadLds& dl) {
    if (threadIdx.x != 0) return;
    const uint32_t n = dl.count[0] + dl.count[1] + dl.count[2] + dl.count[3];
    if (n == 0u) return;
    atomicAdd((unsigned long long*)&pb.totals[totalIndex(T_SHADOW_RAYS, blockIdx.x % kShards)], (unsigned long long)n);
    atomicAdd((unsigned long long*)&pb.totals[totalIndex(T_SHADOW_SKIPPED, blockIdx.x % kShards)], (unsigned long long)n);
}

// PRIMARY: the instantiation for windows with a primary pass (RenderParams::primary; planShadeVariant picks it): the fused start below.
// It is a template argument and not a branch on rp.primary because the second trip costs registers whether or not it runs: one kernel
// for both took k_shade<RGB, glossy> from 163 to 181 VGPRs and the spectral kernels to 190 - 220 B more scratch, and renders WITHOUT
// the pass (spectral, environment light: render_plan.h) ran 13 - 14 % slower than before.  Without PRIMARY the
// kernel is what it was.  Built for the RGB kernels only: the plan keeps the pass off in spectral contexts.
// RESUME (with PRIMARY): the fused start goes on from the stream the primary pass left (PathBuffers::primaryRng; windows whose plan keeps
// that plane, render_plan.h) instead of seeding its own.  A template argument for the reason PRIMARY is one.
template <class S, bool LDS_TABLES, bool MF, bool MULTI = false, bool TEX = false, bool PRIMARY = false, bool RESUME = false>
__global__ __launch_bounds__(kShadeBlock)
__attribute__((amdgpu_waves_per_eu(SLR_SHADE_WAVES(S::N == 3, MF)))) void k_shade(DevScene sc, PathBuffers pb, RenderParams rp, uint32_t parity) {
    __shared__ ShadeLds<S::N != 3> lds;
    __shared__ PushLds pushLds;
    __shared__ StartLds start;
    __shared__ DeadLds deadLds;
    // The fused start without the glossy lobes runs at 4 waves per SIMD (128 VGPRs, no scratch) if nothing of one trip occupies registers
    // through the other; two things did, 140 VGPRs' worth, and are undone where kTight is set.  The other instantiations
    // are 2 to 3 waves either way and keep their code.
    constexpr bool kTight = PRIMARY && !MF;
    constexpr bool kSkipDead = S::N == 3;          // logicSlot traces no light sample that decides nothing (RGB)
    const uint32_t slot = blockIdx.x * kShadeBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;

    // ---- the end of a render: nothing left anywhere / nothing left in this block ------------------------------------------
    {
        // every slot is out of passes / the tail kernel takes over / this block is finished (all uniform); the three words are
        // requested together: evaluated one after the other they were three dependent scalar-cache round trips
        const uint32_t liveSlots = pb.activeSlots[0], tailMode = pb.tailMode[0], dead = pb.blockDead[blockIdx.x];
        if ((liveSlots == 0u) | (tailMode != 0u) | (dead != 0u)) return;
    }

    // ONE round trip for everything the visit needs that does not depend on the slot's state: flags, visibility word, the pixel's
    // pool counter, the state records (SlotLoads) and the tables staged below; ONE barrier publishes the tables and decides
    // whether the block has any work left.
    uint32_t flags = pb.flags[slot];                                      // numSlots = 256 x workgroups: always in range
    const uint32_t vis = pb.visible[slot];
    SlotLoads<S> in;
    in.issue(sc, pb, rp, slot);
    const uint32_t state0 = F_STATE(flags);
    const uint32_t globalWave = blockIdx.x * (kShadeBlock / 64) + wave;
    const uint32_t taken = pb.cursor[globalWave];                         // samples this wave has taken from its queue (wave-uniform)
    if (threadIdx.x == 0) start.wentIdle = 0u;
    if (LDS_TABLES) stageShadeTables<S::N != 3>(sc, lds);
    {
        const int anyWork = __syncthreads_or(state0 != ST_IDLE);
        if (!anyWork) {
            // every slot here is idle — its queue is exhausted and a slot never leaves ST_IDLE within a window: the block is
            // finished for the rest of the window; say so, and the scanning kernels stop reading its state
            if (threadIdx.x == 0) pb.blockDead[blockIdx.x] = 1u;
            return;
        }
    }
    const float* lightPMF = LDS_TABLES ? lds.lightPMF : sc.lightPMF;
    const float* lightCDF = LDS_TABLES ? lds.lightCDF : sc.lightCDF;

    // Two trips through ONE inlined visit.  Trip 0: this lane's own slot.  Trip 1 (PRIMARY instantiations only): the samples the workgroup
    // starts in this launch, on its first lanes — the camera half in registers, the camera ray's hit from the primary pass's record,
    // then the very visit a slot in ST_FIRST_HIT gets: the slot leaves the launch with its first bounce in flight instead of
    // spending an iteration, and a trip through the slot state, on its camera ray.  Every exit from the loop is uniform over the workgroup.
    // The two trips are UNROLLED (two copies of the visit's code): kept as a loop, the register allocation of k_shade<RGB, lds> went
    // from 120 VGPRs to 200 (the visit's inputs as loop-carried values; 141 unrolled) and the headline frame from 300 ms to 364 ms —
    // measured, DESIGN.md 7.17.
    bool shadow0 = false, shadow1 = false;         // the shadow rays of the two trips: one reservation for both, after the loop
    uint32_t deadWave = 0u;                        // light samples of this wave's lanes that were not traced, both trips (wave-uniform)
    uint32_t curSlot = slot, curVis = vis;
    bool curActive = state0 == ST_FIRST_HIT || state0 == ST_NEXT_HIT || state0 == ST_FINISH;
    uint4 curHdr = make_uint4(0u, 0u, 0u, 0u);     // trip 1: the new sample's header, from registers
#pragma clang loop unroll(full)
    for (uint32_t trip = 0; trip < 2u; ++trip) {
    bool emitExt = false, emitShadow = false, pathEnded = false, deadShadow = false;
    S radiance;
    // kTight: each trip reads the scene's uniform scalars through a copy of its own, opaque to the compiler.  The trips are a loop until
    // it is unrolled, and loop-invariant code motion runs first: it lifts the float conversions and quotients of these words out of the
    // visit, where they then sit in seven vector registers (the chip has no scalar float unit) from the top of the kernel to trip 1
    DevScene scT;
    if constexpr (kTight) {
        scT = sc;
        asm volatile("" : "+s"(scT.envWidth), "+s"(scT.envHeight), "+s"(scT.envMapWidth), "+s"(scT.envMapHeight), "+s"(scT.aggImportance));
    }
    const DevScene& scV = kTight ? scT : sc;
    if (curActive)
        logicSlot<S, LDS_TABLES, MF, MULTI, TEX, true, kTight>(scV, pb, rp, lds, lightPMF, lightCDF, curSlot, in, flags, curVis, radiance, emitExt, emitShadow, pathEnded, &deadShadow);
    if constexpr (kSkipDead) deadWave += (uint32_t)__popcll(__ballot(deadShadow));

    // ---- a path that ended: its contribution goes to the result window, in the same launch ------------------------------------
    if (pathEnded) {
        const uint4 hdr = trip == 0u ? pb.hdr[(size_t)curSlot * pb.hdrStride] : curHdr;
        writeResult<S>(pb, rp, curSlot, flags, hdr, S::N == 3, radiance);
        // a path that ends in its first visit (a miss, a zero BSDF sample): the slot takes its next sample in the next launch
        if (trip != 0u) pb.flags[curSlot] = F_MAKE((uint32_t)ST_REGEN, 0u, 0u, 0u, 0u, 0u);
    }
    if (trip != 0u) { shadow1 = emitShadow; break; }
    shadow0 = emitShadow;
    // ---- stream compaction of the shadow rays (extension rays need no queue: the traversal kernel reads the state flag); with the
    //      fused start, after the second trip ----------
    if (!PRIMARY) {
        if constexpr (kSkipDead) { if (lane == 0) deadLds.count[wave] = deadWave; }     // published by blockPush's barriers
        blockPush(pushLds, emitShadow, slot, false, 0u, pb.shadowQueue, pb.queueCount + parity * kQueueSetWords, rp.shardCapacity, pb.errorWord);
        if constexpr (kSkipDead) countDeadShadows(pb, deadLds);
    }
    if (rp.countSlots) {
        const uint64_t ma = __ballot(emitExt || emitShadow || pathEnded);
        if (lane == 0 && ma) atomicAdd((unsigned long long*)&pb.totals[totalIndex(T_SLOT_VISITS, blockIdx.x % kShards)], (unsigned long long)__popcll(ma));
    }

    // ---- the next sample of every slot that needs one (its path ended, or it has not started yet: ST_REGEN after k_reset_slots):
    //      the wanting lanes of a wave, in lane order, take the next items of the wave's queue (pt_kernels.h WorkItem) --------------
    const bool wants = pathEnded || state0 == ST_REGEN;
    {
        const uint64_t mw = __ballot(wants);
        WorkItem w;
        w.valid = false;
        if (wants) w = workItemOf(rp, globalWave, taken + (uint32_t)__popcll(mw & ((1ull << lane) - 1ull)));
        if (lane == 0 && mw) pb.cursor[globalWave] = taken + (uint32_t)__popcll(mw);
        const bool becameIdle = wants && !w.valid;
        if (becameIdle) pb.flags[slot] = F_MAKE((uint32_t)ST_IDLE, 0u, 0u, 0u, 0u, 0u);
        const uint64_t mi = __ballot(becameIdle);
        if (lane == 0 && mi) atomicAdd(&start.wentIdle, (uint32_t)__popcll(mi));
        // compaction of the samples to start over the workgroup: wave counts in LDS, then lanes 0 .. n-1 run startSample, so
        // that the 50-draw seeding of the stream (the seeding contract, ~400 integer operations) and the camera arithmetic run
        // on full waves instead of on the quarter of the lanes whose path has just ended
        const bool starts = wants && w.valid;
        const uint64_t ms = __ballot(starts);
        if (lane == 0) start.waveBase[wave] = (uint32_t)__popcll(ms);
        __syncthreads();
        uint32_t base = 0;
        for (uint32_t k = 0; k < wave; ++k) base += start.waveBase[k];
        if (starts) {
            const uint32_t i = base + (uint32_t)__popcll(ms & ((1ull << lane) - 1ull));
            start.lane[i] = threadIdx.x;
            start.pix[i] = w.pix;
            start.pass[i] = w.pass;
        }
        __syncthreads();
        // the live count: one atomic per workgroup and launch, on one of kShards lines (PathBuffers::idleShards)
        if (threadIdx.x == 0 && start.wentIdle) atomicAdd(&pb.idleShards[(blockIdx.x % kShards) * kCounterStride], start.wentIdle);
        const uint32_t n = start.waveBase[0] + start.waveBase[1] + start.waveBase[2] + start.waveBase[3];
        if (!PRIMARY) {
            // no primary pass (RenderParams::primary): the camera ray goes through the slot state and k_trace_ws
            if (threadIdx.x < n)
                startSample<S>(sc, pb, rp, blockIdx.x * kShadeBlock + start.lane[threadIdx.x], start.pix[threadIdx.x], start.pass[threadIdx.x]);
            break;
        }
        if (n == 0u) break;
        curActive = threadIdx.x < n;
        if (curActive) {
            curSlot = blockIdx.x * kShadeBlock + start.lane[threadIdx.x];
            const uint32_t pix = start.pix[threadIdx.x], pass = start.pass[threadIdx.x];
            // RESUME: one round trip for everything the new sample needs — the record, the stream the primary pass left behind the camera
            // draws (it drew them for the same sample: no seeding here) and the pixel's coordinates; else the record first: its round
            // trip is hidden behind the seeding of the stream
            loadPrimaryRecord<S>(sc, pb, rp, pix, pass, in.h, in.hitInstance);
            SampleStart st;
            if constexpr (RESUME) st = resumeSample<S>(sc, rp, pb.pixelXY[pix], pb.primaryRng[windowEntry(pix, pass, rp.sppCount)]);
            else st = beginSample<S>(sc, pb, rp, pix, pass);
            curHdr = make_uint4(pix, __float_as_uint(st.camWeight), __float_as_uint(st.wlOffset), pass);
            pb.hdr[(size_t)curSlot * pb.hdrStride] = curHdr;
            // the rest of what startSample writes stays in registers: the visit below stores the state of the first bounce
            in.r4 = make_uint4(st.rng.s0, st.rng.s1, st.rng.s2, st.rng.s3);
            in.alpha = S(1.0f); in.pdfPrev = 0.0f;
            in.o4 = make_float4(st.org.x, st.org.y, st.org.z, 0.0f);
            in.d4 = make_float4(st.dir.x, st.dir.y, st.dir.z, INFINITY);
            in.wlOffset = S::N == 3 ? 0.0f : st.wlOffset;
            flags = F_MAKE((uint32_t)ST_FIRST_HIT, 0u, st.wl, 0u, 0u, 0u);
            curVis = 0u;
        }
        if (threadIdx.x == 0)       // the read-out of slrhip_debug_primary_samples: one atomic (no return) per workgroup and launch, on one of kShards lines
            atomicAdd((unsigned long long*)&pb.totals[totalIndex(T_PRIMARY_STARTS, blockIdx.x % kShards)], (unsigned long long)n);
    }
    }
    if (PRIMARY) {
        if constexpr (kSkipDead) { if (lane == 0) deadLds.count[wave] = deadWave; }
        blockPush(pushLds, shadow0, slot, shadow1, curSlot, pb.shadowQueue, pb.queueCount + parity * kQueueSetWords, rp.shardCapacity, pb.errorWord);
        if constexpr (kSkipDead) countDeadShadows(pb, deadLds);
    }
}

// pt_shade_variants.h: a translation unit builds a k_shade by instantiating this (`template ShadeKernel shadeKernel<...>();`); the
// instantiations are spread over pt_shade_{rgb,spec16,multi_*,tex_*}*.hip so that the build parallelises.
template <class S, bool LDS_TABLES, bool MF, bool MULTI, bool TEX, bool PRIMARY, bool RESUME>
ShadeKernel shadeKernel() { return &k_shade<S, LDS_TABLES, MF, MULTI, TEX, PRIMARY, RESUME>; }

} // namespace slrhip
