// pt_trace_ws.hip — the render's traversal: k_trace_ws, one launch per wavefront iteration for the extension and the shadow rays
// of the path state's slots, through the wave-specialised consumer of pt_trace_ws.h (gfx950, wave64).
//
//   wave 0      PRODUCER (wsProduce): streams the slot arrays in order (coalesced 1 KiB bursts, kSub 64-slot sub-chunks in
//               flight), keeps the slots that have a ray, and appends them to the ring of rays in LDS; then the shadow queue.
//   waves 1..NC CONSUMERS (wsConsume): results go to the slots' hit / hitInstance / visible records (WsRenderIO).
//
// The index-fed clients of the same consumer (ray queries, the feature trace, the primary pass) are in pt_trace_indexed.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "pt_trace_ws.h"

namespace slrhip {

#ifndef SLR_WS_AHEAD
#define SLR_WS_AHEAD 4
#endif
static const int kAhead = SLR_WS_AHEAD;               // chunks whose state flags the producer reads in one round trip (see wsProduce)
static_assert(64 % kAhead == 0 && kAhead <= 32, "the producer's 64-chunk dead-block mask is consumed kAhead bits at a time");

static WsTuning readWsTuning() {
    WsTuning t;
    if (const char* e = tuningEnv("SLRHIP_WS_REFILL")) t.refill = (uint32_t)std::min(std::max(atoi(e), 1), 64);
    if (const char* e = tuningEnv("SLRHIP_WS_NC")) { const int n = atoi(e); t.consumers = n == 3 || n == 7 || n == 15 ? n : 0; }
    if (const char* e = tuningEnv("SLRHIP_WS_BLOCKS_PER_CU")) { const int b = atoi(e); t.blocksPerCU = b >= 1 && b <= 8 ? b : 0; }   // experiments
    return t;
}
const WsTuning& wsTuning() {
    static const WsTuning tuning = readWsTuning();
    return tuning;
}
int traceWsBlocksPerCU(bool quantized) { return wsBlocksPerCU(wsConsumers(quantized)); }

__device__ __forceinline__ void wsBlockAdd(uint64_t* totals, uint32_t kind, uint32_t v, uint32_t* scratch) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < blockDim.x / 64; ++w) t += scratch[w];
        if (t) atomicAdd((unsigned long long*)&totals[totalIndex(kind, blockIdx.x % kShards)], (unsigned long long)t);
    }
}

// The render's slots: a ring entry names a slot of the path state, results go to its hit / hitInstance / visible records.
struct WsRenderIO {
    const PathBuffers& pb;
    __device__ __forceinline__ uint32_t* errorWord() const { return pb.errorWord; }
    template <bool INST>
    __device__ __forceinline__ void finish(uint32_t slot, uint32_t hitTri, float hitT, float hitB1, float hitB2, int32_t hitInst) const {
        if (slot & kShadowBit) pb.visible[slot & ~kShadowBit] = hitTri == 0xFFFFFFFFu ? 1u : 0u;      // testVisibility
        else {
            pb.hit[slot] = make_float4(__uint_as_float(hitTri), hitT, hitB1, hitB2);
            if (INST) pb.hitInstance[slot] = hitInst;
        }
    }
};

// The producer wave (see the head of this file and k_trace_ws): phase 1 walks the slots for extension rays, phase 2 the shadow
// queue; both append to the ray ring of the workgroup.
template <class LDS>
__device__ __forceinline__ void wsProduce(const PathBuffers& pb, LDS& lds, uint32_t numSlots, uint32_t shardCapacity, uint32_t parity,
                                          uint32_t& extRays, uint32_t& shadowRays, WsDebug& dbg) {
    const uint32_t lane = threadIdx.x;
    uint32_t tailLocal = 0;
    const uint32_t chunk = kSub * 64;
    bool ok = true;
    {
        // The state flags of kAhead chunks are fetched in one round trip, the ray records only for chunks that have a ray:
        // near the end of a render most slots are idle, and a producer that pays one memory round trip per 128 slots
        // whether or not they hold a ray makes an almost empty launch last ~58 us (28 dependent round trips per workgroup).
        // Blocks of 256 slots whose slots have all run out of passes are marked by k_shade (PathBuffers::blockDead): their
        // state is not read at all.  One 64-lane load fetches the marks of this workgroup's next 64 chunks.
        const uint32_t numChunks = (numSlots + chunk - 1) / chunk;
        uint64_t deadMask = 0;
        uint32_t group = 0;
        for (uint32_t c0 = blockIdx.x; ok && c0 < numChunks; c0 += gridDim.x * kAhead, group += kAhead) {
            if ((group & 63u) == 0) {
                const uint64_t cl = (uint64_t)c0 + (uint64_t)lane * gridDim.x;       // this lane's chunk among the next 64
                deadMask = __ballot(cl >= numChunks || pb.blockDead[(cl * chunk) / 256u] != 0u);
            }
            const uint32_t deadBits = (uint32_t)(deadMask >> (group & 63u)) & ((1u << kAhead) - 1u);
            if (deadBits == (1u << kAhead) - 1u) continue;                            // wave-uniform
            uint32_t fl[kAhead][kSub];
#pragma unroll
            for (int a = 0; a < kAhead; ++a)
#pragma unroll
                for (int j = 0; j < kSub; ++j) {
                    const uint64_t s = (uint64_t)(c0 + a * gridDim.x) * chunk + j * 64 + lane;
                    fl[a][j] = (s < numSlots && !((deadBits >> a) & 1u)) ? __builtin_nontemporal_load(&pb.flags[s]) : 0u;
                }
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                const uint32_t c = c0 + a * gridDim.x;
                bool live[kSub];
                bool any = false;
#pragma unroll
                for (int j = 0; j < kSub; ++j) {
                    const uint32_t state = fl[a][j] & 7u;
                    live[j] = state == 2u || state == 3u;
                    any = any || __ballot(live[j]) != 0;
                }
                if (!any) continue;       // wave-uniform (also true past the last chunk: those flags were read as 0)
                float4 o[kSub], d[kSub];
#pragma unroll
                for (int j = 0; j < kSub; ++j) {
                    const uint32_t s = c * chunk + j * 64 + lane;
                    o[j] = live[j] ? ntLoad4(&pb.rayOrg[(size_t)s * pb.rayStride]) : make_float4(0, 0, 0, 0);
                    d[j] = live[j] ? ntLoad4(&pb.rayDir[(size_t)s * pb.rayStride]) : make_float4(0, 0, 0, 0);
                }
                ok = wsWaitSpace(lds, tailLocal, chunk, &dbg.producerWaits);
                if (!ok) { if (lane == 0) atomicOr(pb.errorWord, ERR_RING_SPACE); break; }
#pragma unroll
                for (int j = 0; j < kSub; ++j) tailLocal += wsAppend(lds, tailLocal, live[j], c * chunk + j * 64 + lane, o[j], d[j]);
                WS_STORE(&lds.tail, tailLocal, __ATOMIC_RELEASE);
            }
        }
        extRays = tailLocal;
    }
    if (ok) {
        const uint32_t shard = blockIdx.x % kShards;
        const uint32_t n = pb.queueCount[queueCounterIndex(parity, Q_SHADOW, shard)];
        const uint32_t* queue = pb.shadowQueue + (size_t)shard * shardCapacity;
        const uint32_t numChunks = (n + chunk - 1) / chunk;
        for (uint32_t c = blockIdx.x / kShards; c < numChunks; c += gridDim.x / kShards) {
            uint32_t sl[kSub];
            float4 o[kSub], d[kSub];
#pragma unroll
            for (int j = 0; j < kSub; ++j) {
                const uint32_t i = c * chunk + j * 64 + lane;
                sl[j] = i < n ? __builtin_nontemporal_load(&queue[i]) : kIdle;
            }
#pragma unroll
            for (int j = 0; j < kSub; ++j) {
                const bool valid = sl[j] != kIdle;
                o[j] = valid ? ntLoad4(&pb.rayOrg[(size_t)sl[j] * pb.rayStride]) : make_float4(0, 0, 0, 0);
                d[j] = valid ? ntLoad4(&pb.shadowDir[sl[j]]) : make_float4(0, 0, 0, 0);
                o[j].w = kRayEpsilon;
            }
            if (!wsWaitSpace(lds, tailLocal, chunk, &dbg.producerWaits)) { if (lane == 0) atomicOr(pb.errorWord, ERR_RING_SPACE); break; }
#pragma unroll
            for (int j = 0; j < kSub; ++j) tailLocal += wsAppend(lds, tailLocal, sl[j] != kIdle, sl[j] | kShadowBit, o[j], d[j]);
            WS_STORE(&lds.tail, tailLocal, __ATOMIC_RELEASE);
        }
        shadowRays = tailLocal - extRays;
    }
    WS_STORE(&lds.done, 1u, __ATOMIC_RELEASE);
    if (lane != 0) { extRays = 0; shadowRays = 0; }
}

// ONE launch traces both ray kinds of an iteration, so the tail of the extension rays (the last long rays of a few
// waves) is filled by shadow rays instead of idle CUs; measured: ~70 + ~50 us of fixed cost per launch pair before.
//   phase 1, extension rays (closest hit): the producer walks ALL slots of its share (no queue); a slot has a ray in flight
//            iff its state is FIRST_HIT or NEXT_HIT (flag values 2 and 3, pt_slot_state.h).
//   phase 2, shadow rays: Scene::testVisibility (SurfaceObject.cpp:418-430) = "no hit in [eps, d(1-eps)]"; workgroup b
//            serves queue region b % kShards (gridDim is a multiple of kShards).
template <bool COUNT, int NC, bool QUANT, bool INST>
__global__ __launch_bounds__(64 * (NC + 1)) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_trace_ws(DevScene sc, PathBuffers pb, uint32_t numSlots, uint32_t shardCapacity, uint32_t parity, uint32_t refill, uint32_t tailSlots) {
    __shared__ WsLds<NC> lds;
    const uint32_t live = liveSlots(pb, numSlots);                                   // as of the end of the k_shade launch before this one (uniform)
    if (blockIdx.x == 0 && threadIdx.x == 0) pb.activeSlots[0] = live;               // for the next k_shade launch and the host
    if (live == 0) return;                         // every slot is idle: nothing to trace
    if (tailModeBegins(pb, live, tailSlots, parity)) return;      // the last paths go to the tail kernel (uniform over the grid, pt_kernels.h)
    if (blockIdx.x == 0 && threadIdx.x < Q_KINDS * kShards) {
        // clear the counter set the logic kernel of this iteration fills
        pb.queueCount[queueCounterIndex(parity ^ 1, threadIdx.x / kShards, threadIdx.x % kShards)] = 0;
    }
    wsResetRing(lds);
    uint32_t extRays = 0, shadowRays = 0;
    WsCounts cnt;
    WsDebug dbg;
    if (threadIdx.x < 64) wsProduce(pb, lds, numSlots, shardCapacity, parity, extRays, shadowRays, dbg);
    else wsConsume<COUNT, NC, QUANT, INST>(sc, WsRenderIO{pb}, lds, refill, cnt, dbg);
    wsBlockAdd(pb.totals, T_EXT_RAYS, extRays, lds.red);
    wsBlockAdd(pb.totals, T_SHADOW_RAYS, shadowRays, lds.red);
    if (COUNT) {
        wsBlockAdd(pb.totals, T_NODES_CLOSEST, cnt.nodes[0], lds.red); wsBlockAdd(pb.totals, T_TRIS_CLOSEST, cnt.tris[0], lds.red);
        wsBlockAdd(pb.totals, T_NODES_SHADOW, cnt.nodes[1], lds.red); wsBlockAdd(pb.totals, T_TRIS_SHADOW, cnt.tris[1], lds.red);
        const bool l0 = (threadIdx.x & 63u) == 0;      // wave-level figures: lane 0 of each wave speaks; cycles in units of 64
        wsBlockAdd(pb.totals, T_WS_STEPS, l0 ? dbg.steps : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_IDLE_SPINS, l0 ? dbg.idleSpins : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_CYCLES, l0 ? (uint32_t)(dbg.cycles >> 6) : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_IDLE_CYCLES, l0 ? (uint32_t)(dbg.idleCycles >> 6) : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_REFILLS, l0 ? dbg.refills : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_PRODUCER_WAITS, l0 ? dbg.producerWaits : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_NODE_BLOCKS, l0 ? dbg.nodeBlocks : 0u, lds.red);
        wsBlockAdd(pb.totals, T_WS_TRI_BLOCKS, dbg.triBlocks, lds.red);
        wsBlockAdd(pb.totals, T_WS_ACTIVE_LANES, l0 ? dbg.activeLanes : 0u, lds.red);
    }
}

template <bool COUNT, int NC>
static void launchTraceWsT(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, uint32_t blocks, hipStream_t stream) {
    const dim3 grid(blocks), block(64 * (NC + 1));
    const uint32_t refill = wsTuning().refill;
    // instanced scenes: float nodes only (slrhip_upload_scene does not quantize them)
    if (sc.instances) hipLaunchKernelGGL((k_trace_ws<COUNT, NC, false, true>), grid, block, 0, stream, sc, pb, rp.numSlots, rp.shardCapacity, parity, refill, rp.tailSlots);
    else if (sc.nodesQ) hipLaunchKernelGGL((k_trace_ws<COUNT, NC, true, false>), grid, block, 0, stream, sc, pb, rp.numSlots, rp.shardCapacity, parity, refill, rp.tailSlots);
    else hipLaunchKernelGGL((k_trace_ws<COUNT, NC, false, false>), grid, block, 0, stream, sc, pb, rp.numSlots, rp.shardCapacity, parity, refill, rp.tailSlots);
}
void launchTraceWs(const DevScene& sc, const PathBuffers& pb, const RenderParams& rp, uint32_t parity, uint32_t blocks, bool count,
                   hipStream_t stream) {
    blocks = (blocks + kShards - 1) / kShards * kShards;
    dispatchNc(wsConsumers(sc.nodesQ != nullptr), [&](auto nc) {
        if (count) launchTraceWsT<true, nc()>(sc, pb, rp, parity, blocks, stream);
        else launchTraceWsT<false, nc()>(sc, pb, rp, parity, blocks, stream);
    });
}

} // namespace slrhip
