// pt_toplevel.hip — device code of slrhip_rebuild_top_level: the top-level primitives (instance leaves and loose-triangle packets)
// sorted by the Morton code of their box centres (pt_toplevel.h: the key, same bits as the host's) and seated in that order into the
// leaf slots of the tree as it stands.  gfx950, wave64.  The call is bound by launch latency, so the launch count is what is
// designed for.  Launches in stream order:
//
//   at most kTopSeatGroup primitives — ONE launch:
//   k_top_seat_group  ONE workgroup of 1024 lanes, primitive p = lane + 1024 j.  Boxes through the canonical references (two
//                     16-byte loads a primitive); the scene box by a reduction (wave shuffles, then sixteen partial boxes through
//                     LDS; min and max are exact, so the order they are taken in does not matter); (key, index) pairs into LDS,
//                     padded to a power of two with a sentinel above every 63-bit key; a bitonic network over the PAIRS (ties by
//                     index: the stable order); then one lane per slot stores one child word and six planes.
//   more — three launches:
//   k_top_keys        one lane per primitive; the scene box is the union of the root's valid child boxes (uploads and refits keep
//                     unions exact: the same bits as a reduction over the primitives), seven 16-byte loads at one address a wave.
//   a device radix sort of (key, index) pairs over bits 0 .. 63 (hipcub; stable), into `order`
//   k_top_seat        one lane per slot.
//
// The refit of pt_instances.hip follows either path.  No atomics, no flags between workgroups, no hand-off inside a launch between
// workgroups: the order comes from the launches.  Only leaf child words and child planes of the first topNodes nodes are stored
// (4-byte vector stores); an inner child's word is never a slot.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "pt_instance.h"
#include "pt_toplevel.h"

namespace slrhip {

namespace {

struct PrimBox { float lo[3], hi[3]; };

// primitive p < s.count of the canonical order
__device__ __forceinline__ PrimBox primitiveBox(const TopSeat& s, uint32_t p) {
    const float4* src = p < s.numInstances ? s.instBoxes + 2u * (size_t)p : s.packetBoxes + 2u * (size_t)(p - s.numInstances);
    const float4 a = src[0], b = src[1];
    return PrimBox{{a.x, a.y, a.z}, {b.x, b.y, b.z}};
}

// slot i < s.count receives primitive p < s.count
__device__ __forceinline__ void seat(const TopSeat& s, uint32_t i, uint32_t p) {
    const uint32_t slot = s.slots[i], node = slot >> 2, c = slot & 3u;
    if (node >= s.topNodes) return;                                           // (never: the plan walked the first topNodes nodes)
    const PrimBox b = primitiveBox(s, p);
    float* planes = reinterpret_cast<float*>(s.nodes + (size_t)node * 8u);    // minx[4] miny[4] minz[4] maxx[4] maxy[4] maxz[4] child[4] pad[4]
    planes[c] = b.lo[0]; planes[4u + c] = b.lo[1]; planes[8u + c] = b.lo[2];
    planes[12u + c] = b.hi[0]; planes[16u + c] = b.hi[1]; planes[20u + c] = b.hi[2];
    reinterpret_cast<uint32_t*>(planes)[24u + c] = s.refs[p];
}

__device__ __forceinline__ float waveMin(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fminf(v, __shfl_xor(v, d));
    return v;
}
__device__ __forceinline__ float waveMax(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}

__global__ __launch_bounds__(kTopSeatBlock) void k_top_seat_group(TopSeat s) {
    __shared__ uint64_t sKey[kTopSeatGroup];
    __shared__ uint32_t sIdx[kTopSeatGroup];
    __shared__ float sPart[kTopSeatBlock / 64u][6];
    const uint32_t t = threadIdx.x, n = s.count;                              // n <= kTopSeatGroup (launchTopSeat)
    constexpr uint32_t kPer = kTopSeatGroup / kTopSeatBlock;
    PrimBox box[kPer];
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t p = t + kTopSeatBlock * j;
        if (p < n) {
            box[j] = primitiveBox(s, p);
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], box[j].lo[a]); hi[a] = fmaxf(hi[a], box[j].hi[a]); }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = waveMin(lo[a]); hi[a] = waveMax(hi[a]); }
    if ((t & 63u) == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { sPart[t >> 6][a] = lo[a]; sPart[t >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
    for (uint32_t w = 0; w < kTopSeatBlock / 64u; ++w) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], sPart[w][a]); hi[a] = fmaxf(hi[a], sPart[w][3 + a]); }
    }
    uint32_t padded = 64u;                                                    // a power of two >= n, <= kTopSeatGroup
    while (padded < n) padded <<= 1;
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t p = t + kTopSeatBlock * j;
        if (p < padded) {
            uint64_t key = ~0ull;                                             // the sentinel: above every 63-bit key
            if (p < n) { key = topLevelKey(box[j].lo, box[j].hi, lo, hi); s.keys[p] = key; }
            sKey[p] = key; sIdx[p] = p;
        }
    }
    __syncthreads();
    // bitonic network over (key, index) pairs, ascending; every lane reaches every barrier
    for (uint32_t k = 2u; k <= padded; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t q = t; q < (padded >> 1); q += kTopSeatBlock) {
                const uint32_t i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), m = i | j;      // the pair (i, i + j) of compare q
                const uint64_t ka = sKey[i], kb = sKey[m];
                const uint32_t ia = sIdx[i], ib = sIdx[m];
                const bool up = (i & k) == 0u;
                const bool greater = ka > kb || (ka == kb && ia > ib);
                if (greater == up) { sKey[i] = kb; sKey[m] = ka; sIdx[i] = ib; sIdx[m] = ia; }
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < kPer; ++j) {
        const uint32_t i = t + kTopSeatBlock * j;
        if (i < n) {
            const uint32_t p = sIdx[i];                                       // the sentinels sort behind every primitive: p < n
            s.order[i] = p;
            if (p < n) seat(s, i, p);
        }
    }
}

__global__ __launch_bounds__(256) void k_top_keys(TopSeat s) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= s.count) return;
    const float4* root = s.nodes;
    const float4 p0 = root[0], p1 = root[1], p2 = root[2], p3 = root[3], p4 = root[4], p5 = root[5];
    const uint4 refs = *reinterpret_cast<const uint4*>(root + 6);
    const float lo[3] = {unionMin(p0, refs), unionMin(p1, refs), unionMin(p2, refs)};
    const float hi[3] = {unionMax(p3, refs), unionMax(p4, refs), unionMax(p5, refs)};
    const PrimBox b = primitiveBox(s, p);
    s.keys[p] = topLevelKey(b.lo, b.hi, lo, hi);
}

__global__ __launch_bounds__(256) void k_top_seat(TopSeat s) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= s.count) return;
    const uint32_t p = s.order[i];
    if (p < s.count) seat(s, i, p);
}

} // namespace

size_t topSeatSortBytes(uint32_t count) {
    size_t bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)count, 0, 64,
                                           (hipStream_t)nullptr) != hipSuccess)
        return 0;
    return bytes ? bytes : 1;
}

uint32_t launchTopSeat(const TopSeat& s, hipStream_t stream, hipError_t* err) {
    *err = hipSuccess;
    if (s.count <= kTopSeatGroup) {
        hipLaunchKernelGGL(k_top_seat_group, dim3(1), dim3(kTopSeatBlock), 0, stream, s);
        return 1;
    }
    const uint32_t blocks = (s.count + 255u) / 256u;
    hipLaunchKernelGGL(k_top_keys, dim3(blocks), dim3(256), 0, stream, s);
    size_t bytes = s.sortTempBytes;
    *err = hipcub::DeviceRadixSort::SortPairs(s.sortTemp, bytes, (const uint64_t*)s.keys, s.sortedKeys, (const uint32_t*)s.identity, s.order, (int)s.count, 0, 64, stream);
    if (*err != hipSuccess) return 0;
    hipLaunchKernelGGL(k_top_seat, dim3(blocks), dim3(256), 0, stream, s);
    return 3;
}

} // namespace slrhip
