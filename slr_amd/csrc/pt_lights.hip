// pt_lights.hip — device code of slrhip_set_materials and slrhip_set_texture_texels.  gfx950, wave64.  Launches in stream order (a
// launch reads what earlier launches stored; nothing is handed between workgroups inside one):
//
//   k_lights_count    one lane per triangle, 256 per workgroup: one 16-byte load of the index record gives its material; the emitting
//                     bit comes from the mask of one bit per material, staged once per workgroup in LDS (up to kLightsMaskLds words;
//                     a larger mask is read from memory).  A ballot and a population count per wave, the four wave counts added in
//                     wave order: the workgroup's count.
//   k_lights_scan     one workgroup turns the counts into exclusive offsets, in chunks of 256 (pt_adaptive.hip's scan), and stores
//                     the total behind them.
//   k_lights_scatter  the same ballot again.  rank = the workgroup's offset + the waves before + the lanes before in the ballot: the
//                     rank of an emitting triangle among the emitting triangles in triangle order, as prepareTriangles numbers them.
//                     EVERY triangle stores ShadeTri::light (rank or -1: one word, the rest of the record stays); an emitting one also
//                     stores its index and its material into LightTri[rank].  A rank at or beyond numLights stores nothing (never: the
//                     host's count is the histogram's).
//   (k_geometry_lights of pt_geometry.hip then fills the light records from the kept vertices, in both copies.)
//   k_light_tables    one lane per entry: PMF[i] = 1 / n, CDF[i] = i / n (pt_lights.h), into the arrays and the staged segments.
//   k_texels_store    one lane per texel: three 4-byte loads, three stores (a texture's first texel is a multiple of 12 bytes only).
//
// No atomics, no flags between workgroups: the order comes from the triangle index and from the launches.  Vector stores only.
#include "pt_lights.h"

#include "pt_envmap.h"

namespace slrhip {

namespace {

// The mask as this workgroup reads it: staged in `lds` (every lane takes part, then a barrier) or left in memory.
__device__ __forceinline__ const uint32_t* stageMask(const LightsUpdate& u, uint32_t* lds) {
    if (u.maskWords > kLightsMaskLds) return u.emitMask;                     // uniform over the launch
    for (uint32_t w = threadIdx.x; w < u.maskWords; w += kLightsBlock) lds[w] = u.emitMask[w];
    __syncthreads();
    return lds;
}

// Triangle i (any i) emits: its material's bit.  A material beyond the table (never: the upload checked) does not.
__device__ __forceinline__ bool emits(const LightsUpdate& u, const uint32_t* mask, uint32_t i, uint32_t& material) {
    material = 0u;
    if (i >= u.numTriangles) return false;
    material = reinterpret_cast<const uint4*>(u.triangles)[i].w;            // v[3], material
    if (material >= u.numMaterials) return false;
    return ((mask[material >> 5] >> (material & 31u)) & 1u) != 0u;
}

__global__ __launch_bounds__(kLightsBlock) void k_lights_count(LightsUpdate u) {
    __shared__ uint32_t lds[kLightsMaskLds];
    __shared__ uint32_t waves[kLightsBlock / 64];
    const uint32_t* mask = stageMask(u, lds);
    uint32_t material;
    const bool on = emits(u, mask, blockIdx.x * kLightsBlock + threadIdx.x, material);
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63u) == 0u) waves[threadIdx.x >> 6] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kLightsBlock / 64; ++w) t += waves[w];
        u.offsets[blockIdx.x] = t;
    }
}

// Exclusive scan of offsets[0 .. numBlocks) in place by ONE workgroup, chunk after chunk on top of the carry (Hillis-Steele in LDS);
// offsets[numBlocks] = the total.
__global__ __launch_bounds__(kLightsBlock) void k_lights_scan(uint32_t* __restrict__ offsets, uint32_t numBlocks) {
    __shared__ uint32_t buf[2][kLightsBlock];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < numBlocks; base += kLightsBlock) {        // uniform over the workgroup: every lane reaches every barrier
        const uint32_t b = base + threadIdx.x;
        const uint32_t own = b < numBlocks ? offsets[b] : 0u;
        uint32_t cur = 0;
        buf[0][threadIdx.x] = own;
        __syncthreads();
        for (uint32_t off = 1; off < kLightsBlock; off <<= 1) {
            const uint32_t v = buf[cur][threadIdx.x] + (threadIdx.x >= off ? buf[cur][threadIdx.x - off] : 0u);
            buf[cur ^ 1u][threadIdx.x] = v;
            cur ^= 1u;
            __syncthreads();
        }
        const uint32_t inclusive = buf[cur][threadIdx.x];
        const uint32_t chunkTotal = buf[cur][kLightsBlock - 1];
        if (b < numBlocks) offsets[b] = carry + inclusive - own;
        carry += chunkTotal;
        __syncthreads();                       // buf is rewritten by the next chunk
    }
    if (threadIdx.x == 0) offsets[numBlocks] = carry;
}

__global__ __launch_bounds__(kLightsBlock) void k_lights_scatter(LightsUpdate u) {
    __shared__ uint32_t lds[kLightsMaskLds];
    __shared__ uint32_t waves[kLightsBlock / 64];
    const uint32_t* mask = stageMask(u, lds);
    const uint32_t i = blockIdx.x * kLightsBlock + threadIdx.x;
    uint32_t material;
    const bool on = emits(u, mask, i, material);
    const uint64_t m = __ballot(on);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) waves[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (i >= u.numTriangles) return;
    uint32_t rank = u.offsets[blockIdx.x];
    for (uint32_t w = 0; w < wave; ++w) rank += waves[w];
    rank += (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    const bool light = on && rank < u.numLights;
    reinterpret_cast<int32_t*>(u.shadeTris + (size_t)i * 6u + 1u)[3] = light ? (int32_t)rank : -1;
    if (!light) return;
    uint32_t* rec = reinterpret_cast<uint32_t*>(u.lightTris + (size_t)rank * 9u);
    rec[3] = i;                                                              // [0].w
    rec[7] = material;                                                       // [1].w
}

__global__ __launch_bounds__(256) void k_light_tables(LightsUpdate u) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = u.numLights;
    if (i > n) return;
    const float c = n ? __fdiv_rn((float)i, (float)n) : 0.0f;
    u.cdf[i] = c;
    if (u.stagedCdf) u.stagedCdf[i] = c;
    if (i == n) return;
    const float p = __fdiv_rn(1.0f, (float)n);
    u.pmf[i] = p;
    if (u.stagedPmf) u.stagedPmf[i] = p;
}

__global__ __launch_bounds__(256) void k_texels_store(const float* __restrict__ src, float* __restrict__ dst, uint32_t count, bool half) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const float* s = src + (size_t)t * 3u;
    float a = s[0], b = s[1], c = s[2];
    if (half) { a = envHalf(a); b = envHalf(b); c = envHalf(c); }
    float* d = dst + (size_t)t * 3u;
    d[0] = a; d[1] = b; d[2] = c;
}

} // namespace

uint32_t launchLightsRebuild(const LightsUpdate& u, hipStream_t stream) {
    if (!u.rebuild || u.numTriangles == 0) return 0u;
    const uint32_t blocks = lightsBlocks(u.numTriangles);
    hipLaunchKernelGGL(k_lights_count, dim3(blocks), dim3(kLightsBlock), 0, stream, u);
    hipLaunchKernelGGL(k_lights_scan, dim3(1), dim3(kLightsBlock), 0, stream, u.offsets, blocks);
    hipLaunchKernelGGL(k_lights_scatter, dim3(blocks), dim3(kLightsBlock), 0, stream, u);
    return 3u;
}

uint32_t launchLightTables(const LightsUpdate& u, hipStream_t stream) {
    hipLaunchKernelGGL(k_light_tables, dim3((u.numLights + 1u + 255u) / 256u), dim3(256), 0, stream, u);
    return 1u;
}

void launchTexelsStore(const float* src, float* dst, uint32_t count, bool half, hipStream_t stream) {
    if (count) hipLaunchKernelGGL(k_texels_store, dim3((count + 255u) / 256u), dim3(256), 0, stream, src, dst, count, half);
}

} // namespace slrhip
