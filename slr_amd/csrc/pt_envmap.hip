// pt_envmap.hip — device code of slrhip_set_environment: the environment texels are stored, and the importance map and the 2-D
// sampling distribution are built from them where they are.  gfx950, wave64.  Five launches in stream order:
//
//   k_env_store       copies the caller's texels into the context's array, with the optional binary16 rounding and the (r, g, b) ->
//                     (u, v, s) conversion.  Pure streaming: a thread takes FOUR texels = 48 contiguous bytes, three 16-byte loads
//                     and three 16-byte stores (the width is a multiple of 4 and both bases are 16-byte aligned).
//   k_env_importance  one lane per map cell.  The four rows of a cell's 4x4 block are 48 contiguous, 16-byte aligned bytes each: three
//                     16-byte loads per row, consecutive lanes read consecutive 48-byte pieces.  It reads the STORED texels.
//   k_env_rows        one lane owns one row of the map and walks it in index order: the sequential Kahan chain IS the definition
//                     (RegularConstantContinuous1D), so it is not replaced by a scan.  Neighbouring lanes read addresses a whole row
//                     apart, so a wave stages 64-row x 64-column tiles through LDS with coalesced loads and stores; a tile row is
//                     padded to 65 dwords, which puts lane l's element c on bank (l + c) mod 32: the per-lane walk (ds_read_b32 /
//                     ds_write_b32: 32 banks, conflicts counted per 32-lane half) is conflict-free.  The walk leaves the running
//                     sums in the tile, which is stored as the unnormalised row CDF; the next tile is fetched into registers
//                     before the walk, so its loads are in flight while the chain runs.  The row's integral goes to topPDF.
//   k_env_normalise   one lane per map cell: the row PDF and the row CDF divided by the row's integral.
//   k_env_top       one workgroup: the rows' integrals go to LDS, ONE lane runs the same chain over them, every lane divides.
//
// No atomics.  The arithmetic is pt_envmap.h's, shared with the host (slrhip_env_importance, slrhip_env_texels_to_uvs,
// prepareEnvironment); this file is built with -ffp-contract=off like the rest, and it calls no library function: the sines of the
// rows come from the host (EnvBuild::sinRow).
#include <hip/hip_runtime.h>

#include "pt_envmap.h"

namespace slrhip {

namespace {

const uint32_t kEnvTile = 64;                // rows of a workgroup of k_env_rows (one wave) and columns of a tile
const uint32_t kEnvPitch = kEnvTile + 1;     // dwords per tile row in LDS

template <bool kHalf, bool kUvs>
__global__ __launch_bounds__(256) void k_env_store(const float4* __restrict__ src, float4* __restrict__ dst, size_t groups) {
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= groups) return;                                                  // groups = width * height / 4: nothing is read past the image
    const float4 q0 = src[3 * t], q1 = src[3 * t + 1], q2 = src[3 * t + 2];
    float v[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    if (kHalf) {
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = envHalf(v[k]);
    }
    if (kUvs) {
#pragma unroll
        for (int k = 0; k < 4; ++k) envRgbToUvs(v[3 * k], v[3 * k + 1], v[3 * k + 2], v[3 * k], v[3 * k + 1], v[3 * k + 2]);
    }
    dst[3 * t] = make_float4(v[0], v[1], v[2], v[3]);
    dst[3 * t + 1] = make_float4(v[4], v[5], v[6], v[7]);
    dst[3 * t + 2] = make_float4(v[8], v[9], v[10], v[11]);
}

template <bool kSpectral>
__global__ __launch_bounds__(256) void k_env_importance(const float* __restrict__ texels, float* __restrict__ importance, uint32_t width,
                                                        uint32_t mapWidth, uint32_t numCells) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= numCells) return;
    const uint32_t my = t / mapWidth, mx = t - my * mapWidth;
    float b[3][16];                                                           // b[component][4 y + x]
#pragma unroll
    for (int y = 0; y < 4; ++y) {
        const float4* row = reinterpret_cast<const float4*>(texels + ((size_t)(4u * my + y) * width + 4u * mx) * 3u);
        const float4 q0 = row[0], q1 = row[1], q2 = row[2];
        const float v[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int x = 0; x < 4; ++x) {
#pragma unroll
            for (int c = 0; c < 3; ++c) b[c][4 * y + x] = v[3 * x + c];
        }
    }
    const float a0 = envAreaAverage(b[0]), a1 = envAreaAverage(b[1]), a2 = envAreaAverage(b[2]);
    importance[t] = kSpectral ? envImportanceUVS(a0, a1, a2) : envImportanceRGB(a0, a1, a2);
}

// Column x0 + lane of the tile's 64 rows into registers (zero past the map): 64 independent coalesced loads.
__device__ __forceinline__ void envFetchTile(const EnvBuild& e, uint32_t y0, uint32_t rows, uint32_t x0, uint32_t lane, float (&v)[kEnvTile]) {
    const bool inside = x0 + lane < e.mapWidth;
#pragma unroll
    for (uint32_t r = 0; r < kEnvTile; ++r) v[r] = inside && r < rows ? e.importance[(size_t)(y0 + r) * e.mapWidth + x0 + lane] : 0.0f;
}

__global__ __launch_bounds__(kEnvTile) void k_env_rows(EnvBuild e) {
    __shared__ float tile[kEnvTile * kEnvPitch];
    const uint32_t lane = threadIdx.x, y0 = blockIdx.x * kEnvTile, y = y0 + lane;
    const uint32_t mw = e.mapWidth, mh = e.mapHeight;
    const uint32_t rows = mh - y0 < kEnvTile ? mh - y0 : kEnvTile;            // the grid is ceil(mh / 64): y0 < mh
    const bool mine = y < mh;
    const double sinRow = mine ? e.sinRow[y] : 0.0;

    // the chain: lane `lane` walks row y; the tiles pass through LDS both ways, and the next tile's loads are in flight during the walk
    float next[kEnvTile];
    envFetchTile(e, y0, rows, 0, lane, next);
    EnvSum sum;
    for (uint32_t x0 = 0; x0 < mw; x0 += kEnvTile) {
        const uint32_t cols = mw - x0 < kEnvTile ? mw - x0 : kEnvTile;
#pragma unroll
        for (uint32_t r = 0; r < kEnvTile; ++r) tile[r * kEnvPitch + lane] = next[r];
        __syncthreads();
        if (x0 + kEnvTile < mw) envFetchTile(e, y0, rows, x0 + kEnvTile, lane, next);
        if (mine)
            for (uint32_t c = 0; c < cols; ++c) {
                float* cell = &tile[lane * kEnvPitch + c];
                *cell = envCdfStep(sum, envRowValue(sinRow, *cell), mw);
            }
        __syncthreads();
        if (lane < cols)
            for (uint32_t r = 0; r < rows; ++r) e.rowCDF[(size_t)(y0 + r) * (mw + 1u) + x0 + lane + 1u] = tile[r * kEnvPitch + lane];
        __syncthreads();                                                      // the next tile's loads overwrite this one
    }
    if (mine) {
        e.topPDF[y] = sum.result;                                             // the row's integral: k_env_normalise's and k_env_top's input
        e.rowCDF[(size_t)y * (mw + 1u)] = 0.0f;
    }
}

// The division by the row's integral (still unnormalised in topPDF: k_env_top runs after this): one lane per cell.
__global__ __launch_bounds__(256) void k_env_normalise(EnvBuild e) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x, mw = e.mapWidth;
    if (t >= mw * e.mapHeight) return;
    const uint32_t y = t / mw, x = t - y * mw;
    const float total = e.topPDF[y];
    e.rowPDF[t] = envRowValue(e.sinRow[y], e.importance[t]) / total;
    const size_t k = (size_t)y * (mw + 1u) + x + 1u;
    e.rowCDF[k] = e.rowCDF[k] / total;
}

__global__ __launch_bounds__(256) void k_env_top(EnvBuild e) {
    __shared__ float vals[kEnvMaxMapSide];
    __shared__ float total;
    const uint32_t mh = e.mapHeight;                                          // <= kEnvMaxMapSide (environmentRefusal)
    for (uint32_t i = threadIdx.x; i < mh; i += 256u) vals[i] = e.topPDF[i];
    __syncthreads();
    if (threadIdx.x == 0) {
        EnvSum sum;
        for (uint32_t i = 0; i < mh; ++i) vals[i] = envCdfStep(sum, vals[i], mh);
        total = sum.result;
        e.topCDF[0] = 0.0f;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < mh; i += 256u) {
        e.topPDF[i] = e.topPDF[i] / total;
        e.topCDF[i + 1u] = vals[i] / total;
    }
}

} // namespace

void launchEnvBuild(const EnvBuild& e, hipStream_t stream) {
    const size_t groups = (size_t)e.width * e.height / 4u;                    // <= 2^28
    const dim3 storeGrid((uint32_t)((groups + 255u) / 256u)), block(256);
    const float4* src = reinterpret_cast<const float4*>(e.src);
    float4* dst = reinterpret_cast<float4*>(e.texels);
    if (e.storeHalf) {
        if (e.toUvs) hipLaunchKernelGGL((k_env_store<true, true>), storeGrid, block, 0, stream, src, dst, groups);
        else hipLaunchKernelGGL((k_env_store<true, false>), storeGrid, block, 0, stream, src, dst, groups);
    }
    else {
        if (e.toUvs) hipLaunchKernelGGL((k_env_store<false, true>), storeGrid, block, 0, stream, src, dst, groups);
        else hipLaunchKernelGGL((k_env_store<false, false>), storeGrid, block, 0, stream, src, dst, groups);
    }
    const uint32_t numCells = e.mapWidth * e.mapHeight;                       // <= 2^26
    const dim3 cellGrid((numCells + 255u) / 256u);
    if (e.spectral) hipLaunchKernelGGL((k_env_importance<true>), cellGrid, block, 0, stream, e.texels, e.importance, e.width, e.mapWidth, numCells);
    else hipLaunchKernelGGL((k_env_importance<false>), cellGrid, block, 0, stream, e.texels, e.importance, e.width, e.mapWidth, numCells);
    hipLaunchKernelGGL(k_env_rows, dim3((e.mapHeight + kEnvTile - 1u) / kEnvTile), dim3(kEnvTile), 0, stream, e);
    hipLaunchKernelGGL(k_env_normalise, cellGrid, block, 0, stream, e);
    hipLaunchKernelGGL(k_env_top, dim3(1), block, 0, stream, e);
}

} // namespace slrhip
