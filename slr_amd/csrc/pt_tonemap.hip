// pt_tonemap.hip — device code of slrhip_tonemap: the image export defined in include/slrhip.h, one launch.  gfx950, wave64.
//
// One thread takes FOUR horizontally adjacent pixels of one image row.  A row of the BMP layout is 3 * width + width % 4 bytes, a
// multiple of four, and `output` is 4-byte aligned, so every row starts on a dword and a thread's 12 bytes do too: it stores three
// dwords (RGBA8: four) and no single byte.  The thread that holds a row's last n = width % 4 pixels (n != 0) owns 3 * n colour bytes
// and the row's n zero padding bytes: exactly n dwords.  The colours are read as float4s; the caller's pointers are only 4-byte
// aligned (and a row of 3 * width floats starts anywhere), so the vector types below carry that alignment: gfx950 takes a dword-aligned
// global_load_dwordx4 / global_store_dwordx3.
//
// The arithmetic is pt_tonemap.h's, shared with the host export; this file supplies the two library calls in double (the OCML exp and
// pow) and is built with -ffp-contract=off like the rest.
#include "../../include/slrhip.h"
#include "pt_kernels.h"
#include "pt_tonemap.h"

namespace slrhip {

namespace {

typedef float Float4A4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t Uint3A4 __attribute__((ext_vector_type(3), aligned(4)));
typedef uint32_t Uint4A4 __attribute__((ext_vector_type(4), aligned(4)));

struct DeviceTonemapMath {
    static __device__ __forceinline__ float expNeg(float Y) { return (float)::exp((double)(-Y)); }
    static __device__ __forceinline__ double gammaPow(float value) { return ::pow((double)value, 1.0 / 2.4); }
};

struct Tonemap {
    uint32_t width, height, groups, numThreads;      // groups = ceil(width / 4) threads per row; numThreads = groups * height
    float scale;
    size_t rowBytes;                                 // of the output (4 * width does not fit 32 bits for every width)
    const float* color;
    uint8_t* output;
};

template <int C, bool kBmp>
__global__ __launch_bounds__(256) void k_tonemap(Tonemap a) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.numThreads) return;
    const uint32_t row = t / a.groups, x0 = (t - row * a.groups) * 4u;
    const uint32_t n = a.width - x0 < 4u ? a.width - x0 : 4u;                 // pixels of this thread: 4, or the row's last 1 .. 3
    const float* src = a.color + ((size_t)row * a.width + x0) * C;

    float c[4 * C];
    if (n == 4u) {
#pragma unroll
        for (int j = 0; j < C; ++j) {                                         // 4 pixels x C floats = C float4s in a row
            const Float4A4 v = *reinterpret_cast<const Float4A4*>(src + 4 * j);
            c[4 * j] = v.x; c[4 * j + 1] = v.y; c[4 * j + 2] = v.z; c[4 * j + 3] = v.w;
        }
    }
    else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int b = 0; b < C; ++b) c[k * C + b] = (uint32_t)k < n ? src[k * C + b] : 0.0f;      // nothing is read past the row
        }
#pragma unroll
        for (int b = 0; b < C; ++b) c[3 * C + b] = 0.0f;
    }

    uint32_t px[4];                                                           // B | G << 8 | R << 16 of each pixel; 0 past the row
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint8_t bgr[3];
        tonemapPixel<C, DeviceTonemapMath>(c + k * C, a.scale, bgr);
        px[k] = (uint32_t)k < n ? (uint32_t)bgr[0] | (uint32_t)bgr[1] << 8 | (uint32_t)bgr[2] << 16 : 0u;
    }

    if (kBmp) {
        // bytes B0 G0 R0 B1 | G1 R1 B2 G2 | R2 B3 G3 R3; with n < 4 the bytes behind pixel n - 1 are the row's padding, zero
        uint8_t* dst = a.output + (a.height - 1u - row) * a.rowBytes + (size_t)x0 * 3u;
        const uint32_t d0 = px[0] | px[1] << 24, d1 = px[1] >> 8 | px[2] << 16, d2 = px[2] >> 16 | px[3] << 8;
        if (n == 4u) *reinterpret_cast<Uint3A4*>(dst) = Uint3A4{d0, d1, d2};
        else {
            uint32_t* o = reinterpret_cast<uint32_t*>(dst);
            o[0] = d0;
            if (n >= 2u) o[1] = d1;
            if (n == 3u) o[2] = d2;
        }
    }
    else {
        uint8_t* dst = a.output + row * a.rowBytes + (size_t)x0 * 4u;
        uint32_t q[4];                                                        // R | G << 8 | B << 16 | 255 << 24
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = (px[k] >> 16) | (px[k] & 0xFF00u) | (px[k] & 0xFFu) << 16 | 0xFF000000u;
        if (n == 4u) *reinterpret_cast<Uint4A4*>(dst) = Uint4A4{q[0], q[1], q[2], q[3]};
        else {
            uint32_t* o = reinterpret_cast<uint32_t*>(dst);
            o[0] = q[0];
            if (n >= 2u) o[1] = q[1];
            if (n == 3u) o[2] = q[2];
        }
    }
}

} // namespace

void launchTonemap(const slrhip_tonemap_desc& d, hipStream_t stream) {
    Tonemap a;
    a.width = d.width; a.height = d.height;
    a.groups = (d.width + 3u) / 4u;
    a.numThreads = a.groups * d.height;                    // <= width * height < 2^31 (checked by the caller)
    const bool bmp = d.format == SLRHIP_IMAGE_BGR8_BMP;
    a.rowBytes = bmp ? (size_t)3u * d.width + d.width % 4u : (size_t)4u * d.width;
    a.scale = d.scale; a.color = d.color; a.output = d.output;
    const dim3 grid((a.numThreads + 255u) / 256u), block(256);               // < 2^23 + 1 blocks
    if (d.components == 3) {
        if (bmp) hipLaunchKernelGGL((k_tonemap<3, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_tonemap<3, false>), grid, block, 0, stream, a);
    }
    else {
        if (bmp) hipLaunchKernelGGL((k_tonemap<16, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_tonemap<16, false>), grid, block, 0, stream, a);
    }
}

} // namespace slrhip
