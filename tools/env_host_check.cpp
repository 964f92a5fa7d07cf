// tools/env_host_check.cpp — the two host exports of the environment preprocessing (slrhip_env_importance, slrhip_env_texels_to_uvs)
// in a stand-alone program, for a run under the host sanitizers:
//   hipcc -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Islr_amd/csrc \
//         tools/env_host_check.cpp slr_amd/csrc/host_util.cpp -o /tmp/env_host_check && /tmp/env_host_check
// Every buffer is exactly as large as the call may touch (heap blocks: a byte past either end is an AddressSanitizer report): a 4x4
// and an 8x4 image, the in-place conversion, and every refusal, which must write nothing.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/slrhip.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static std::vector<float> image(uint32_t w, uint32_t h) {
    std::vector<float> t((size_t)w * h * 3);
    uint32_t s = 12345u + w;
    for (float& v : t) { s = s * 1664525u + 1013904223u; v = (float)(s >> 20) * (1.0f / 512.0f); }      // multiples of 2^-9 below 8: halves
    t[0] = t[1] = t[2] = 0.0f;                                                                           // a black texel
    t[3] = 4094.0f; t[4] = 5.9604645e-8f; t[5] = 65504.0f;
    return t;
}

int main() {
    for (uint32_t w : {4u, 8u}) {
        const uint32_t h = 4, mw = w / 4, mh = h / 4;
        const std::vector<float> t = image(w, h);
        for (int32_t mode : {SLRHIP_MODE_RGB, SLRHIP_MODE_SPECTRAL}) {
            std::vector<float> imp((size_t)mw * mh, -1.0f);
            CHECK(slrhip_env_importance(mode, t.data(), w, h, imp.data(), imp.size()) == SLRHIP_OK);
            for (float v : imp) CHECK(std::isfinite(v) && v != -1.0f);
            std::vector<float> small(imp.size() - 1 + 1, -1.0f);
            CHECK(slrhip_env_importance(mode, t.data(), w, h, small.data(), imp.size() - 1) == SLRHIP_ERR_INVALID_ARGUMENT);
            CHECK(small[0] == -1.0f);
        }
        std::vector<float> uvs(t.size(), -1.0f), inPlace = t;
        CHECK(slrhip_env_texels_to_uvs(t.data(), (size_t)w * h, uvs.data()) == SLRHIP_OK);
        CHECK(slrhip_env_texels_to_uvs(inPlace.data(), (size_t)w * h, inPlace.data()) == SLRHIP_OK);
        CHECK(std::memcmp(uvs.data(), inPlace.data(), uvs.size() * sizeof(float)) == 0);
        CHECK(uvs[2] == 0.0f && std::isfinite(uvs[0]) && std::isfinite(uvs[1]));                         // the black texel: x = y = 1/3
        std::vector<float> imp((size_t)mw * mh);
        CHECK(slrhip_env_importance(SLRHIP_MODE_SPECTRAL, uvs.data(), w, h, imp.data(), imp.size()) == SLRHIP_OK);
    }
    float one = -1.0f;
    const std::vector<float> t = image(8, 4);
    CHECK(slrhip_env_importance(SLRHIP_MODE_RGB, nullptr, 4, 4, &one, 1) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_importance(SLRHIP_MODE_RGB, t.data(), 4, 4, nullptr, 1) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_importance(SLRHIP_MODE_RGB, t.data(), 6, 4, &one, 1) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_importance(SLRHIP_MODE_RGB, t.data(), 4, 0, &one, 1) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_importance(SLRHIP_MODE_RGB, t.data(), 32772, 4, &one, 1) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_importance(7, t.data(), 4, 4, &one, 1) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_texels_to_uvs(nullptr, 1, &one) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(slrhip_env_texels_to_uvs(t.data(), 1, nullptr) == SLRHIP_ERR_INVALID_ARGUMENT);
    CHECK(one == -1.0f);
    std::printf(failures ? "%d checks FAILED\n" : "env_host_check: all checks passed\n", failures);
    return failures ? 1 : 0;
}
