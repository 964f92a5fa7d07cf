// scene_prep.h — the host half of slrhip_upload_scene: every check on the descriptor and every record derived from it, with no
// device call and no context state (see scene_prep.cpp).  slrhip_api.hip uploads the result.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/slrhip.h"
#include "bvh.h"
#include "pt_kernels.h"

namespace slrhip {

enum class TreeBuild { Host, Device, Instanced };

struct PreparedScene {
    std::vector<DevTexture> textures;
    std::vector<float> texTexels;                 // the image textures' texels (3 floats each), empty unless one is in use
    std::vector<DevMatTex> matTex;
    std::vector<DevMaterial> materials;           // RGB mode
    std::vector<DevMaterialS> materialsS;         // spectral mode
    std::vector<DevSpectrum> spectra;             // spectral mode
    std::vector<float> spectrumPool;              // spectral mode: the sample data + the irregular spectra's 1-nm cell words, padded to float4
    bool hasMicrofacet = false, hasMulti = false;

    TreeBuild build = TreeBuild::Host;
    QBVH bvh;                                     // host and instanced builds: alpha records patched into the leaves
    std::vector<DevInstance> instances;
    bool quantized = false;                       // host build: upload bvh.quantized as well
    bool wantQuantized = false;                   // device build: ask for the quantized records (the tree could pass 64 Ki nodes)

    std::vector<ShadeTri> shadeTris;              // empty for the device build (it writes these records itself)
    std::vector<LightTri> lightTris;
    std::vector<uint32_t> lightTriangles;         // scene index of each light, in light-list order
    std::vector<float> lightPMF, lightCDF;
    float lightIntegral = 0.0f;

    std::vector<float4> triUV, alphaTris;         // per-triangle texture coordinates (scenes with textures); alpha records

    std::vector<float> envTexels, envTopPDF, envTopCDF, envRowPDF, envRowCDF;
    std::vector<uint8_t> gridCells;               // spectral mode, environment or image textures: the Meng-15 tables
    std::vector<float> pointUV, pointSpectrum;
    uint32_t gridWidth = 0, gridHeight = 0;

    DevCamera camera;

    std::vector<float4> shadeTables;              // DevScene::shadeTables, empty when the tables exceed the LDS limits
    bool tablesFit = false;
    uint32_t tableEnd[6] = {};
};

// The builder behind a prepared scene's tree, as include/slrhip_debug.h numbers them (SLRHIP_TREE_*): 0 host SAH, 1 host with spatial
// splits (the only build that counts references), 2 device, 3 instanced.
inline uint32_t treeBuilderOf(const PreparedScene& p) {
    if (p.build == TreeBuild::Instanced) return 3u;
    if (p.build == TreeBuild::Device) return 2u;
    return p.bvh.references ? 1u : 0u;
}

// Checks the descriptor and derives every host-side record.  Returns SLRHIP_OK, or an SLRHIP_ERR_* code with the message in *err.
int prepareScene(const slrhip_scene_desc& d, const slrhip_config& config, PreparedScene* out, std::string* err);

// The camera constants (PerspectiveCamera's constructor, libm on the host): slrhip_upload_scene's and slrhip_set_camera's.
DevCamera prepareCamera(const slrhip_camera& c);

// The traversal kernels' limits on a tree: 3 * depth + 1 entries on the 64-entry stack, nodes and leaf packets addressed with 32-bit
// byte offsets.  Returns SLRHIP_OK, or SLRHIP_ERR_UNSUPPORTED with *err = "slrhip_upload_scene: " + what (depth) or the size message.
int checkTreeLimits(uint32_t depth, uint64_t numNodes, uint64_t numLeafTris, const char* tooDeep, std::string* err);

// Trees beyond the L2 (>= 64 Ki nodes = 8 MiB) are also stored with 8-bit child boxes: half the bytes per node visit.
bool useQuantizedNodes(uint64_t numNodes);

} // namespace slrhip
