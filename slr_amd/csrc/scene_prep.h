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

// What the material pass learns about each material that later passes need.
struct MaterialFacts {
    std::vector<char> emitting;
    std::vector<int32_t> alphaOfMaterial;         // alpha texture of the material, -1 = none
    bool anyAlpha = false;
};

// What slrhip_set_materials needs to know about the triangles, per material (materialUsage): the context keeps it from the upload on.
struct MaterialUsage {
    std::vector<uint32_t> triangles;              // triangles that name the material
    std::vector<char> instanced;                  // ... one of them inside an instance's range
    std::vector<int32_t> alpha;                   // MaterialFacts::alphaOfMaterial
    std::vector<char> emitting;                   // MaterialFacts::emitting, as the context's light list stands
};

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

    MaterialUsage usage;                          // for slrhip_set_materials (materials_prep.h)
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

// ---- the passes of prepareScene that slrhip_set_materials runs again on new tables (materials_prep.cpp); messages and codes are the upload's ----
// The image textures' texels of a scene in place: how many there are and whether the Meng-15 tables are (they stay on the device).
struct KeptTexels { uint64_t numTexels; bool upsampling; };
// `kept` == nullptr: the texels and the tables are the descriptor's, and the texels are copied into p.texTexels.
int prepareTextures(const slrhip_scene_desc& d, bool spectral, const KeptTexels* kept, PreparedScene& p, bool* anyImageTexture, std::string* err);
int prepareMaterialTextures(const slrhip_scene_desc& d, PreparedScene& p, MaterialFacts& f, std::string* err);
int prepareMaterials(const slrhip_scene_desc& d, bool spectral, PreparedScene& p, MaterialFacts& f, std::string* err);
int prepareSpectra(const slrhip_scene_desc& d, bool spectral, PreparedScene& p, std::string* err);
// Packs p.shadeTables / tablesFit / tableEnd from the records and the light arrays of p (which it sizes the light segments by).
void packShadeTables(bool spectral, PreparedScene& p);
// The triangle histogram by material; the triangle and instance ranges have passed the descriptor checks.
MaterialUsage materialUsage(const slrhip_scene_desc& d, const MaterialFacts& f);

// The camera constants (PerspectiveCamera's constructor, libm on the host): slrhip_upload_scene's and slrhip_set_camera's.
DevCamera prepareCamera(const slrhip_camera& c);

// The traversal kernels' limits on a tree: 3 * depth + 1 entries on the 64-entry stack, nodes and leaf packets addressed with 32-bit
// byte offsets.  Returns SLRHIP_OK, or SLRHIP_ERR_UNSUPPORTED with *err = "slrhip_upload_scene: " + what (depth) or the size message.
int checkTreeLimits(uint32_t depth, uint64_t numNodes, uint64_t numLeafTris, const char* tooDeep, std::string* err);

// Trees beyond the L2 (>= 64 Ki nodes = 8 MiB) are also stored with 8-bit child boxes: half the bytes per node visit.
bool useQuantizedNodes(uint64_t numNodes);

} // namespace slrhip
