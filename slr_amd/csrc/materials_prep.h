// materials_prep.h — the host half of slrhip_set_materials: every check on the new tables and every record derived from them, with no
// device call (see materials_prep.cpp).  The passes are prepareScene's own (scene_prep.h); slrhip_materials.hip uploads the result.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/slrhip.h"
#include "scene_prep.h"

namespace slrhip {

// The most lights for which the closed form of the light tables is the upload's Kahan chain bit for bit (pt_lights.h).
const uint32_t kMaxClosedFormLights = 1u << 24;

// What a context keeps of the scene in place for slrhip_set_materials: three facts per material about the triangles, the texture
// records (an update may not change an image's shape or any texture's kind), the number of image texels on the device.
struct MaterialsKept {
    MaterialUsage usage;
    std::vector<DevTexture> textures;
    uint64_t numTexTexels = 0;
    bool upsampling = false;                      // the Meng-15 tables are on the device
};

// The context as the checks see it.
struct MaterialsState {
    bool haveScene = false, geometryKept = false, hasEnv = false;
    const MaterialsKept* kept = nullptr;          // of the scene in place (haveScene)
};

// What the device half needs beyond the records.
struct MaterialsPlan {
    bool emittingChanged = false;                 // a material that triangles name starts or stops emitting: the light list is rebuilt
    uint32_t numLights = 0;
    std::vector<char> emitting;                   // per material, after the call
    std::vector<uint32_t> emitMask;               // the same, one bit per material
};

// The state a fresh upload of `d` would keep (prepareScene's material passes and histogram; no tree is built).  Returns SLRHIP_OK, or
// the upload's code and message for a descriptor those passes refuse.
int materialsKeptOf(const slrhip_scene_desc& d, bool spectral, MaterialsKept* out, std::string* err);

// Checks `desc` against the scene in place and derives the records: out->textures, matTex, materials, materialsS, spectra, spectrumPool,
// hasMicrofacet, hasMulti, and the shade-table blob packed for plan->numLights lights with the lights, PMF and CDF segments left zero
// (the device fills them).  Returns SLRHIP_OK, or an SLRHIP_ERR_* code with the message in *err ("slrhip_set_materials: ...").
int prepareMaterialsUpdate(const slrhip_materials_desc* desc, bool spectral, const MaterialsState& state, PreparedScene* out, MaterialsPlan* plan,
                           std::string* err);

} // namespace slrhip
