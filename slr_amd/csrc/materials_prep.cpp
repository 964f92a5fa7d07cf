// materials_prep.cpp — the host half of slrhip_set_materials (materials_prep.h): the new tables go through the passes of prepareScene
// that made the old ones (scene_prep.cpp: textures, the materials' textures, materials, spectra, the shade-table blob), then through the
// checks that only an update has: what the tree, the leaf records and the texel block were built for must stay.  Nothing here touches
// the device, so tables that fail a check leave the context as it was.
#include "materials_prep.h"

#include <cstring>

namespace slrhip {
namespace {

const char kUploadPrefix[] = "slrhip_upload_scene: ";
const char kPrefix[] = "slrhip_set_materials: ";

int refuse(std::string* err, int code, const std::string& what) {
    *err = kPrefix + what;
    return code;
}

// A pass of the upload refused: its code, and its message under this call's name.
int renamed(int rc, std::string* err) {
    if (err->compare(0, sizeof(kUploadPrefix) - 1, kUploadPrefix) == 0) err->replace(0, sizeof(kUploadPrefix) - 1, kPrefix);
    return rc;
}

#define UPLOAD_TRY(expr) do { if (const int rc_ = (expr)) return renamed(rc_, err); } while (0)

} // namespace

int materialsKeptOf(const slrhip_scene_desc& d, bool spectral, MaterialsKept* out, std::string* err) {
    if (!d.vertices || !d.triangles || !d.materials || !d.spectra || d.num_triangles == 0 || d.num_vertices == 0) {
        *err = std::string(kUploadPrefix) + "empty scene";
        return SLRHIP_ERR_INVALID_ARGUMENT;
    }
    for (uint32_t i = 0; i < d.num_triangles; ++i)
        if (d.triangles[i].material >= d.num_materials) {
            *err = std::string(kUploadPrefix) + "triangle index out of range";
            return SLRHIP_ERR_INVALID_ARGUMENT;
        }
    PreparedScene p;
    MaterialFacts facts;
    bool anyImage = false;
    if (const int rc = prepareTextures(d, spectral, nullptr, p, &anyImage, err)) return rc;
    if (const int rc = prepareMaterialTextures(d, p, facts, err)) return rc;
    if (const int rc = prepareMaterials(d, spectral, p, facts, err)) return rc;
    out->usage = materialUsage(d, facts);
    out->textures = p.textures;
    out->numTexTexels = p.texTexels.size() / 3u;
    out->upsampling = spectral && d.upsampling != nullptr;
    return SLRHIP_OK;
}

int prepareMaterialsUpdate(const slrhip_materials_desc* desc, bool spectral, const MaterialsState& state, PreparedScene* out, MaterialsPlan* plan,
                           std::string* err) {
    if (!desc) return refuse(err, SLRHIP_ERR_INVALID_ARGUMENT, "null argument");
    if (desc->reserved[0] || desc->reserved[1]) return refuse(err, SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_materials_desc::reserved must be 0");
    if (!state.haveScene || !state.kept) return refuse(err, SLRHIP_ERR_NO_SCENE, "no scene uploaded");
    const MaterialsKept& kept = *state.kept;
    const uint32_t numTextures = desc->textures ? desc->num_textures : 0u;
    if (!desc->materials || !desc->spectra) return refuse(err, SLRHIP_ERR_INVALID_ARGUMENT, "null material or spectrum table");
    if (desc->num_materials != kept.usage.triangles.size())
        return refuse(err, SLRHIP_ERR_INVALID_ARGUMENT, "num_materials differs from the uploaded scene's (triangles name materials by index)");
    if (numTextures != kept.textures.size())
        return refuse(err, SLRHIP_ERR_INVALID_ARGUMENT, "num_textures differs from the uploaded scene's (texture coordinates exist only for a scene with textures)");

    // the upload's passes over the new tables: its checks, codes and messages
    slrhip_scene_desc d;
    std::memset(&d, 0, sizeof(d));
    d.materials = desc->materials; d.num_materials = desc->num_materials;
    d.spectra = desc->spectra; d.num_spectra = desc->num_spectra;
    d.spectrum_data = desc->spectrum_data; d.num_spectrum_data = desc->num_spectrum_data;
    d.textures = desc->textures; d.num_textures = numTextures;
    PreparedScene& p = *out;
    MaterialFacts facts;
    bool anyImage = false;
    const KeptTexels texels = {kept.numTexTexels, kept.upsampling};
    UPLOAD_TRY(prepareTextures(d, spectral, &texels, p, &anyImage, err));
    UPLOAD_TRY(prepareMaterialTextures(d, p, facts, err));
    UPLOAD_TRY(prepareMaterials(d, spectral, p, facts, err));
    UPLOAD_TRY(prepareSpectra(d, spectral, p, err));

    // what the scene in place was built for
    for (uint32_t t = 0; t < numTextures; ++t) {
        const DevTexture &now = p.textures[t], &was = kept.textures[t];
        if (now.kind != was.kind) return refuse(err, SLRHIP_ERR_UNSUPPORTED, "a texture changes its kind");
        if (now.kind == SLRHIP_TEXTURE_IMAGE_SPECTRUM && (now.spec0 != was.spec0 || now.spec1 != was.spec1 || now.pad != was.pad))
            return refuse(err, SLRHIP_ERR_UNSUPPORTED, "an image texture changes its width, height or first texel");
    }
    const MaterialUsage& usage = kept.usage;
    for (uint32_t m = 0; m < desc->num_materials; ++m)
        if (facts.alphaOfMaterial[m] != usage.alpha[m])
            return refuse(err, SLRHIP_ERR_UNSUPPORTED, "a material's alpha map changes (the leaf records carry it)");
    uint64_t lights = 0;
    bool changed = false;
    for (uint32_t m = 0; m < desc->num_materials; ++m) {
        if (facts.emitting[m] && usage.instanced[m]) return refuse(err, SLRHIP_ERR_UNSUPPORTED, "instanced triangles must not emit");
        if (facts.emitting[m]) lights += usage.triangles[m];
        if (usage.triangles[m] && (facts.emitting[m] != 0) != (usage.emitting[m] != 0)) changed = true;
    }
    if (lights == 0 && !state.hasEnv) return refuse(err, SLRHIP_ERR_UNSUPPORTED, "scene has no emitting triangle and no environment light");
    if (lights > kMaxClosedFormLights) return refuse(err, SLRHIP_ERR_UNSUPPORTED, "more than 2^24 emitting triangles");
    if (changed && !state.geometryKept)
        return refuse(err, SLRHIP_ERR_UNSUPPORTED,
                      "the set of emitting materials changes, which needs the kept geometry (a context created with SLRHIP_FLAG_DYNAMIC_GEOMETRY and a scene "
                      "slrhip_set_vertices covers)");

    plan->emittingChanged = changed;
    plan->numLights = (uint32_t)lights;
    plan->emitting = facts.emitting;
    plan->emitMask.assign((desc->num_materials + 31u) / 32u, 0u);
    for (uint32_t m = 0; m < desc->num_materials; ++m)
        if (facts.emitting[m]) plan->emitMask[m >> 5] |= 1u << (m & 31u);

    // the blob, sized for the new list; the device writes its lights, PMF and CDF segments
    // (packShadeTables reads only the SIZES of the light arrays, and no size beyond kLdsLights is staged: a longer list stands in as
    // kLdsLights + 1 records, so that the host never holds millions of empty ones)
    const size_t standIn = std::min<size_t>(plan->numLights, (size_t)kLdsLights + 1u);
    LightTri none;
    std::memset(&none, 0, sizeof(none));
    p.lightTris.assign(standIn, none);
    p.lightPMF.assign(standIn, 0.0f);
    p.lightCDF.assign(standIn + 1u, 0.0f);
    p.lightIntegral = (float)plan->numLights;            // the Kahan sum of numLights ones: exact up to 2^24
    packShadeTables(spectral, p);
    return SLRHIP_OK;
}

} // namespace slrhip
