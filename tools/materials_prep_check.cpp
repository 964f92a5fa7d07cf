// materials_prep_check.cpp — the host half of slrhip_set_materials (slr_amd/csrc/materials_prep.cpp: the checks, the triangle facts, the
// packing of the shade tables) driven from a plain program, so that it can run under the host sanitizers without a GPU or Python:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -ffp-contract=off tools/materials_prep_check.cpp \
//       slr_amd/csrc/{materials_prep,scene_prep,bvh,sbvh,host_util}.cpp -fsanitize=address,undefined -lpthread -o materials_prep_check
//
// (tools/materials_prep_check.sh does that and runs it; the sanitizers instrument the host side only.)  Exit status 0 and "materials_prep_check: ok" when every expectation holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../slr_amd/csrc/materials_prep.h"

using namespace slrhip;

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what); ++failures; }
}

struct Tables {
    std::vector<slrhip_material> materials;
    std::vector<slrhip_spectrum> spectra;
    std::vector<float> data;
    std::vector<slrhip_texture> textures;
    slrhip_materials_desc desc() const {
        slrhip_materials_desc d;
        std::memset(&d, 0, sizeof(d));
        d.materials = materials.data(); d.num_materials = (uint32_t)materials.size();
        d.spectra = spectra.data(); d.num_spectra = (uint32_t)spectra.size();
        d.spectrum_data = data.data(); d.num_spectrum_data = (uint32_t)data.size();
        d.textures = textures.data(); d.num_textures = (uint32_t)textures.size();
        return d;
    }
};

slrhip_material matte(int32_t spectrum, int32_t emittance = -1, uint32_t reserved = 0) {
    slrhip_material m;
    std::memset(&m, 0, sizeof(m));
    m.type = SLRHIP_MATERIAL_MATTE; m.spectrum[0] = spectrum; m.spectrum[1] = m.spectrum[2] = -1; m.param = -1.0f; m.emittance = emittance; m.reserved = reserved;
    return m;
}

int check(const Tables& t, bool spectral, const MaterialsState& s, MaterialsPlan* plan, PreparedScene* p, std::string* err) {
    const slrhip_materials_desc d = t.desc();
    return prepareMaterialsUpdate(&d, spectral, s, p, plan, err);
}

} // namespace

int main() {
    // 40 triangles over 4 vertices: material i % 4, the last 8 inside an instance; material 3 emits; material 2 has an alpha map
    std::vector<slrhip_vertex> vertices(4);
    std::memset(vertices.data(), 0, vertices.size() * sizeof(slrhip_vertex));
    vertices[1].position[0] = 1.0f; vertices[2].position[1] = 1.0f; vertices[3].position[2] = 1.0f;
    std::vector<slrhip_triangle> triangles(40);
    for (uint32_t i = 0; i < 40; ++i) { triangles[i] = slrhip_triangle{{0, 1, 2 + (i & 1u)}, i < 32 ? i % 4u : i % 2u}; }
    Tables t;
    t.spectra.resize(3);
    std::memset(t.spectra.data(), 0, 3 * sizeof(slrhip_spectrum));
    for (int k = 0; k < 3; ++k) { t.spectra[k].kind = SLRHIP_SPECTRUM_REGULAR; t.spectra[k].num_samples = 4; t.spectra[k].data_offset = 4u * k; t.spectra[k].scale = 1.0f;
                                  t.spectra[k].lambda_min = 360.0f; t.spectra[k].lambda_max = 830.0f; t.spectra[k].rgb[0] = t.spectra[k].rgb[1] = t.spectra[k].rgb[2] = 0.5f; }
    t.data.assign(12, 0.5f);
    t.textures.resize(2);
    std::memset(t.textures.data(), 0, 2 * sizeof(slrhip_texture));
    t.textures[0].kind = SLRHIP_TEXTURE_CHECKER_FLOAT; t.textures[0].scale[0] = t.textures[0].scale[1] = 1.0f; t.textures[0].value[0] = 1.0f;
    t.textures[1].kind = SLRHIP_TEXTURE_IMAGE_SPECTRUM; t.textures[1].scale[0] = t.textures[1].scale[1] = 1.0f;
    t.textures[1].reserved[0] = 2; t.textures[1].reserved[1] = 3; t.textures[1].reserved[2] = 1;
    t.materials = {matte(0), matte(SLRHIP_TEXTURE_REF(1)), matte(1, -1, SLRHIP_MATERIAL_ALPHA_MAP(0)), matte(1, 2)};
    std::vector<float> texels(7 * 3, 0.25f);
    slrhip_instance inst;
    std::memset(&inst, 0, sizeof(inst));
    inst.first_triangle = 32; inst.num_triangles = 8;
    for (int k = 0; k < 4; ++k) inst.local_to_world[5 * k] = inst.world_to_local[5 * k] = 1.0f;

    slrhip_scene_desc scene;
    std::memset(&scene, 0, sizeof(scene));
    scene.vertices = vertices.data(); scene.num_vertices = 4; scene.triangles = triangles.data(); scene.num_triangles = 40;
    scene.materials = t.materials.data(); scene.num_materials = 4; scene.spectra = t.spectra.data(); scene.num_spectra = 3;
    scene.spectrum_data = t.data.data(); scene.num_spectrum_data = 12; scene.textures = t.textures.data(); scene.num_textures = 2;
    scene.texture_texels = texels.data(); scene.num_texture_texels = 7; scene.instances = &inst; scene.num_instances = 1;

    std::string err;
    MaterialsKept kept;
    expect(materialsKeptOf(scene, false, &kept, &err) == SLRHIP_OK, "the facts of the uploaded scene");
    expect(kept.usage.triangles == std::vector<uint32_t>({12, 12, 8, 8}), "the triangle histogram");
    expect(kept.usage.instanced == std::vector<char>({1, 1, 0, 0}), "the instanced bits");
    expect(kept.usage.alpha == std::vector<int32_t>({-1, -1, 0, -1}), "the alpha maps");
    expect(kept.usage.emitting == std::vector<char>({0, 0, 0, 1}), "the emitting set");
    expect(kept.numTexTexels == 7 && kept.textures.size() == 2, "the texture shapes");

    MaterialsState have;
    have.haveScene = true; have.kept = &kept;
    for (const bool spectral : {false, true}) {
        MaterialsPlan plan;
        PreparedScene p;
        expect(check(t, false, have, &plan, &p, &err) == SLRHIP_OK && !plan.emittingChanged && plan.numLights == 8 && p.tablesFit, "the uploaded tables go ahead");
        expect(p.tableEnd[5] == p.shadeTables.size() && p.lightTris.size() == 8, "the blob's segments end at its end");
        (void)spectral;
    }
    {   // the same in spectral mode, with the Meng-15 tables said to be in place
        MaterialsKept ks = kept;
        ks.upsampling = true;
        MaterialsState s = have;
        s.kept = &ks;
        MaterialsPlan plan;
        PreparedScene p;
        expect(check(t, true, s, &plan, &p, &err) == SLRHIP_OK && p.tablesFit && p.tableEnd[5] == p.shadeTables.size(), "spectral tables go ahead");
        p = PreparedScene();
        expect(check(t, true, have, &plan, &p, &err) == SLRHIP_ERR_INVALID_ARGUMENT, "spectral image textures need the tables");
    }
    const auto refused = [&](const Tables& tables, const MaterialsState& s, int code, const char* message) {
        MaterialsPlan plan;
        PreparedScene p;
        std::string e;
        const int rc = check(tables, false, s, &plan, &p, &e);
        expect(rc == code && e.rfind("slrhip_set_materials: ", 0) == 0 && e.find(message) != std::string::npos, message);
    };
    {
        MaterialsPlan plan;
        PreparedScene p;
        expect(prepareMaterialsUpdate(nullptr, false, have, &p, &plan, &err) == SLRHIP_ERR_INVALID_ARGUMENT, "null descriptor");
        slrhip_materials_desc d = t.desc();
        d.reserved[1] = 1;
        expect(prepareMaterialsUpdate(&d, false, have, &p, &plan, &err) == SLRHIP_ERR_INVALID_ARGUMENT, "reserved");
    }
    refused(t, MaterialsState(), SLRHIP_ERR_NO_SCENE, "no scene uploaded");
    Tables u = t;
    u.materials.pop_back();
    refused(u, have, SLRHIP_ERR_INVALID_ARGUMENT, "num_materials differs");
    u = t; u.textures.pop_back();
    refused(u, have, SLRHIP_ERR_INVALID_ARGUMENT, "num_textures differs");
    u = t; u.textures[1].reserved[0] = 1;
    refused(u, have, SLRHIP_ERR_UNSUPPORTED, "width, height or first texel");
    u = t; u.textures[1].reserved[2] = 2;
    refused(u, have, SLRHIP_ERR_INVALID_ARGUMENT, "image texture outside");
    u = t; u.textures[1].kind = SLRHIP_TEXTURE_CHECKER_SPECTRUM; u.textures[1].spectrum[0] = 0; u.textures[1].spectrum[1] = 1;
    refused(u, have, SLRHIP_ERR_UNSUPPORTED, "changes its kind");
    u = t; u.materials[2].reserved = 0;
    refused(u, have, SLRHIP_ERR_UNSUPPORTED, "alpha map changes");
    u = t; u.materials[0].emittance = 2;
    refused(u, have, SLRHIP_ERR_UNSUPPORTED, "instanced triangles must not emit");
    u = t; u.materials[3].emittance = -1;
    refused(u, have, SLRHIP_ERR_UNSUPPORTED, "no emitting triangle and no environment light");
    u = t; u.materials[2].emittance = 2;
    refused(u, have, SLRHIP_ERR_UNSUPPORTED, "the set of emitting materials changes");
    u = t; u.materials[0].spectrum[0] = 3;
    refused(u, have, SLRHIP_ERR_INVALID_ARGUMENT, "spectrum index out of range");
    {
        MaterialsState s = have;
        s.geometryKept = true;
        MaterialsPlan plan;
        PreparedScene p;
        u = t; u.materials[2].emittance = 2;
        expect(check(u, false, s, &plan, &p, &err) == SLRHIP_OK && plan.emittingChanged && plan.numLights == 16 && p.tablesFit && plan.emitMask == std::vector<uint32_t>({12u}),
               "sixteen lights fit");
        s.hasEnv = true;
        u = t; u.materials[3].emittance = -1;
        p = PreparedScene();                                  // (a call fills a fresh one)
        expect(check(u, false, s, &plan, &p, &err) == SLRHIP_OK && plan.numLights == 0 && p.lightCDF.size() == 1 && p.tablesFit, "an environment stands in for the last light");
        // more lights than the staged tables hold: the stand-in records keep the host from holding them all
        MaterialsKept big = kept;
        big.usage.triangles = {12, 12, 8, 1u << 24};
        s.kept = &big;
        p = PreparedScene();
        expect(check(t, false, s, &plan, &p, &err) == SLRHIP_OK && plan.numLights == (1u << 24) && !p.tablesFit && p.shadeTables.empty() && p.lightTris.size() == 17, "2^24 lights");
        big.usage.triangles[3] += 1;
        std::string e;
        p = PreparedScene();
        expect(check(t, false, s, &plan, &p, &e) == SLRHIP_ERR_UNSUPPORTED && e.find("2^24") != std::string::npos, "more than 2^24 lights");
    }
    if (failures) return 1;
    std::puts("materials_prep_check: ok");
    return 0;
}
