// scene_prep.cpp — the host half of slrhip_upload_scene (scene_prep.h).
//
// Host-side responsibilities that the reference spreads over SurfaceObjectAggregate's constructor (Core/SurfaceObject.cpp:226-250:
// accelerator + light list), Scene::build (:396-406) and PerspectiveCamera's constructor (Cameras/PerspectiveCamera.cpp:15-24):
// check the descriptor, flatten it into the device records, build the tree.  Nothing here touches the device, so a descriptor that
// fails a check leaves the context as it was.  Built with -ffp-contract=off like bvh.cpp: the Oren-Nayar constants, face normals,
// areas, camera constants and Kahan sums round exactly as the reference's scalar code.
#include "scene_prep.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "pt_envmap.h"
#include "pt_triangle.h"

namespace slrhip {
namespace {

#define PREP_TRY(expr) do { if (const int rc_ = (expr)) return rc_; } while (0)

int reject(std::string* err, int code, const std::string& what) {
    *err = "slrhip_upload_scene: " + what;
    return code;
}

// Kahan sum, BasicTypes/CompensatedSum.h:24-30
struct KahanF {
    float result = 0.0f, comp = 0.0f;
    void add(float value) {
        float cInput = value - comp;
        float sumTemp = result + cInput;
        comp = (sumTemp - result) - cInput;
        result = sumTemp;
    }
};

// --- the descriptor's own consistency: sizes, the Meng-15 tables, the environment map, triangle indices ------------------------
int checkDescriptor(const slrhip_scene_desc& d, bool spectral, std::string* err) {
    if (!d.vertices || !d.triangles || !d.materials || !d.spectra || d.num_triangles == 0 || d.num_vertices == 0)
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "empty scene");
    // the Meng-15 tables, wherever they are given: the kernels index with these bytes
    if (spectral && d.upsampling) {
        const slrhip_upsampling_tables* t = d.upsampling;
        if (!t->cells || !t->point_uv || !t->point_spectrum || t->grid_width == 0 || t->grid_height == 0 || t->num_points == 0 || t->num_points > 255)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "incomplete slrhip_scene_desc::upsampling");
        for (size_t c = 0; c < (size_t)t->grid_width * t->grid_height; ++c) {
            const uint8_t* cell = t->cells + c * 8;
            if (cell[1] > 6) return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "upsampling cell with more than 6 points");
            for (int k = 0; k < (cell[0] ? 4 : cell[1]); ++k)
                if (cell[2 + k] >= t->num_points) return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "upsampling point index out of range");
        }
    }
    if (d.env) {
        const slrhip_envmap& e = *d.env;
        if (spectral && !d.upsampling)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "an environment map in spectral mode needs slrhip_scene_desc::upsampling");
        if (!e.texels || !e.importance || e.width == 0 || e.height == 0 || e.map_width == 0 || e.map_height == 0 ||
            e.width > 32768 || e.height > 32768 || e.map_width > 32768 || e.map_height > 32768)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "bad environment map");
    }
    // a bad index would fault the GPU
    for (uint32_t i = 0; i < d.num_triangles; ++i) {
        const slrhip_triangle& t = d.triangles[i];
        if (t.v[0] >= d.num_vertices || t.v[1] >= d.num_vertices || t.v[2] >= d.num_vertices || t.material >= d.num_materials)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "triangle index out of range");
    }
    return SLRHIP_OK;
}

} // namespace

// --- textures: checkerboard spectrum / float / normal textures, image textures --------------------------------
int prepareTextures(const slrhip_scene_desc& d, bool spectral, const KeptTexels* kept, PreparedScene& p, bool* anyImageTexture, std::string* err) {
    const bool haveTexels = kept ? kept->numTexels != 0 : d.texture_texels != nullptr;
    const uint64_t numTexels = kept ? kept->numTexels : d.num_texture_texels;
    const bool haveUpsampling = kept ? kept->upsampling : d.upsampling != nullptr;
    const uint32_t numTextures = d.textures ? d.num_textures : 0u;
    if (numTextures > 32767u) return reject(err, SLRHIP_ERR_UNSUPPORTED, "more than 32767 textures");
    p.textures.resize(numTextures);
    for (uint32_t i = 0; i < numTextures; ++i) {
        const slrhip_texture& t = d.textures[i];
        DevTexture dt;
        std::memset(&dt, 0, sizeof(dt));
        dt.kind = t.kind; dt.ox = t.offset[0]; dt.oy = t.offset[1]; dt.sx = t.scale[0]; dt.sy = t.scale[1];
        dt.v0 = t.value[0]; dt.v1 = t.value[1]; dt.spec0 = dt.spec1 = -1;
        if (t.kind == SLRHIP_TEXTURE_CHECKER_SPECTRUM) {
            for (int k = 0; k < 2; ++k) {
                if (t.spectrum[k] < 0 || (uint32_t)t.spectrum[k] >= d.num_spectra)
                    return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "texture names a spectrum out of range");
                if (spectral && d.spectra[t.spectrum[k]].kind == SLRHIP_SPECTRUM_RGB_ONLY)
                    return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "spectral mode needs a spectral descriptor for every spectrum in use");
            }
            dt.spec0 = t.spectrum[0]; dt.spec1 = t.spectrum[1];
            for (int c = 0; c < 3; ++c) { dt.rgb0[c] = d.spectra[t.spectrum[0]].rgb[c]; dt.rgb1[c] = d.spectra[t.spectrum[1]].rgb[c]; }
        }
        else if (t.kind == SLRHIP_TEXTURE_CHECKER_NORMAL) {
            if (!(t.value[0] > 0.0f && t.value[0] <= 1.0f))        // SLRAssert of the reference's constructor
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "checkerboard normal texture needs stepWidth in (0, 1]");
        }
        else if (t.kind == SLRHIP_TEXTURE_IMAGE_SPECTRUM) {
            // ImageSpectrumTexture: width, height and the first texel travel in the record (DevTexture, device_types.h)
            const uint64_t w = t.reserved[0], h = t.reserved[1], first = t.reserved[2];
            if (w == 0 || h == 0 || w > 65535 || h > 65535 || !haveTexels || first + w * h > numTexels)
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "image texture outside slrhip_scene_desc::texture_texels");
            if (spectral && !haveUpsampling)
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "image textures in spectral mode need slrhip_scene_desc::upsampling");
            dt.spec0 = (int32_t)w; dt.spec1 = (int32_t)h; dt.pad = (uint32_t)first;
            *anyImageTexture = true;
        }
        else if (t.kind != SLRHIP_TEXTURE_CHECKER_FLOAT) return reject(err, SLRHIP_ERR_UNSUPPORTED, "unknown texture kind");
        p.textures[i] = dt;
    }
    if (*anyImageTexture && !kept) p.texTexels.assign(d.texture_texels, d.texture_texels + (size_t)d.num_texture_texels * 3);
    return SLRHIP_OK;
}

// The textures each material names: normal map, alpha map, textured spectrum slots.
int prepareMaterialTextures(const slrhip_scene_desc& d, PreparedScene& p, MaterialFacts& f, std::string* err) {
    const uint32_t numTextures = (uint32_t)p.textures.size();
    p.matTex.resize(d.num_materials);
    f.alphaOfMaterial.assign(d.num_materials, -1);
    for (uint32_t i = 0; i < d.num_materials; ++i) {
        const slrhip_material& m = d.materials[i];
        DevMatTex mt = {{-1, -1, -1}, -1};
        const uint32_t nmap = m.reserved & 0xFFFFu, amap = m.reserved >> 16;
        if (nmap > numTextures || amap > numTextures) return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "material names a texture out of range");
        if (nmap) {
            if (d.textures[nmap - 1].kind != SLRHIP_TEXTURE_CHECKER_NORMAL) return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "a normal map must be a CHECKER_NORMAL texture");
            mt.normalMap = (int32_t)nmap - 1;
        }
        if (amap) {
            if (d.textures[amap - 1].kind != SLRHIP_TEXTURE_CHECKER_FLOAT) return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "an alpha map must be a CHECKER_FLOAT texture");
            f.alphaOfMaterial[i] = (int32_t)amap - 1;
            f.anyAlpha = true;
        }
        if (m.emittance < -1) return reject(err, SLRHIP_ERR_UNSUPPORTED, "textured emittance is not supported");
        for (int k = 0; k < 3 && m.type != SLRHIP_MATERIAL_MULTI; ++k) {
            if (m.spectrum[k] >= -1) continue;
            const uint32_t t = (uint32_t)(-2 - m.spectrum[k]);
            if (t >= numTextures || (d.textures[t].kind != SLRHIP_TEXTURE_CHECKER_SPECTRUM && d.textures[t].kind != SLRHIP_TEXTURE_IMAGE_SPECTRUM))
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "material spectrum slot names a texture that is not a spectrum texture");
            mt.slot[k] = (int32_t)t;
        }
        p.matTex[i] = mt;
    }
    return SLRHIP_OK;
}

namespace {

// MultiBSDF of two earlier materials — single lobes, or MULTI records of single lobes (include/slrhip.h); the record carries
// indices, scales, flags
int multiMaterial(const slrhip_scene_desc& d, uint32_t i, bool spectral, DevMaterial& dm, std::string* err) {
    const slrhip_material& m = d.materials[i];
    if ((uint32_t)m.spectrum[2] > 3u)
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "MULTI material with unknown inverse bits");
    uint32_t childType[2];
    for (int k = 0; k < 2; ++k) {
        if (m.spectrum[k] < 0 || (uint32_t)m.spectrum[k] >= i)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "MULTI component must be an earlier entry of the material table");
        if ((uint32_t)m.spectrum[k] > kMultiMaxChildIndex)
            return reject(err, SLRHIP_ERR_UNSUPPORTED, "MULTI component index beyond 1023");
        const slrhip_material& cmat = d.materials[m.spectrum[k]];
        childType[k] = cmat.type;
        if (childType[k] == SLRHIP_MATERIAL_MULTI) {
            // one level of nesting: the components of a component are single lobes (four lobes in all, the reference's
            // MultiBSDF::maxNumElems); an InverseBSDF over a MultiBSDF is not supported
            if (d.materials[cmat.spectrum[0]].type >= SLRHIP_MATERIAL_MULTI || d.materials[cmat.spectrum[1]].type >= SLRHIP_MATERIAL_MULTI)
                return reject(err, SLRHIP_ERR_UNSUPPORTED, "MULTI materials nest one level deep (at most four lobes)");
            if ((m.spectrum[2] >> k) & 1)
                return reject(err, SLRHIP_ERR_UNSUPPORTED, "inverse of a MULTI component is not supported");
        }
        if (((m.spectrum[2] >> k) & 1) && (childType[k] == SLRHIP_MATERIAL_GLASS || childType[k] == SLRHIP_MATERIAL_MICROFACET_GLASS))
            return reject(err, SLRHIP_ERR_UNSUPPORTED, "inverse of a two-sided lobe (glass, microfacet glass) is not supported");
    }
    if (m.emittance >= 0 && (uint32_t)m.emittance >= d.num_spectra)
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "spectrum index out of range");
    if (spectral && m.emittance >= 0 && d.spectra[m.emittance].kind == SLRHIP_SPECTRUM_RGB_ONLY)
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "spectral mode needs a spectral descriptor for every spectrum in use");
    dm.param = 1.0f * m.param;          // `scale * (1.0f - factor)` / `scale * factor` with scale = 1 (MixedSurfaceMaterial.cpp:16-17)
    dm.onA = 1.0f * m.param2;
    const uint32_t bits = packMultiBits((uint32_t)m.spectrum[0], (uint32_t)m.spectrum[1], (uint32_t)m.spectrum[2], childType[0], childType[1]);
    std::memcpy(&dm.onB, &bits, sizeof(bits));
    if (m.emittance >= 0)
        for (int k = 0; k < 3; ++k) dm.emittance[k] = d.spectra[m.emittance].rgb[k];
    return SLRHIP_OK;
}

// A single lobe: its scalars and its constant spectra, resolved to RGB values.
int singleMaterial(const slrhip_scene_desc& d, const slrhip_material& m, DevMaterial& dm, std::string* err) {
    if (m.type == SLRHIP_MATERIAL_WARD || m.type == SLRHIP_MATERIAL_ASHIKHMIN) {
        dm.onA = m.param2;          // the lobe's second scalar travels in the Oren-Nayar slot (unused by these types)
        if (!(m.param > 0.0f) || !(m.param2 > 0.0f))
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "Ward / Ashikhmin need param > 0 and param2 > 0");
    }
    if (m.type == SLRHIP_MATERIAL_MATTE && m.param >= 0.0f) {
        // OrenNayerBRDF ctor, OrenNayerBRDF.h:28-30: double literals in a float expression
        const float sigma = m.param;
        dm.onA = (float)(1.0f - 0.5f * sigma * sigma / (sigma * sigma + 0.33));
        dm.onB = (float)(0.45 * sigma * sigma / (sigma * sigma + 0.09));
    }
    if ((m.type == SLRHIP_MATERIAL_MICROFACET_METAL || m.type == SLRHIP_MATERIAL_MICROFACET_GLASS) && !(m.param > 0.0f))
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "microfacet material needs alpha_g > 0");
    auto fetch = [&](int32_t idx, float* dst) -> bool {
        if (idx < 0) return true;
        if ((uint32_t)idx >= d.num_spectra) return false;
        for (int k = 0; k < 3; ++k) dst[k] = d.spectra[idx].rgb[k];   // RGBTemplate::evaluate RGBTypes.h:124-126
        return true;
    };
    // `scale * spectrum` with scale = 1.0f (basic_SurfaceMaterials.cpp:22,33,42) is exact
    if (!fetch(m.spectrum[0], dm.a) || !fetch(m.spectrum[1], dm.b) || !fetch(m.spectrum[2], dm.c) || !fetch(m.emittance, dm.emittance))
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "spectrum index out of range");
    if (m.spectrum[0] == -1 && m.type <= SLRHIP_MATERIAL_GLASS)
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "material without its first spectrum");
    if (m.type == SLRHIP_MATERIAL_ASHIKHMIN && (m.spectrum[0] == -1 || m.spectrum[1] == -1))
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "Ashikhmin needs Rs and Rd");
    if (m.type == SLRHIP_MATERIAL_WARD && m.spectrum[0] == -1)
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "Ward needs R");
    if (m.type >= SLRHIP_MATERIAL_METAL && m.type <= SLRHIP_MATERIAL_MICROFACET_GLASS && (m.spectrum[1] == -1 || m.spectrum[2] == -1))
        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "material without its eta / k spectra");
    return SLRHIP_OK;
}

// The spectral-mode record of a material: its scalars and the spectrum indices a, b, c, emittance (-1 = unused).
DevMaterialS spectralRecord(const DevMaterial& dm, int32_t a, int32_t b, int32_t c, int32_t emittance) {
    DevMaterialS ds;
    ds.type = dm.type; ds.param = dm.param; ds.onA = dm.onA; ds.onB = dm.onB;
    ds.spec[0] = a; ds.spec[1] = b; ds.spec[2] = c; ds.spec[3] = emittance;
    return ds;
}

} // namespace

// --- materials: one record per mode ----------------------------------------------------------------------------------------------
int prepareMaterials(const slrhip_scene_desc& d, bool spectral, PreparedScene& p, MaterialFacts& f, std::string* err) {
    p.materials.resize(d.num_materials);
    p.materialsS.resize(d.num_materials);
    f.emitting.assign(d.num_materials, 0);
    for (uint32_t i = 0; i < d.num_materials; ++i) {
        const slrhip_material& m = d.materials[i];
        DevMaterial dm;
        std::memset(&dm, 0, sizeof(dm));
        dm.type = m.type;
        dm.param = m.param;
        if (m.type > SLRHIP_MATERIAL_MULTI)
            return reject(err, SLRHIP_ERR_UNSUPPORTED, "unknown material type");
        if (m.type == SLRHIP_MATERIAL_MULTI) {
            PREP_TRY(multiMaterial(d, i, spectral, dm, err));
            p.materialsS[i] = spectralRecord(dm, -1, -1, -1, m.emittance);
        }
        else {
            PREP_TRY(singleMaterial(d, m, dm, err));
            p.materialsS[i] = spectralRecord(dm, m.spectrum[0], m.spectrum[1], m.spectrum[2], m.emittance);
            if (spectral)
                for (int k = 0; k < 4; ++k)
                    if (p.materialsS[i].spec[k] >= 0 && d.spectra[p.materialsS[i].spec[k]].kind == SLRHIP_SPECTRUM_RGB_ONLY)
                        return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "spectral mode needs a spectral descriptor for every spectrum in use");
        }
        f.emitting[i] = m.emittance >= 0;
        p.materials[i] = dm;
    }
    for (uint32_t i = 0; i < d.num_materials; ++i) {
        const DevMatTex& mt = p.matTex[i];
        if (mt.slot[0] >= 0 || mt.slot[1] >= 0 || mt.slot[2] >= 0 || mt.normalMap >= 0) { p.materials[i].type |= kMatTexturedBit; p.materialsS[i].type |= kMatTexturedBit; }
    }
    for (const DevMaterial& dm : p.materials) {
        if ((dm.type & 0xFFu) >= SLRHIP_MATERIAL_MICROFACET_METAL) p.hasMicrofacet = true;     // GGX, Ward, Ashikhmin: the kernels with the glossy-lobe code
        if ((dm.type & 0xFFu) == SLRHIP_MATERIAL_MULTI) p.hasMulti = true;
    }
    return SLRHIP_OK;
}

// --- spectrum table (spectral mode): descriptors + the float pool, bounds-checked here because the kernels index it ---------------
int prepareSpectra(const slrhip_scene_desc& d, bool spectral, PreparedScene& p, std::string* err) {
    p.spectra.resize(d.num_spectra);
    for (uint32_t i = 0; i < d.num_spectra && spectral; ++i) {
        const slrhip_spectrum& sp = d.spectra[i];
        DevSpectrum ds;
        std::memset(&ds, 0, sizeof(ds));
        ds.kind = sp.kind; ds.numPoints = sp.reserved; ds.numSamples = sp.num_samples; ds.dataOffset = sp.data_offset;
        ds.scale = sp.scale; ds.lambdaMin = sp.lambda_min; ds.lambdaMax = sp.lambda_max;
        ds.cellOffset = 0xFFFFFFFFu;
        size_t need = 0;
        if (sp.kind == SLRHIP_SPECTRUM_REGULAR) need = sp.num_samples;
        else if (sp.kind == SLRHIP_SPECTRUM_IRREGULAR) need = 2 * (size_t)sp.num_samples;
        else if (sp.kind == SLRHIP_SPECTRUM_UPSAMPLED) need = 4 + 4 * (size_t)sp.num_samples;
        if (sp.kind != SLRHIP_SPECTRUM_RGB_ONLY) {
            if (sp.num_samples < 2 || (size_t)sp.data_offset + need > d.num_spectrum_data || !d.spectrum_data)
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "spectrum data out of range");
            if (sp.kind == SLRHIP_SPECTRUM_UPSAMPLED && sp.data_offset % 4 != 0)
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "upsampled spectrum payload must start at a multiple of 4 floats");
            if (sp.kind == SLRHIP_SPECTRUM_UPSAMPLED && sp.reserved != 0 && sp.reserved != 3 && sp.reserved != 4)
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "upsampled spectrum must resolve to 0, 3 or 4 points");
        }
        p.spectra[i] = ds;
    }
    std::vector<float>& pool = p.spectrumPool;
    if (spectral && d.spectrum_data) pool.assign(d.spectrum_data, d.spectrum_data + d.num_spectrum_data);
    // Irregular spectra are evaluated with std::lower_bound per wavelength (SpectrumTypes.h:143-146): on the GPU that is a
    // chain of dependent loads per component.  A path's wavelengths lie in [360, 830], so for every 1-nm cell the host
    // stores lower_bound(cell start) as one byte: the device starts there and walks at most a step or two — the same index.
    for (uint32_t i = 0; i < d.num_spectra && spectral; ++i) {
        const slrhip_spectrum& sp = d.spectra[i];
        if (sp.kind != SLRHIP_SPECTRUM_IRREGULAR || sp.num_samples > 255) continue;
        while (pool.size() % 4) pool.push_back(0.0f);
        const float* lambdas = d.spectrum_data + sp.data_offset;
        const uint32_t cells = 472;                                   // 360 + j, j = 0 .. 471
        std::vector<uint32_t> words(cells / 4, 0u);
        for (uint32_t j = 0; j < cells; ++j) {
            const float start = 360.0f + (float)j;
            const uint32_t lb = (uint32_t)(std::lower_bound(lambdas, lambdas + sp.num_samples, start) - lambdas);
            words[j / 4] |= lb << (8 * (j % 4));
        }
        p.spectra[i].cellOffset = (uint32_t)pool.size();
        for (uint32_t w : words) { float f; std::memcpy(&f, &w, 4); pool.push_back(f); }
    }
    while (pool.size() % 4) pool.push_back(0.0f);          // the shade kernel stages the pool into LDS 16 bytes at a time
    return SLRHIP_OK;
}

// --- what slrhip_set_materials needs to know about the triangles: a histogram by material ---------------------------------------
MaterialUsage materialUsage(const slrhip_scene_desc& d, const MaterialFacts& f) {
    MaterialUsage u;
    u.triangles.assign(d.num_materials, 0u);
    u.instanced.assign(d.num_materials, 0);
    u.alpha = f.alphaOfMaterial;
    u.emitting = f.emitting;
    for (uint32_t i = 0; i < d.num_triangles; ++i) ++u.triangles[d.triangles[i].material];
    for (uint32_t k = 0; k < (d.instances ? d.num_instances : 0u); ++k) {
        const slrhip_instance& in = d.instances[k];
        for (uint32_t t = 0; t < in.num_triangles && (uint64_t)in.first_triangle + t < d.num_triangles; ++t)
            u.instanced[d.triangles[in.first_triangle + t].material] = 1;
    }
    return u;
}

namespace {

// --- accelerator -------------------------------------------------------------------------------------------------------------------
// Host build (binned SAH, bvh.cpp / spatial splits, sbvh.cpp) unless the context asks for the device build (bvh_device.hip: LBVH,
// the same collapse; for scenes of millions of triangles, where the host build takes seconds).  The device build also writes the
// per-triangle records on the GPU; it does not cover alpha-textured triangles (their leaf entries are patched on the host).
int prepareTree(const slrhip_scene_desc& d, const slrhip_config& config, const MaterialFacts& f, PreparedScene& p, std::string* err) {
    static const std::string envBuild = [] { const char* e = getenv("SLRHIP_BVH"); return std::string(e ? e : ""); }();      // "host" / "device": override
    // automatic: from 2^20 triangles on (host build of 10 M triangles: 2.9 s on 16 cores; device: 0.13 s, traversal 5 % slower)
    const bool wantDevice = envBuild == "device" || (config.flags & SLRHIP_FLAG_BVH_DEVICE_BUILD) != 0 ||
                            (envBuild != "host" && envBuild != "sbvh" && !(config.flags & SLRHIP_FLAG_BVH_SPATIAL_SPLITS) && d.num_triangles >= (1u << 20));
    const uint32_t numInstances = d.instances ? d.num_instances : 0u;
    if (numInstances) {
        // instanced meshes (TransformedSurfaceObject, Core/SurfaceObject.cpp:303-392): two-level tree in one node array (bvh.h)
        p.build = TreeBuild::Instanced;
        for (uint32_t k = 0; k < numInstances; ++k) {
            const slrhip_instance& in = d.instances[k];
            if (in.num_triangles == 0 || (uint64_t)in.first_triangle + in.num_triangles > d.num_triangles)
                return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "instance names triangles out of range");
            for (uint32_t t = 0; t < in.num_triangles; ++t)
                if (f.emitting[d.triangles[in.first_triangle + t].material])
                    return reject(err, SLRHIP_ERR_UNSUPPORTED, "instanced triangles must not emit");
        }
        std::string why;
        if (buildInstancedQBVH(d.vertices, d.triangles, d.num_triangles, d.instances, numInstances, &p.bvh, &p.instances, &why) != 0)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, why);
        PREP_TRY(checkTreeLimits(p.bvh.depth, p.bvh.nodes.size(), p.bvh.leafTris.size(), "two-level tree deeper than the 64-entry traversal stack (QBVH.h:299)", err));
    }
    else if (wantDevice && !f.anyAlpha && d.num_triangles >= 1024) {
        p.build = TreeBuild::Device;
        // whether the tree will pass 64 Ki nodes is not known before it is built: ask for the quantized records whenever it could
        p.wantQuantized = useQuantizedNodes(d.num_triangles / 2);
        return SLRHIP_OK;
    }
    else {
        p.build = TreeBuild::Host;
        if (buildQBVH(d.vertices, d.triangles, d.num_triangles, &p.bvh, (config.flags & SLRHIP_FLAG_BVH_SPATIAL_SPLITS) != 0) != 0)
            return reject(err, SLRHIP_ERR_INVALID_ARGUMENT, "BVH build failed");
        PREP_TRY(checkTreeLimits(p.bvh.depth, p.bvh.nodes.size(), p.bvh.leafTris.size(), "tree deeper than the 64-entry traversal stack (QBVH.h:299)", err));
    }
    p.quantized = p.build == TreeBuild::Host && useQuantizedNodes(p.bvh.nodes.size());      // instanced scenes traverse float nodes
    if (p.quantized) quantizeNodes(&p.bvh);
    return SLRHIP_OK;
}

// --- per-triangle shading records and the light list (SurfaceObject.cpp:232-249) -------------------------------------------------
int prepareTriangles(const slrhip_scene_desc& d, const MaterialFacts& f, PreparedScene& p, std::string* err) {
    const bool deviceBuild = p.build == TreeBuild::Device;
    p.shadeTris.resize(deviceBuild ? 0 : d.num_triangles);      // the device build writes these records itself (k_shade_tris)
    std::vector<float> importances;
    const char* emitting = f.emitting.data();
    for (uint32_t i = 0; i < d.num_triangles; ++i) {
        const slrhip_triangle& t = d.triangles[i];
        if (deviceBuild && !emitting[t.material]) continue;
        const slrhip_vertex &v0 = d.vertices[t.v[0]], &v1 = d.vertices[t.v[1]], &v2 = d.vertices[t.v[2]];
        ShadeTri s;
        std::memset(&s, 0, sizeof(s));
        shadeTriGeometry(v0, v1, v2, s);                    // pt_triangle.h: the arithmetic k_shade_tris and slrhip_set_vertices share
        s.material = t.material;
        s.light = -1;
        if (emitting[t.material]) {
            s.light = (int32_t)p.lightTris.size();
            LightTri l;
            std::memset(&l, 0, sizeof(l));
            lightTriGeometry(v0, v1, v2, s, l);
            l.tri = i; l.material = t.material;
            p.lightTris.push_back(l);
            p.lightTriangles.push_back(i);
            importances.push_back(1.0f);                    // SingleSurfaceObject::importance :69-71
        }
        if (!deviceBuild) p.shadeTris[i] = s;
    }
    if (p.lightTris.empty() && !d.env) return reject(err, SLRHIP_ERR_UNSUPPORTED, "scene has no emitting triangle and no environment light");

    // RegularConstantDiscrete1D ctor, Core/distributions.cpp:76-95
    p.lightPMF = importances;
    p.lightCDF.assign(importances.size() + 1, 0.0f);
    KahanF sum;
    for (size_t i = 0; i < p.lightPMF.size(); ++i) { sum.add(p.lightPMF[i]); p.lightCDF[i + 1] = sum.result; }
    p.lightIntegral = sum.result;
    for (size_t i = 0; i < p.lightPMF.size(); ++i) { p.lightPMF[i] /= p.lightIntegral; p.lightCDF[i + 1] /= p.lightIntegral; }
    return SLRHIP_OK;
}

// (u0, v0, u1, v1), (u2, v2, z, 0) of one triangle: the layout of DevScene::triUV and of the alpha records.
void gatherTexcoords(const slrhip_scene_desc& d, const slrhip_triangle& t, float z, float4* out) {
    float uv[6];
    triangleTexcoords(d.vertices[t.v[0]], d.vertices[t.v[1]], d.vertices[t.v[2]], uv);
    out[0] = make_float4(uv[0], uv[1], uv[2], uv[3]);
    out[1] = make_float4(uv[4], uv[5], z, 0.0f);
}

// Alpha textures (Triangle::m_alphaTex): one record per triangle that has one, named by its leaf entries; texture coordinates of
// every triangle for the textured shading kernels.
void prepareTexcoords(const slrhip_scene_desc& d, const MaterialFacts& f, PreparedScene& p) {
    if (f.anyAlpha) {
        std::vector<uint32_t> recordOf(d.num_triangles, kNoAlpha);
        for (uint32_t i = 0; i < d.num_triangles; ++i) {
            const int32_t a = f.alphaOfMaterial[d.triangles[i].material];
            if (a < 0) continue;
            recordOf[i] = (uint32_t)(p.alphaTris.size() / 2);
            float texIdx; const uint32_t bits = (uint32_t)a; std::memcpy(&texIdx, &bits, 4);
            p.alphaTris.resize(p.alphaTris.size() + 2);
            gatherTexcoords(d, d.triangles[i], texIdx, &p.alphaTris[p.alphaTris.size() - 2]);
        }
        for (LeafTri& lt : p.bvh.leafTris) lt.alpha = recordOf[lt.tri];
    }
    if (!p.textures.empty()) {
        p.triUV.resize((size_t)d.num_triangles * 2);
        for (uint32_t i = 0; i < d.num_triangles; ++i) gatherTexcoords(d, d.triangles[i], 0.0f, &p.triUV[(size_t)i * 2]);
    }
}

// --- environment sphere: texels + the importance distribution ------------------------------------------------------------------
// InfiniteSphereSurfaceObject ctor (SurfaceObject.cpp:137-141) -> IBLEmission::createIBLImportanceMap
// (IBLEmission.cpp:11-13) -> RegularConstantContinuous2D (Core/distributions.cpp:186-212) over
// sin(pi (y + 0.5) / mapHeight) * importance (Textures/image_textures.cpp:126-133).
void prepareEnvironment(const slrhip_scene_desc& d, PreparedScene& p) {
    if (!d.env) return;
    const slrhip_envmap& e = *d.env;
    const uint32_t mw = e.map_width, mh = e.map_height;
    p.envTexels.assign(e.texels, e.texels + (size_t)e.width * e.height * 3);
    p.envRowPDF.resize((size_t)mw * mh);
    p.envRowCDF.assign((size_t)(mw + 1) * mh, 0.0f);
    p.envTopPDF.resize(mh);
    p.envTopCDF.assign(mh + 1, 0.0f);
    // the steps are pt_envmap.h's, shared with the kernels of slrhip_set_environment
    for (uint32_t y = 0; y < mh; ++y) {
        float* row = p.envRowPDF.data() + (size_t)y * mw;
        const double sinRow = envSinRow(y, mh);
        for (uint32_t x = 0; x < mw; ++x) row[x] = envRowValue(sinRow, e.importance[(size_t)y * mw + x]);
        p.envTopPDF[y] = envBuild1D(row, p.envRowCDF.data() + (size_t)y * (mw + 1), mw);
    }
    envBuild1D(p.envTopPDF.data(), p.envTopCDF.data(), mh);
}

// --- spectral mode with an environment map or image textures: the Meng-15 tables to look texels up at run time ----------------
void prepareUpsampling(const slrhip_scene_desc& d, PreparedScene& p) {
    const slrhip_upsampling_tables* t = d.upsampling;
    p.gridCells.assign(t->cells, t->cells + (size_t)t->grid_width * t->grid_height * 8);
    p.pointUV.assign(t->point_uv, t->point_uv + (size_t)t->num_points * 2);
    p.pointSpectrum.assign(t->point_spectrum, t->point_spectrum + (size_t)t->num_points * 95);
    p.gridWidth = t->grid_width; p.gridHeight = t->grid_height;
}

} // namespace

// --- the tables the shade kernels stage in LDS, packed in the order of ShadeLds' segments (DevScene::shadeTables) ---------------
void packShadeTables(bool spectral, PreparedScene& p) {
    p.tablesFit = p.materials.size() <= (size_t)kLdsMaterials && p.lightTris.size() <= (size_t)kLdsLights &&
                  (!spectral || (p.spectra.size() <= (size_t)kLdsSpectra && p.spectrumPool.size() <= (size_t)kLdsPoolFloats));
    if (!p.tablesFit) return;
    std::vector<float4>& blob = p.shadeTables;
    uint32_t seg = 0;
    const auto append = [&](const void* src, size_t bytes) {
        const size_t n = (bytes + 15) / 16, at = blob.size();
        blob.resize(at + n, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        if (bytes) std::memcpy(blob.data() + at, src, bytes);
        p.tableEnd[seg++] = (uint32_t)blob.size();
    };
    if (spectral) {
        append(p.materialsS.data(), p.materialsS.size() * sizeof(DevMaterialS));
        append(p.spectra.data(), p.spectra.size() * sizeof(DevSpectrum));
        append(p.spectrumPool.data(), p.spectrumPool.size() * sizeof(float));
    }
    else append(p.materials.data(), p.materials.size() * sizeof(DevMaterial));
    append(p.lightTris.data(), p.lightTris.size() * sizeof(LightTri));
    append(p.lightPMF.data(), p.lightPMF.size() * sizeof(float));
    append(p.lightCDF.data(), p.lightCDF.size() * sizeof(float));
    while (seg < 6) { p.tableEnd[seg] = (uint32_t)blob.size(); ++seg; }
}

// --- camera constants, PerspectiveCamera.cpp:15-24, :55 -------------------------------------------------------------------------
DevCamera prepareCamera(const slrhip_camera& c) {
    DevCamera cam;
    std::memcpy(cam.mat, c.local_to_world, sizeof(cam.mat));
    std::memcpy(cam.matInv, c.world_to_local, sizeof(cam.matInv));
    cam.lensRadius = c.lens_radius;
    cam.imgPlaneDistance = c.img_plane_distance;
    cam.objPlaneDistance = c.obj_plane_distance;
    cam.opHeight = 2.0f * cam.objPlaneDistance * std::tan(c.fov_y * 0.5f);
    cam.opWidth = cam.opHeight * c.aspect;
    cam.imgPlaneArea = (float)((double)(cam.opWidth * cam.opHeight) * std::pow((double)(cam.imgPlaneDistance / cam.objPlaneDistance), 2.0));
    cam.areaPDF = cam.lensRadius > 0.0f ? (float)(1.0f / (M_PI * (double)cam.lensRadius * (double)cam.lensRadius)) : 1.0f;
    cam.sensitivity = c.sensitivity > 0 ? c.sensitivity
                                        : (float)(1.0f / (M_PI * (double)cam.lensRadius * (double)cam.lensRadius));
    return cam;
}

int checkTreeLimits(uint32_t depth, uint64_t numNodes, uint64_t numLeafTris, const char* tooDeep, std::string* err) {
    if (3 * depth + 1 > 64) return reject(err, SLRHIP_ERR_UNSUPPORTED, tooDeep);
    if (numNodes * sizeof(QNode) >= (1ull << 32) || numLeafTris * sizeof(LeafTri) >= (1ull << 32))
        return reject(err, SLRHIP_ERR_UNSUPPORTED, "node or leaf array beyond the 4 GiB the traversal kernels address with 32-bit offsets");
    return SLRHIP_OK;
}

bool useQuantizedNodes(uint64_t numNodes) {
    static const bool noQuant = [] { const char* e = tuningEnv("SLRHIP_QUANT"); return e && std::string(e) == "0"; }();
    static const bool forceQuant = [] { const char* e = tuningEnv("SLRHIP_QUANT"); return e && std::string(e) == "1"; }();   // experiment: small trees too
    return (numNodes >= 65536 || forceQuant) && !noQuant;
}

int prepareScene(const slrhip_scene_desc& d, const slrhip_config& config, PreparedScene* out, std::string* err) {
    PreparedScene& p = *out;
    const bool spectral = config.mode == SLRHIP_MODE_SPECTRAL;
    MaterialFacts facts;
    bool anyImageTexture = false;
    PREP_TRY(checkDescriptor(d, spectral, err));
    PREP_TRY(prepareTextures(d, spectral, nullptr, p, &anyImageTexture, err));
    PREP_TRY(prepareMaterialTextures(d, p, facts, err));
    PREP_TRY(prepareMaterials(d, spectral, p, facts, err));
    PREP_TRY(prepareSpectra(d, spectral, p, err));
    p.usage = materialUsage(d, facts);
    PREP_TRY(prepareTree(d, config, facts, p, err));
    PREP_TRY(prepareTriangles(d, facts, p, err));
    prepareTexcoords(d, facts, p);
    prepareEnvironment(d, p);
    // (also for a scene that names the tables without needing them yet: slrhip_set_environment can then give it an environment)
    if (spectral && (d.upsampling || d.env || anyImageTexture)) prepareUpsampling(d, p);
    p.camera = prepareCamera(d.camera);
    packShadeTables(spectral, p);
    return SLRHIP_OK;
}

} // namespace slrhip
