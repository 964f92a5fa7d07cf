// slrhip_materials.hip — changing materials, spectra, textures and lights of the uploaded scene without a scene upload:
// slrhip_set_materials replaces the four tables and rebuilds what depends on them, slrhip_set_texture_texels stores new texels into
// one image texture, slrhip_debug_materials reads the tables back.  The checks and the records are materials_prep.cpp's (the upload's
// own passes), the kernels pt_lights.hip's and pt_geometry.hip's (k_geometry_lights); here are the uploads, the launch list, the
// DevScene and the read-outs.
#include "../../include/slrhip_debug.h"
#include "pt_geometry.h"
#include "pt_lights.h"
#include "slrhip_ctx.h"

using namespace slrhip;

namespace {

MaterialsState stateOf(const slrhip_ctx* ctx) {
    MaterialsState s;
    s.haveScene = ctx->haveScene;
    s.geometryKept = ctx->haveScene && ctx->geometryKept;
    s.hasEnv = ctx->haveScene && ctx->scene.hasEnv != 0;
    s.kept = &ctx->matKept;
    return s;
}

// Segment `seg` of the staged blob as floats, or nullptr when the tables are not staged.
float* stagedSegment(slrhip_ctx* ctx, const PreparedScene& p, uint32_t seg) {
    if (!p.tablesFit) return nullptr;
    return reinterpret_cast<float*>(ctx->shadeTables.ptr + p.tableEnd[seg - 1u]);
}

// The device half: uploads, the launch list, the DevScene.  The context holds no scene while it runs (the caller sees to that).
int commitMaterials(slrhip_ctx* ctx, const PreparedScene& p, const MaterialsPlan& plan, hipStream_t stream) {
    const bool spectral = ctx->config.mode == SLRHIP_MODE_SPECTRAL;
    const uint32_t n = plan.numLights;
    HIP_TRY(hipDeviceSynchronize());               // albedo, feature and query calls may still read the old tables
    // 1. the records of both modes, the spectra, the pool, the textures
    HIP_TRY(ctx->materials.upload(p.materials));
    HIP_TRY(ctx->materialsS.upload(p.materialsS));
    HIP_TRY(ctx->spectrumPool.upload(p.spectrumPool));
    HIP_TRY(ctx->spectra.upload(p.spectra));
    HIP_TRY(ctx->textures.upload(p.textures));
    HIP_TRY(ctx->matTex.upload(p.matTex));
    // 2. the light arrays and the blob, sized for the host's count (a list that stays keeps its records: the count is the same)
    if (!plan.emittingChanged && n != ctx->scene.numLights) return fail(SLRHIP_ERR_HIP, "slrhip_set_materials: the light count changed with the emitting set unchanged (internal error)");
    HIP_TRY(ctx->lightTris.alloc(n));
    HIP_TRY(ctx->lightPMF.alloc(n));
    HIP_TRY(ctx->lightCDF.alloc((size_t)n + 1u));
    HIP_TRY(ctx->shadeTables.upload(p.shadeTables));
    const uint32_t lightsSeg = spectral ? 3u : 1u;
    float4* stagedLights = n ? reinterpret_cast<float4*>(stagedSegment(ctx, p, lightsSeg)) : nullptr;

    LightsUpdate u{};
    u.numTriangles = (uint32_t)ctx->shadeTris.count; u.numMaterials = (uint32_t)p.materials.size(); u.numLights = n;
    u.maskWords = (uint32_t)plan.emitMask.size();
    u.shadeTris = reinterpret_cast<float4*>(ctx->shadeTris.ptr);
    u.lightTris = reinterpret_cast<float4*>(ctx->lightTris.ptr);
    u.pmf = ctx->lightPMF.ptr; u.cdf = ctx->lightCDF.ptr;
    u.stagedPmf = stagedSegment(ctx, p, lightsSeg + 1u); u.stagedCdf = stagedSegment(ctx, p, lightsSeg + 2u);
    u.rebuild = plan.emittingChanged;
    uint32_t launches = 0;
    if (plan.emittingChanged) {
        // 3. the light list over the kept index array, then the records from the kept vertices (both copies)
        if (!ctx->geometryKept || ctx->geoNumTriangles != u.numTriangles) return fail(SLRHIP_ERR_HIP, "slrhip_set_materials: the geometry is not kept (internal error)");
        HIP_TRY(ctx->matEmitMask.upload(plan.emitMask));
        HIP_TRY(ctx->matOffsets.alloc((size_t)lightsBlocks(u.numTriangles) + 1u));
        u.triangles = ctx->geoTriangles.ptr; u.emitMask = ctx->matEmitMask.ptr; u.offsets = ctx->matOffsets.ptr;
        launches += launchLightsRebuild(u, stream);
        GeometryUpdate g{};
        g.numVertices = ctx->geoNumVertices; g.numTriangles = ctx->geoNumTriangles; g.numLights = n;
        g.vertices = reinterpret_cast<float*>(ctx->geoVertices.ptr); g.triangles = ctx->geoTriangles.ptr;
        g.lightTris = u.lightTris; g.stagedLights = stagedLights;
        launches += launchGeometryLights(g, stream);
    }
    else if (stagedLights)                         // the records stay; the blob's copy of them moves with the segments before it
        HIP_TRY(hipMemcpyAsync(stagedLights, ctx->lightTris.ptr, (size_t)n * sizeof(LightTri), hipMemcpyDeviceToDevice, stream));
    launches += launchLightTables(u, stream);
    HIP_TRY(hipGetLastError());

    // 5. the DevScene is passed to every launch by value, and the kernel selection (pt_shade.hip, pt_tail.hip) reads it per launch; the
    // graph of a block of iterations lives inside one slrhip_render call (BlockGraph), so none outlives these pointers
    DevScene& sc = ctx->scene;
    sc.lightTris = ctx->lightTris.ptr; sc.numLights = n; sc.lightPow2 = prevPowerOf2(n);
    sc.lightPMF = ctx->lightPMF.ptr; sc.lightCDF = ctx->lightCDF.ptr; sc.aggImportance = p.lightIntegral;
    sc.materials = ctx->materials.ptr; sc.materialsS = ctx->materialsS.ptr; sc.numMaterials = (uint32_t)p.materials.size();
    sc.hasMicrofacet = p.hasMicrofacet; sc.hasMulti = p.hasMulti;
    sc.spectra = ctx->spectra.ptr; sc.numSpectra = (uint32_t)p.spectra.size();
    sc.spectrumPool = ctx->spectrumPool.ptr; sc.numSpectrumData = (uint32_t)p.spectrumPool.size();
    sc.textures = ctx->textures.ptr; sc.numTextures = (uint32_t)p.textures.size(); sc.matTex = ctx->matTex.ptr;
    sc.shadeTables = p.tablesFit ? ctx->shadeTables.ptr : nullptr;
    std::memcpy(sc.tableEnd, p.tableEnd, sizeof(sc.tableEnd));
    // 6. a later slrhip_set_vertices rewrites the new list; the next call is checked against these tables
    if (ctx->geometryKept) ctx->geoNumLights = n;
    ctx->matKept.usage.emitting = plan.emitting;
    ctx->matKept.textures = p.textures;
    ctx->matLastLaunches = launches; ctx->matLastRebuilt = plan.emittingChanged;
    return SLRHIP_OK;
}

} // namespace

extern "C" {

int slrhip_set_materials(slrhip_ctx* ctx, const slrhip_materials_desc* desc, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_materials: null context");
    PreparedScene p;
    MaterialsPlan plan;
    std::string err;
    if (const int rc = prepareMaterialsUpdate(desc, ctx->config.mode == SLRHIP_MODE_SPECTRAL, stateOf(ctx), &p, &plan, &err)) return fail(rc, err);
    HIP_TRY(hipSetDevice(ctx->device));
    // an upload below may free an array before it fails: the context holds no scene until the last step has succeeded
    ctx->haveScene = false;
    if (const int rc = commitMaterials(ctx, p, plan, (hipStream_t)streamPtr)) { ctx->haveRender = false; return rc; }
    ctx->haveScene = true;
    return SLRHIP_OK;
}

int slrhip_set_texture_texels(slrhip_ctx* ctx, uint32_t texture, const float* deviceSrc, uint32_t flags, void* streamPtr) {
    if (!ctx || !deviceSrc) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_texture_texels: null argument");
    if (reinterpret_cast<uintptr_t>(deviceSrc) % 4u) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_texture_texels: device_src must be 4-byte aligned");
    if (flags & ~SLRHIP_TEXELS_STORE_HALF) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_texture_texels: unknown flag bits");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_set_texture_texels: no scene uploaded");
    if (texture >= ctx->matKept.textures.size()) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_texture_texels: texture index out of range");
    const DevTexture& t = ctx->matKept.textures[texture];
    if (t.kind != SLRHIP_TEXTURE_IMAGE_SPECTRUM) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_set_texture_texels: the texture is not an IMAGE_SPECTRUM texture");
    const uint64_t count = (uint64_t)(uint32_t)t.spec0 * (uint32_t)t.spec1, first = t.pad;
    if (first + count > ctx->matKept.numTexTexels || (first + count) * 3u > ctx->texTexels.count)
        return fail(SLRHIP_ERR_HIP, "slrhip_set_texture_texels: the image lies outside the texel block (internal error)");
    HIP_TRY(hipSetDevice(ctx->device));
    launchTexelsStore(deviceSrc, ctx->texTexels.ptr + first * 3u, (uint32_t)count, (flags & SLRHIP_TEXELS_STORE_HALF) != 0, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the checks of slrhip_set_materials, without a context.
int slrhip_debug_materials_update_check(int32_t mode, const slrhip_scene_desc* uploaded, int32_t geometryKept, const slrhip_materials_desc* desc, uint32_t* facts,
                                        size_t numFacts) {
    const bool spectral = mode == SLRHIP_MODE_SPECTRAL;
    MaterialsKept kept;
    MaterialsState s;
    std::string err;
    if (uploaded) {
        if (const int rc = materialsKeptOf(*uploaded, spectral, &kept, &err)) return fail(rc, err);
        s.haveScene = true; s.geometryKept = geometryKept != 0; s.hasEnv = uploaded->env != nullptr;
        if (facts) {
            const size_t n = kept.usage.triangles.size();
            if (numFacts < 3u * n) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_materials_update_check: facts too small");
            for (size_t m = 0; m < n; ++m) {
                facts[3u * m] = kept.usage.triangles[m]; facts[3u * m + 1u] = kept.usage.instanced[m] ? 1u : 0u; facts[3u * m + 2u] = (uint32_t)kept.usage.alpha[m];
            }
        }
    }
    s.kept = &kept;
    PreparedScene p;
    MaterialsPlan plan;
    if (const int rc = prepareMaterialsUpdate(desc, spectral, s, &p, &plan, &err)) return fail(rc, err);
    return SLRHIP_OK;
}

// Diagnostic (include/slrhip_debug.h): the tables slrhip_set_materials and slrhip_set_texture_texels replace, to host memory.
int slrhip_debug_materials(slrhip_ctx* ctx, uint32_t what, void* hostDst, size_t numWords) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_materials: null argument");
    if (!ctx->haveScene) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_debug_materials: no scene uploaded");
    const DevScene& sc = ctx->scene;
    const bool spectral = ctx->config.mode == SLRHIP_MODE_SPECTRAL;
    const size_t blob = sc.shadeTables ? sc.tableEnd[5] : 0u;
    const void* src = nullptr;
    size_t need = 0;
    switch (what) {
    case 0: need = 32; break;
    case 1: src = spectral ? (const void*)sc.materialsS : (const void*)sc.materials; need = (size_t)sc.numMaterials * (spectral ? 8u : 20u); break;
    case 2: src = sc.spectra; need = (size_t)sc.numSpectra * 8u; break;
    case 3: src = sc.spectrumPool; need = sc.numSpectrumData; break;
    case 4: src = sc.lightPMF; need = sc.numLights; break;
    case 5: src = sc.lightCDF; need = (size_t)sc.numLights + 1u; break;
    case 6: src = sc.shadeTables; need = blob * 4u; break;
    case 7: src = sc.texTexels; need = (size_t)ctx->matKept.numTexTexels * 3u; break;
    case 8: src = sc.textures; need = (size_t)sc.numTextures * 16u; break;
    case 9: src = sc.matTex; need = (size_t)sc.numMaterials * 4u; break;
    default: return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_materials: unknown `what`");
    }
    if (numWords < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_debug_materials: host_dst too small");
    if (what == 0) {
        uint32_t* out = static_cast<uint32_t*>(hostDst);
        std::fill(out, out + 32, 0u);
        out[0] = sc.numLights; out[1] = sc.shadeTables ? 1u : 0u;
        std::copy(sc.tableEnd, sc.tableEnd + 6, out + 2);
        out[8] = sc.hasMicrofacet ? 1u : 0u; out[9] = sc.hasMulti ? 1u : 0u; out[10] = sc.numMaterials; out[11] = sc.numSpectra;
        out[12] = sc.numSpectrumData; out[13] = sc.numTextures; out[14] = (uint32_t)ctx->matKept.numTexTexels; out[15] = sc.lightPow2;
        std::memcpy(out + 16, &sc.aggImportance, sizeof(float));
        out[17] = (uint32_t)blob;
        out[24] = ctx->matLastLaunches; out[25] = ctx->matLastRebuilt ? 1u : 0u;
        return SLRHIP_OK;
    }
    if (need == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(hostDst, src, need * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SLRHIP_OK;
}

} // extern "C"
