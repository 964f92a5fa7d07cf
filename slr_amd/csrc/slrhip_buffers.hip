// slrhip_buffers.hip — the per-pixel buffers beside the framebuffer, on the context and the render loop of slrhip_api.hip: first-hit
// features and camera rays, the albedo buffer, the motion buffer, the noise statistics with slrhip_render_until, the sample clamp, adaptive sampling.
#include <cmath>

#include "slrhip_ctx.h"

using namespace slrhip;

static_assert(sizeof(StatsTotals) == sizeof(struct slrhip_statistics_summary) && offsetof(StatsTotals, sumVarianceOfMean) == offsetof(struct slrhip_statistics_summary, sum_variance_of_mean) &&
              offsetof(StatsTotals, maxSample) == offsetof(struct slrhip_statistics_summary, max_sample), "StatsTotals is slrhip_statistics_summary's layout");
static_assert(sizeof(ClampTotals) == sizeof(struct slrhip_clamp_summary) && offsetof(ClampTotals, removed) == offsetof(struct slrhip_clamp_summary, removed) &&
              offsetof(ClampTotals, largest) == offsetof(struct slrhip_clamp_summary, largest), "ClampTotals is slrhip_clamp_summary's layout");

// ---- the per-pixel records (slrhip_ctx.h PixelRecords): one plumbing for the noise statistics and the sample clamp ----
template <typename Totals> struct RecordKind;
template <> struct RecordKind<StatsTotals> {
    static PixelRecords<StatsTotals>& of(slrhip_ctx* ctx) { return ctx->stats; }
    static constexpr uint32_t kChannels = SLRHIP_STATISTICS_ALL;
    static constexpr const char *kChannelBits = "SLRHIP_STATISTICS_*", *kOff = ": statistics are off (slrhip_statistics_begin after slrhip_render_begin switches them on)";
};
template <> struct RecordKind<ClampTotals> {
    static PixelRecords<ClampTotals>& of(slrhip_ctx* ctx) { return ctx->clamp; }
    static constexpr uint32_t kChannels = SLRHIP_CLAMP_ALL;
    static constexpr const char *kChannelBits = "SLRHIP_CLAMP_*", *kOff = ": the clamp is off (slrhip_clamp_begin after slrhip_render_begin switches it on)";
};

template <typename Totals> static int checkRecords(slrhip_ctx* ctx, const char* what) {
    const std::string w(what);
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, w + ": call slrhip_render_begin first");
    if (!RecordKind<Totals>::of(ctx).on) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + RecordKind<Totals>::kOff);
    return SLRHIP_OK;
}
static int checkStatistics(slrhip_ctx* ctx, const char* what) { return checkRecords<StatsTotals>(ctx, what); }

// Switches the records on for this render; the first enabling call allocates.  They are cleared before their first use (clearStatistics).
template <typename Totals> static int beginRecords(slrhip_ctx* ctx, const char* what) {
    PixelRecords<Totals>& r = RecordKind<Totals>::of(ctx);
    if (!r.on) {
        HIP_TRY(hipSetDevice(ctx->device));
        const uint32_t pixels = ctx->params.numPixels;
        hipError_t e = r.records.alloc(pixels);
        if (e == hipSuccess) e = r.partials.alloc(statsSummaryBlocks(pixels));
        if (e == hipSuccess) e = r.totals.alloc(1);
        if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string(what) + ": allocating the records: " + hipGetErrorString(e));
    }
    r.on = true; r.clear = true;
    return SLRHIP_OK;
}

// one channel as a [height][width] frame in device memory
template <typename Totals> static int resolveRecords(slrhip_ctx* ctx, const char* what, uint32_t channel, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (const int rc = checkRecords<Totals>(ctx, what)) return rc;
    const std::string w(what);
    if (channel == 0 || (channel & (channel - 1u)) || (channel & ~RecordKind<Totals>::kChannels))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": `channel` must be one " + RecordKind<Totals>::kChannelBits + " bit");
    if (!deviceDst || ((uintptr_t)deviceDst & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": null or misaligned destination (4 bytes)");
    const RenderParams& rp = ctx->params;
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight;
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, w + ": destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, s)) return rc;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), s));
    launchRecordResolve<Totals>(RecordKind<Totals>::of(ctx).records.ptr, ctx->pixelXY.ptr, rp.numPixels, rp.imageWidth, channel, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

// The same to host memory, through `resolve` (the kind's slrhip_resolve_* on the scratch: a too-small destination is reported in ITS name).
template <typename Totals, typename Resolve> static int readRecords(slrhip_ctx* ctx, const char* what, float* hostDst, Resolve resolve) {
    if (const int rc = checkRecords<Totals>(ctx, what)) return rc;
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": null destination");
    const size_t need = (size_t)ctx->params.imageWidth * ctx->params.imageHeight;
    return readThroughScratch(ctx, hostDst, need, need, true, nullptr, resolve);
}

// the shard's totals (Summary is Totals' layout: the static_asserts above); waits for the stream
template <typename Totals, typename Summary> static int summarizeRecords(slrhip_ctx* ctx, const char* what, Summary* hostOut, void* streamPtr) {
    if (const int rc = checkRecords<Totals>(ctx, what)) return rc;
    if (!hostOut) return fail(SLRHIP_ERR_INVALID_ARGUMENT, std::string(what) + ": null destination");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, s)) return rc;
    PixelRecords<Totals>& r = RecordKind<Totals>::of(ctx);
    launchRecordSummary<Totals>(r.records.ptr, ctx->params.numPixels, r.partials.ptr, r.totals.ptr, s);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(hostOut, r.totals.ptr, sizeof(*hostOut), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    hostOut->reserved = 0;
    return SLRHIP_OK;
}

// ---- first-hit feature buffers (slrhip_render_features / slrhip_resolve_features / slrhip_camera_rays) -------------------------
static const uint32_t kFeatureVectors = SLRHIP_FEATURE_GEOMETRIC_NORMAL | SLRHIP_FEATURE_SHADING_NORMAL | SLRHIP_FEATURE_SHADING_TANGENT;

FeatureParams slrhip::featureParams(const slrhip_ctx* ctx, uint32_t channels, uint32_t passBegin, uint32_t numPasses) {
    const RenderParams& rp = ctx->params;
    FeatureParams fp{};
    fp.pixelXY = ctx->pixelXY.ptr; fp.records = ctx->featRecords.ptr; fp.b2 = (channels & (kFeatureVectors & ~SLRHIP_FEATURE_GEOMETRIC_NORMAL)) ? ctx->featB2.ptr : nullptr; fp.errorWord = ctx->featError.ptr;
    fp.numPixels = rp.numPixels; fp.numPasses = numPasses; fp.passBegin = passBegin; fp.channels = channels;
    fp.rngSeed = rp.rngSeed; fp.timeStart = rp.timeStart; fp.timeEnd = rp.timeEnd;
    fp.imageWidth = rp.imageWidth; fp.imageHeight = rp.imageHeight;
    return fp;
}
// The error word the feature and the albedo passes share: allocated and cleared, in stream order, by whichever runs first after a
// slrhip_render_begin; sticky until the next one.
static int clearFeatureError(slrhip_ctx* ctx, hipStream_t s) {
    if (ctx->featErrorReady) return SLRHIP_OK;
    HIP_TRY(ctx->featError.alloc(1));
    HIP_TRY(hipMemsetAsync(ctx->featError.ptr, 0, sizeof(uint32_t), s));
    ctx->featErrorReady = true;
    return SLRHIP_OK;
}
static FeatureSums featureSums(const slrhip_ctx* ctx) { return FeatureSums{ctx->featGeometric.ptr, ctx->featShading.ptr, ctx->featTangent.ptr, ctx->featIds.ptr}; }
// The record window the feature and the albedo passes share: room for `records` records and, unless 0, `b2` second barycentrics.
// Growing MOVES the arrays (DevArray::alloc frees and allocates): graphs are captured after both first calls (include/slrhip.h).
static int sizeFeatureRecords(slrhip_ctx* ctx, size_t records, size_t b2) {
    HIP_TRY(ctx->featRecords.alloc(records));
    if (b2) HIP_TRY(ctx->featB2.alloc(b2));
    return SLRHIP_OK;
}

extern "C" {

int slrhip_render_features(slrhip_ctx* ctx, uint32_t channels, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render_features: call slrhip_render_begin first");
    if (channels == 0 || (channels & ~SLRHIP_FEATURE_ALL)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: no or unknown channel bits");
    if ((uint64_t)sppBegin + sppCount > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: pass range beyond 2^32");
    if (sppCount == 0) return SLRHIP_OK;
    const RenderParams& rp = ctx->params;
    // one channel set between two slrhip_render_begin calls: every channel then sums over the same passes (sum / COVERAGE is a mean)
    if (ctx->featChannels && channels != ctx->featChannels)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_features: the channel set differs from that of the first feature call since slrhip_render_begin");
    const bool first = ctx->featChannels == 0;
    ctx->featChannels = channels;
    if (rp.numPixels == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    if (first) {
        // the first feature call since render_begin: the sums (cleared in stream order) and a record window whose size depends on
        // the shard and the channel set alone, so that no later call allocates whatever its pass count
        const size_t pixels = rp.numPixels;
        const bool wantB2 = (channels & (kFeatureVectors & ~SLRHIP_FEATURE_GEOMETRIC_NORMAL)) != 0;
        ctx->featWindow = featureWindow(rp.numPixels, wantB2);
        HIP_TRY(ctx->featGeometric.alloc(pixels)); HIP_TRY(ctx->featShading.alloc(pixels)); HIP_TRY(ctx->featTangent.alloc(pixels));
        HIP_TRY(ctx->featIds.alloc(pixels));
        if (const int rc = sizeFeatureRecords(ctx, pixels * ctx->featWindow, wantB2 ? pixels * ctx->featWindow : 0)) return rc;      // exactly
        HIP_TRY(hipMemsetAsync(ctx->featGeometric.ptr, 0, pixels * sizeof(float4), s));
        HIP_TRY(hipMemsetAsync(ctx->featShading.ptr, 0, pixels * sizeof(float4), s));
        HIP_TRY(hipMemsetAsync(ctx->featTangent.ptr, 0, pixels * sizeof(float4), s));
        HIP_TRY(hipMemsetAsync(ctx->featIds.ptr, 0xFF, pixels * sizeof(uint4), s));
        if (const int rc = clearFeatureError(ctx, s)) return rc;
    }
    const FeatureSums sums = featureSums(ctx);
    for (uint32_t done = 0; done < sppCount; done += ctx->featWindow) {
        const uint32_t n = std::min(ctx->featWindow, sppCount - done);
        // the pixels keep the ids of the highest pass rendered so far
        const uint64_t end = (uint64_t)sppBegin + done + n;
        const uint32_t idsPass = end >= ctx->featPassEnd ? n - 1u : 0xFFFFFFFFu;
        ctx->featPassEnd = std::max(ctx->featPassEnd, end);
        launchFeatures(ctx->scene, featureParams(ctx, channels, sppBegin + done, n), sums, idsPass, ctx->numCUs, s);
    }
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_resolve_features(slrhip_ctx* ctx, uint32_t channel, void* deviceDst, size_t numElements, void* streamPtr) {
    if (!ctx || !deviceDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: null argument");
    if ((uintptr_t)deviceDst & 3u) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: misaligned pointer (4 bytes)");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_resolve_features: call slrhip_render_begin first");
    if (channel == 0 || (channel & (channel - 1u)) || (channel & ~SLRHIP_FEATURE_ALL))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: `channel` must be one SLRHIP_FEATURE_* bit");
    if (!(ctx->featChannels & channel))
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: no slrhip_render_features call since slrhip_render_begin asked for this channel");
    const RenderParams& rp = ctx->params;
    const size_t k = (channel & (SLRHIP_FEATURE_DISTANCE | SLRHIP_FEATURE_COVERAGE)) ? 1u : 3u;
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight * k;
    if (numElements < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_features: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemsetAsync(deviceDst, channel == SLRHIP_FEATURE_IDS ? 0xFF : 0, need * sizeof(uint32_t), s));
    if (rp.numPixels) launchFeatureResolve(featureParams(ctx, channel, 0, 0), featureSums(ctx), channel, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_features(slrhip_ctx* ctx, uint32_t channel, void* hostDst, size_t numElements) {
    if (!ctx || !hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_features: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_read_features: call slrhip_render_begin first");
    // the scratch has room for three planes whatever the channel; the resolve checks the channel and the caller's numElements
    const size_t plane = (size_t)ctx->params.imageWidth * ctx->params.imageHeight;
    const size_t k = (channel & (SLRHIP_FEATURE_DISTANCE | SLRHIP_FEATURE_COVERAGE)) ? 1u : 3u;
    return readThroughScratch(ctx, hostDst, plane * k, plane * 3u, true, "slrhip_read_features", [&](float* scratch) { return slrhip_resolve_features(ctx, channel, scratch, numElements, nullptr); });
}

int slrhip_camera_rays(slrhip_ctx* ctx, uint32_t pass, slrhip_ray* rays, uint32_t* pixelXY, uint32_t capacity, uint32_t* count, void* streamPtr) {
    if (!ctx || !count) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: null context or count");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_camera_rays: call slrhip_render_begin first");
    const RenderParams& rp = ctx->params;
    *count = rp.numPixels;
    if (rp.numPixels == 0 || (!rays && !pixelXY && capacity == 0)) return SLRHIP_OK;          // the count alone
    if (!rays) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: null ray pointer");
    if (((uintptr_t)rays & 15u) || ((uintptr_t)pixelXY & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: misaligned pointer (rays: 16 bytes; pixel_xy: 4)");
    if (capacity < rp.numPixels)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_camera_rays: capacity " + std::to_string(capacity) + " is smaller than the shard's " + std::to_string(rp.numPixels) + " pixels");
    HIP_TRY(hipSetDevice(ctx->device));
    launchCameraRays(ctx->scene, featureParams(ctx, 0, pass, 1), reinterpret_cast<float4*>(rays), pixelXY, (hipStream_t)streamPtr);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_features_status(slrhip_ctx* ctx, uint32_t* bits, void* stream) {
    if (!ctx || !bits) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_features_status: null argument");
    *bits = 0;
    if (!ctx->haveRender || !ctx->featErrorReady) return SLRHIP_OK;     // no feature or albedo pass can have run
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(bits, ctx->featError.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SLRHIP_OK;
}

// ---- the albedo buffer (slrhip_render_albedo / slrhip_resolve_albedo / slrhip_read_albedo) -----------------------------------------
// The traversal and the record window are the feature pass's; the fold and the sums are pt_albedo.hip's.
int slrhip_render_albedo(slrhip_ctx* ctx, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_albedo: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_render_albedo: call slrhip_render_begin first");
    if ((uint64_t)sppBegin + sppCount > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_albedo: pass range beyond 2^32");
    if (sppCount == 0) return SLRHIP_OK;
    const RenderParams& rp = ctx->params;
    if (rp.numPixels == 0) { ctx->albPasses += sppCount; return SLRHIP_OK; }
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    const bool wantB2 = ctx->scene.numTextures != 0;                 // the texture coordinate needs both barycentrics
    const uint32_t components = rp.spectral ? SLRHIP_SPECTRAL_COMPONENTS : SLRHIP_RGB_COMPONENTS;
    if (!ctx->albReady) {
        // the first albedo call since render_begin: the sums (cleared in stream order) and room in the record window, sized by the
        // shard and the scene alone, so that no later call allocates whatever its pass count.  The window's arrays only ever grow:
        // a feature call that sized them for more passes keeps its room.
        const size_t pixels = rp.numPixels;
        ctx->albWindow = featureWindow(rp.numPixels, wantB2);
        HIP_TRY(ctx->albSums.alloc(pixels * components));
        if (const int rc = sizeFeatureRecords(ctx, std::max(ctx->featRecords.capacity, pixels * ctx->albWindow),
                                              wantB2 ? std::max(ctx->featB2.capacity, pixels * ctx->albWindow) : 0)) return rc;
        HIP_TRY(hipMemsetAsync(ctx->albSums.ptr, 0, pixels * components * sizeof(float), s));
        if (const int rc = clearFeatureError(ctx, s)) return rc;
        ctx->albReady = true;
    }
    for (uint32_t done = 0; done < sppCount; done += ctx->albWindow) {
        const uint32_t n = std::min(ctx->albWindow, sppCount - done);
        FeatureParams fp = featureParams(ctx, 0, sppBegin + done, n);
        fp.b2 = wantB2 ? ctx->featB2.ptr : nullptr;
        launchFeatureTrace(ctx->scene, fp, ctx->numCUs, s);
        launchAlbedoFold(ctx->scene, fp, rp.spectral != 0, ctx->albSums.ptr, s);
    }
    ctx->albPasses += sppCount;
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_resolve_albedo(slrhip_ctx* ctx, float* deviceDst, size_t numFloats, uint32_t* passes, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_albedo: null context");
    if (!deviceDst || ((uintptr_t)deviceDst & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_albedo: null or misaligned destination (4 bytes)");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_resolve_albedo: call slrhip_render_begin first");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_albedo: destination too small");
    if (passes) *passes = (uint32_t)std::min<uint64_t>(ctx->albPasses, 0xFFFFFFFFull);
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), s));
    if (rp.numPixels && ctx->albReady)
        launchAlbedoResolve(featureParams(ctx, 0, 0, 0), rp.spectral ? SLRHIP_SPECTRAL_COMPONENTS : SLRHIP_RGB_COMPONENTS, ctx->albSums.ptr, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_albedo(slrhip_ctx* ctx, float* hostDst, size_t numFloats, uint32_t* passes) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_albedo: null context");
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_albedo: null destination");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_read_albedo: call slrhip_render_begin first");
    const size_t need = frameFloats(ctx->params);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_albedo: destination too small");
    return readThroughScratch(ctx, hostDst, need, need, true, "slrhip_read_albedo", [&](float* scratch) { return slrhip_resolve_albedo(ctx, scratch, need, passes, nullptr); });
}

// ---- the motion buffer (slrhip_render_motion / slrhip_render_motion_vertices / slrhip_resolve_motion / slrhip_read_motion) -----------
// The traversal and the record window are the feature pass's; the fold and the sums are pt_motion.hip's; the sample is pt_motion.h's.
// What the two entry points share, after their argument checks.  prevVertices == nullptr: slrhip_render_motion's pass (16 B records,
// k_motion_fold<false>); else slrhip_render_motion_vertices' (the window also keeps b2; k_motion_fold<true> on the kept arrays).
static int renderMotion(slrhip_ctx* ctx, const slrhip_motion_desc* d, const slrhip_vertex* prevVertices, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (sppCount == 0) return SLRHIP_OK;
    const RenderParams& rp = ctx->params;
    if (rp.numPixels == 0) return SLRHIP_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    const size_t pixels = rp.numPixels;
    if (!ctx->motionReady) {
        // the first motion call since render_begin: the sums, cleared in stream order
        HIP_TRY(ctx->motionSums.alloc(pixels));
        HIP_TRY(hipMemsetAsync(ctx->motionSums.ptr, 0, pixels * sizeof(float4), s));
        if (const int rc = clearFeatureError(ctx, s)) return rc;
        ctx->motionWindow = ctx->motionVerticesWindow = 0;
        ctx->motionReady = true;
    }
    // ... and the first of its kind: room in the record window, sized by the shard alone (with b2: 20 B per record), so that no later
    // call allocates whatever its pass count.  The window's arrays only ever grow: what the feature, albedo or other motion calls
    // sized them for stays.
    const bool verts = prevVertices != nullptr;
    uint32_t& window = verts ? ctx->motionVerticesWindow : ctx->motionWindow;
    if (window == 0) {
        const uint32_t w = featureWindow(rp.numPixels, verts);
        if (const int rc = sizeFeatureRecords(ctx, std::max(ctx->featRecords.capacity, pixels * w), verts ? std::max(ctx->featB2.capacity, pixels * w) : 0)) return rc;
        window = w;
    }
    // both cameras by value, from the host arithmetic of the upload's camera constants; no previous camera: the current one
    const DevCamera& cam = ctx->scene.camera;
    MotionParams mp{};
    mp.now = makeMotionCamera(cam.mat, cam.matInv, cam.opWidth, cam.opHeight, cam.objPlaneDistance);
    mp.prev = mp.now;
    if (d->previous_camera) {
        const DevCamera prev = prepareCamera(*d->previous_camera);
        mp.prev = makeMotionCamera(prev.mat, prev.matInv, prev.opWidth, prev.opHeight, prev.objPlaneDistance);
    }
    mp.instances = ctx->scene.instances;
    mp.prevTransforms = reinterpret_cast<const float4*>(d->previous_transforms);
    mp.sums = ctx->motionSums.ptr;
    if (verts) {
        mp.vertices = reinterpret_cast<const float*>(ctx->geoVertices.ptr);
        mp.triangles = reinterpret_cast<const uint4*>(ctx->geoTriangles.ptr);
        mp.prevVertices = reinterpret_cast<const float*>(prevVertices);
        mp.numVertices = ctx->geoNumVertices; mp.numTriangles = ctx->geoNumTriangles;
    }
    for (uint32_t done = 0; done < sppCount; done += window) {
        const uint32_t n = std::min(window, sppCount - done);
        FeatureParams fp = featureParams(ctx, 0, sppBegin + done, n);
        fp.b2 = verts ? ctx->featB2.ptr : nullptr;
        launchFeatureTrace(ctx->scene, fp, ctx->numCUs, s);
        launchMotionFold(cam, fp, mp, s);
    }
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_render_motion(slrhip_ctx* ctx, const slrhip_motion_desc* d, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_motion: null context");
    const char* what = nullptr;
    if (const int rc = motionRefusal(ctx->haveRender, ctx->haveScene ? ctx->scene.numInstances : 0u, d, sppBegin, sppCount, &what))
        return fail(rc, std::string("slrhip_render_motion: ") + what);
    return renderMotion(ctx, d, nullptr, sppBegin, sppCount, streamPtr);
}

int slrhip_render_motion_vertices(slrhip_ctx* ctx, const slrhip_motion_vertices_desc* d, uint32_t sppBegin, uint32_t sppCount, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_motion_vertices: null context");
    const char* what = nullptr;
    const bool have = ctx->haveScene;
    if (const int rc = motionVerticesRefusal(ctx->haveRender, have ? ctx->scene.numInstances : 0u, ctx->config.flags, have ? ctx->treeBuilder : 0u, d, sppBegin,
                                             sppCount, &what))
        return fail(rc, std::string("slrhip_render_motion_vertices: ") + what);
    if (d->previous_vertices && (!ctx->geometryKept || !ctx->geoVertices.ptr || !ctx->geoTriangles.ptr))
        return fail(SLRHIP_ERR_HIP, "slrhip_render_motion_vertices: the vertex and index arrays are not kept (internal error)");
    return renderMotion(ctx, &d->frame, d->previous_vertices, sppBegin, sppCount, streamPtr);
}

int slrhip_resolve_motion(slrhip_ctx* ctx, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_motion: null context");
    if (!deviceDst || ((uintptr_t)deviceDst & 3u)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_motion: null or misaligned destination (4 bytes)");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_resolve_motion: call slrhip_render_begin first");
    const RenderParams& rp = ctx->params;
    const size_t need = (size_t)rp.imageWidth * rp.imageHeight * 4u;
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_motion: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    const hipStream_t s = (hipStream_t)streamPtr;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), s));
    if (rp.numPixels && ctx->motionReady) launchMotionResolve(featureParams(ctx, 0, 0, 0), ctx->motionSums.ptr, deviceDst, s);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_motion(slrhip_ctx* ctx, float* hostDst, size_t numFloats) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_motion: null context");
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_motion: null destination");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_read_motion: call slrhip_render_begin first");
    const size_t need = (size_t)ctx->params.imageWidth * ctx->params.imageHeight * 4u;
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_motion: destination too small");
    return readThroughScratch(ctx, hostDst, need, need, true, "slrhip_read_motion", [&](float* scratch) { return slrhip_resolve_motion(ctx, scratch, need, nullptr); });
}

// ---- per-pixel noise statistics (slrhip_statistics_begin / slrhip_resolve_statistics / slrhip_statistics_summary / slrhip_render_until) ----
int slrhip_statistics_begin(slrhip_ctx* ctx) {
    if (!ctx) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_statistics_begin: null context");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_statistics_begin: call slrhip_render_begin first");
    if (!ctx->firstRenderCall) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_statistics_begin: this render has begun (call it before the first slrhip_render after slrhip_render_begin)");
    if (ctx->stats.on) return SLRHIP_OK;               // a second call changes nothing
    return beginRecords<StatsTotals>(ctx, "slrhip_statistics_begin");
}

int slrhip_resolve_statistics(slrhip_ctx* ctx, uint32_t channel, float* deviceDst, size_t numFloats, void* streamPtr) { return resolveRecords<StatsTotals>(ctx, "slrhip_resolve_statistics", channel, deviceDst, numFloats, streamPtr); }
int slrhip_read_statistics(slrhip_ctx* ctx, uint32_t channel, float* hostDst, size_t numFloats) { return readRecords<StatsTotals>(ctx, "slrhip_read_statistics", hostDst, [&](float* scratch) { return slrhip_resolve_statistics(ctx, channel, scratch, numFloats, nullptr); }); }
int slrhip_statistics_summary(slrhip_ctx* ctx, struct slrhip_statistics_summary* hostOut, void* streamPtr) { return summarizeRecords<StatsTotals>(ctx, "slrhip_statistics_summary", hostOut, streamPtr); }

// The stop check of slrhip_render_until: the metric of a summary, in double.
static double noiseMetric(const struct slrhip_statistics_summary& t, uint32_t metric) {
    if (t.pixels == 0) return 0.0;                     // an empty shard has no noise
    const double rmse = std::sqrt(t.sum_variance_of_mean / (double)t.pixels);
    if (metric == SLRHIP_NOISE_RMSE) return rmse;
    const double mean = t.sum_mean / (double)t.pixels;
    return mean == 0.0 ? INFINITY : rmse / mean;
}

int slrhip_render_until(slrhip_ctx* ctx, uint32_t sppBegin, const slrhip_noise_target* target, uint32_t* sppDone, struct slrhip_statistics_summary* last,
                        void* stream) {
    if (sppDone) *sppDone = 0;
    if (const int rc = checkStatistics(ctx, "slrhip_render_until")) return rc;
    if (!target || !sppDone) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: null argument");
    if (target->spp_step == 0 || target->spp_max == 0) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: spp_step and spp_max must be positive");
    if (target->metric != SLRHIP_NOISE_RMSE && target->metric != SLRHIP_NOISE_RELATIVE) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: unknown metric");
    if (std::isnan(target->target)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: the target is NaN");
    if ((uint64_t)sppBegin + target->spp_max > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_until: pass range beyond 2^32");
    struct slrhip_statistics_summary totals;
    std::memset(&totals, 0, sizeof(totals));
    for (uint32_t done = 0; done < target->spp_max;) {
        const uint32_t n = std::min(target->spp_step, target->spp_max - done);
        if (const int rc = slrhip_render(ctx, sppBegin + done, n, stream)) return rc;
        done += n;
        *sppDone = done;
        if (const int rc = slrhip_statistics_summary(ctx, &totals, stream)) return rc;
        if (last) *last = totals;
        // "at least 2 passes": the variance of one sample is not defined (the channels are 0 then, which would read as "no noise")
        if (totals.samples >= 2 * totals.pixels && noiseMetric(totals, target->metric) <= (double)target->target) break;
    }
    return SLRHIP_OK;
}

// ---- the sample clamp (slrhip_clamp_begin / slrhip_resolve_clamp / slrhip_clamp_summary; the rule: pt_clamp.h) ----
int slrhip_clamp_begin(slrhip_ctx* ctx, const slrhip_clamp_desc* d) {
    if (!ctx || !d) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: null argument");
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_clamp_begin: call slrhip_render_begin first");
    if (!ctx->firstRenderCall) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: this render has begun (call it before the first slrhip_render after slrhip_render_begin)");
    if (!(d->limit > 0.0f)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: the limit must be > 0 (and not NaN); INFINITY clamps nothing");
    if (d->flags & ~SLRHIP_CLAMP_DROP_NONFINITE) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: unknown flag bits");
    if (d->reserved[0] || d->reserved[1]) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_clamp_begin: reserved must be 0");
    if (const int rc = beginRecords<ClampTotals>(ctx, "slrhip_clamp_begin")) return rc;          // a second call changes the limit
    ctx->clampLimit = d->limit; ctx->clampFlags = d->flags;
    return SLRHIP_OK;
}

int slrhip_resolve_clamp(slrhip_ctx* ctx, uint32_t channel, float* deviceDst, size_t numFloats, void* streamPtr) { return resolveRecords<ClampTotals>(ctx, "slrhip_resolve_clamp", channel, deviceDst, numFloats, streamPtr); }
int slrhip_read_clamp(slrhip_ctx* ctx, uint32_t channel, float* hostDst, size_t numFloats) { return readRecords<ClampTotals>(ctx, "slrhip_read_clamp", hostDst, [&](float* scratch) { return slrhip_resolve_clamp(ctx, channel, scratch, numFloats, nullptr); }); }
int slrhip_clamp_summary(slrhip_ctx* ctx, struct slrhip_clamp_summary* hostOut, void* streamPtr) { return summarizeRecords<ClampTotals>(ctx, "slrhip_clamp_summary", hostOut, streamPtr); }

// ---- adaptive sampling (slrhip_render_adaptive / slrhip_resolve_framebuffer_mean / slrhip_adaptive_active) ----
// The retirement check after a block: the next active list from the current one (pt_adaptive.hip), its length read back.
static int adaptiveSelect(slrhip_ctx* ctx, const slrhip_adaptive_target& target, hipStream_t stream) {
    const int next = ctx->activeList < 0 ? 0 : ctx->activeList ^ 1;
    AdaptiveSelect a{};
    a.records = ctx->stats.records.ptr; a.shardXY = ctx->pixelXY.ptr;
    a.prevIndex = ctx->activeList < 0 ? nullptr : ctx->adaptIndex[ctx->activeList].ptr; a.prevCount = ctx->activePixels;
    a.nextXY = ctx->adaptXY[next].ptr; a.nextIndex = ctx->adaptIndex[next].ptr;
    a.blockOffsets = ctx->adaptOffsets.ptr; a.countWord = ctx->adaptCount.ptr;
    a.threshold = target.threshold; a.floor = target.floor;
    launchAdaptiveSelect(a, stream);
    HIP_TRY(hipGetLastError());
    uint32_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, ctx->adaptCount.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (count > ctx->activePixels) return fail(SLRHIP_ERR_HIP, "slrhip_render_adaptive: the active list grew from " + std::to_string(ctx->activePixels) + " to " + std::to_string(count) + " pixels (internal error)");
    ctx->activePixels = count; ctx->activeList = next;
    return SLRHIP_OK;
}

int slrhip_render_adaptive(slrhip_ctx* ctx, uint32_t sppBegin, const slrhip_adaptive_target* target, uint32_t* sppDone, uint64_t* samplesDone,
                           void* streamPtr) {
    if (sppDone) *sppDone = 0;
    if (samplesDone) *samplesDone = 0;
    if (const int rc = checkStatistics(ctx, "slrhip_render_adaptive")) return rc;
    if (!target || !sppDone) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: null argument");
    if (!(target->threshold >= 0.0f) || !(target->floor >= 0.0f)) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: threshold and floor must be >= 0 (and not NaN)");
    if (target->spp_min < 2 || target->spp_step == 0 || target->spp_max < target->spp_min)
        return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: need spp_min >= 2, spp_step >= 1 and spp_max >= spp_min");
    if ((uint64_t)sppBegin + target->spp_max > 0xFFFFFFFFull) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_render_adaptive: pass range beyond 2^32");
    const RenderParams& shard = ctx->params;
    if (shard.numSlots == 0 || ctx->activePixels == 0) return SLRHIP_OK;        // an empty shard, or every pixel has retired
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    {
        hipError_t e = hipSuccess;
        for (int k = 0; k < 2; ++k) {
            if (e == hipSuccess) e = ctx->adaptXY[k].alloc(shard.numPixels);
            if (e == hipSuccess) e = ctx->adaptIndex[k].alloc(shard.numPixels);
        }
        if (e == hipSuccess) e = ctx->adaptOffsets.alloc(adaptiveSelectBlocks(shard.numPixels));
        if (e == hipSuccess) e = ctx->adaptCount.alloc(1);
        if (e != hipSuccess) return fail(SLRHIP_ERR_HIP, std::string("slrhip_render_adaptive: allocating the active lists: ") + hipGetErrorString(e));
    }
    if (const int rc = clearStatistics(ctx, stream)) return rc;
    const uint64_t budget = resultWindowBudget();
    uint32_t done = 0;
    while (ctx->activePixels > 0) {
        const uint32_t block = adaptiveBlock(target->spp_min, target->spp_step, target->spp_max, done);
        if (block == 0) break;                                                   // spp_max passes have been handed out
        // the block as the windows of an ordinary call of `block` passes over the active pixels
        ActiveWindow list{};
        const bool compact = ctx->activeList >= 0;
        if (compact) { list.xy = ctx->adaptXY[ctx->activeList].ptr; list.index = ctx->adaptIndex[ctx->activeList].ptr; list.count = ctx->activePixels; }
        const uint32_t window = planWindows(ctx->activePixels, shard.spectral != 0, block, budget);
        HIP_TRY(ctx->results.alloc((size_t)window * ctx->activePixels * (shard.spectral ? 4u : 1u)));
        ctx->buffers.results = ctx->results.ptr;
        for (uint32_t w = 0; w < block; w += window) {
            const uint32_t passes = std::min(window, block - w);
            if (const int rc = renderWindow(ctx, sppBegin + done + w, passes, stream, compact ? &list : nullptr)) return rc;
            if (samplesDone) *samplesDone += (uint64_t)ctx->activePixels * passes;
        }
        done += block;
        *sppDone = done;
        if (const int rc = adaptiveSelect(ctx, *target, stream)) return rc;
    }
    return SLRHIP_OK;
}

int slrhip_resolve_framebuffer_mean(slrhip_ctx* ctx, float* deviceDst, size_t numFloats, void* streamPtr) {
    if (const int rc = checkStatistics(ctx, "slrhip_resolve_framebuffer_mean")) return rc;
    if (!deviceDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_framebuffer_mean: null argument");
    const RenderParams& rp = ctx->params;
    const size_t need = frameFloats(rp);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_resolve_framebuffer_mean: destination too small");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)streamPtr;
    if (const int rc = clearStatistics(ctx, stream)) return rc;
    HIP_TRY(hipMemsetAsync(deviceDst, 0, need * sizeof(float), stream));
    launchResolveMean(ctx->buffers, rp, ctx->stats.records.ptr, deviceDst, stream);
    HIP_TRY(hipGetLastError());
    return SLRHIP_OK;
}

int slrhip_read_framebuffer_mean(slrhip_ctx* ctx, float* hostDst, size_t numFloats) {
    if (const int rc = checkStatistics(ctx, "slrhip_read_framebuffer_mean")) return rc;
    if (!hostDst) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_framebuffer_mean: null argument");
    const size_t need = frameFloats(ctx->params);
    if (numFloats < need) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_read_framebuffer_mean: destination too small");
    return readThroughScratch(ctx, hostDst, need, need, true, nullptr, [&](float* scratch) { return slrhip_resolve_framebuffer_mean(ctx, scratch, need, nullptr); });
}

int slrhip_adaptive_active(slrhip_ctx* ctx, uint32_t* hostCount, void*) {
    if (!ctx || !hostCount) return fail(SLRHIP_ERR_INVALID_ARGUMENT, "slrhip_adaptive_active: null argument");
    *hostCount = 0;
    if (!ctx->haveRender) return fail(SLRHIP_ERR_NO_SCENE, "slrhip_adaptive_active: call slrhip_render_begin first");
    *hostCount = ctx->activePixels;
    return SLRHIP_OK;
}

} // extern "C"
