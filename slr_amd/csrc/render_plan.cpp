// render_plan.cpp — the arithmetic of the render set-up (render_plan.h): pure functions of their arguments.
#include "render_plan.h"

#include <algorithm>

#include "../../include/slrhip.h"
#include "pt_kernels.h"

namespace slrhip {

namespace {

// integers t in [begin, end) with t % count == index
uint64_t countCongruent(uint64_t begin, uint64_t end, uint32_t index, uint32_t count) {
    const auto below = [&](uint64_t n) { return n > index ? (n - index + count - 1) / count : 0; };      // those in [0, n)
    return below(end) - below(begin);
}

int refuse(std::string* err, const char* what) {
    *err = std::string("slrhip_render_begin: ") + what;
    return SLRHIP_ERR_INVALID_ARGUMENT;
}

} // namespace

int planFrame(int32_t width, int32_t height, uint32_t shardIndex, uint32_t shardCount, uint32_t configStripes, bool spectral,
              long autoStripesOverride, int pairs, FramePlan* out, std::string* err) {
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return refuse(err, "image size out of range");
    if (shardCount == 0 || shardIndex >= shardCount) return refuse(err, "bad shard");
    FramePlan p;
    p.width = (uint32_t)width; p.height = (uint32_t)height;
    p.shardIndex = shardIndex; p.shardCount = shardCount;
    p.spectral = spectral;
    // the shard owns the 8x8 tiles t with t % count == index (ImageSensor.cpp:43-44); only the last column and row are cut
    const uint32_t tilesX = (p.width + 7) >> 3, tilesY = (p.height + 7) >> 3;
    const uint32_t lastW = p.width - 8 * (tilesX - 1), lastH = p.height - 8 * (tilesY - 1);
    uint64_t numPixels = 0;
    for (uint32_t ty = 0; ty < tilesY; ++ty) {
        const uint64_t rowBegin = (uint64_t)ty * tilesX, rowEnd = rowBegin + tilesX;
        uint64_t columns = 8 * countCongruent(rowBegin, rowEnd, shardIndex, shardCount);
        if ((rowEnd - 1) % shardCount == shardIndex) columns -= 8 - lastW;
        numPixels += columns * (ty + 1 == tilesY ? lastH : 8u);
    }
    uint32_t stripes = configStripes;
    if (stripes == 0) {
        // Paths in flight: throughput keeps rising with the slot count (longer launches amortise the per-wave tail of the
        // traversal kernel: 807 / 1146 / 1267 Msamples/s at 0.9 / 3.7 / 7.4 M slots on the 1280x720 Cornell scene in round 1),
        // at ~200 B of HBM per slot; the per-pixel sample pool keeps the stripes of a pixel finishing together, so fewer, fuller
        // iterations keep paying.  The count is a power of two (the stripes of a pixel then fill whole lane groups of the shade
        // workgroup, PathBuffers): the smallest that reaches ~22 M slots in RGB mode, ~7.4 M in spectral mode (492 B per slot; its
        // shade kernel is latency-bound, not launch-bound), at most 64 (the width of the pool's mask; also the best count measured
        // for the eighth of the image a rank owns at N = 8).  Measured with the fused shade kernel, 16 vs 32 stripes at 1280x720
        // (profiles/r03_e_*): Cornell 2 709 vs 2 719, environment light 5 630 vs 6 061, 10 M-triangle grid 1 954 vs 1 981 Msamples/s.
        const uint32_t target = spectral ? 7372800u : 22118400u;
        stripes = 1u;
        while (stripes < 64u && numPixels * stripes < target) stripes *= 2u;
        if (numPixels == 0) stripes = 1u;
        if (autoStripesOverride >= 1 && autoStripesOverride <= 64) stripes = (uint32_t)autoStripesOverride;      // measurement: force the automatic choice
    }
    // Slots are paths in flight, not places in the image (pt_kernels.h): `stripes` only sizes their number
    const uint64_t slotCapacity = std::max<uint64_t>((numPixels * stripes + 255u) / 256u, 1) * 256u;
    if (slotCapacity > 0x7FFFFFFFull) return refuse(err, "too many path slots");
    p.numPixels = (uint32_t)numPixels;
    p.stripes = stripes;
    p.slotCapacity = (size_t)slotCapacity;
    p.numSlots = numPixels ? (uint32_t)slotCapacity : 0u;
    // queue regions: slot block b appends to region b % kShards, so a region holds at most ceil(numBlocks / kShards) blocks
    p.numBlocks = (uint32_t)(slotCapacity / 256u);
    p.shardCapacity = ((p.numBlocks + kShards - 1) / kShards) * 256;
    // SLRHIP_PAIRS (bit 0: ray origin + direction, bit 1: the path's radiance sum + its compensation, bit 2: sample header + RNG
    // state): the two records of a pair interleaved in one array, one 32-byte sector per slot (PathBuffers::rayStride / spStride)
    p.rayStride = (pairs & 1) ? 2u : 1u; p.spStride = (pairs & 2) ? 2u : 1u; p.hdrStride = (pairs & 4) ? 2u : 1u;
    *out = p;
    return SLRHIP_OK;
}

std::vector<uint32_t> shardPixels(const FramePlan& p) {
    if (p.numPixels == 0) return {0xFFFFFFFFu};        // an empty shard keeps the buffers valid
    // tiles in shard order, row-major inside each tile, so 64 consecutive slots (one wavefront) are one 8x8 tile
    const uint32_t tilesX = (p.width + 7) >> 3, tilesY = (p.height + 7) >> 3;
    std::vector<uint32_t> pixels;
    pixels.reserve(p.numPixels);
    for (uint32_t t = p.shardIndex; t < tilesX * tilesY; t += p.shardCount) {
        const uint32_t tx = t % tilesX, ty = t / tilesX;
        for (uint32_t ly = 0; ly < 8; ++ly)
            for (uint32_t lx = 0; lx < 8; ++lx) {
                const uint32_t x = tx * 8 + lx, y = ty * 8 + ly;
                if (x < p.width && y < p.height) pixels.push_back(x | (y << 16));
            }
    }
    return pixels;
}

// The result window (PathBuffers::results) holds one entry per pixel and pass: 16 B (RGB) / 64 B (spectral).  A call of more passes
// than fit the budget or than 2^32 samples is rendered as several windows, one after the other; the sensor adds in pass order
// either way, so the image does not depend on the split.
uint32_t planWindows(uint32_t numPixels, bool spectral, uint32_t sppCount, uint64_t budgetBytes) {
    const uint64_t entryBytes = (spectral ? 4u : 1u) * 16u;
    const uint64_t maxPasses = std::max<uint64_t>(1, std::min<uint64_t>(budgetBytes / ((uint64_t)numPixels * entryBytes), 0xF0000000ull / numPixels));      // (run ids + one round of waves stay inside 32 bits)
    // whole runs (RenderParams::runLength passes of a pixel in a row, pt_kernels.h) wherever the call is long enough: a window of
    // an odd number of passes would fall back to runs of one pass and lose the coherence of a wave's slots
    uint32_t window = (uint32_t)std::min<uint64_t>(maxPasses, std::max<uint32_t>(sppCount, 1u));
    if (window >= kDefaultRunLength) window -= window % kDefaultRunLength;
    return window;
}

// The record window of the feature and the albedo passes: 16 B per (pixel, pass), 20 B when the second barycentric is kept, within
// kFeatureRecordBytes and 2^31 records, 64 passes at the most and one at the least.  It depends on the shard and the channel set
// (or the scene) alone, so that no later call allocates whatever its pass count.
uint32_t featureWindow(uint32_t numPixels, bool wantB2) {
    const uint64_t perPass = (uint64_t)numPixels * (wantB2 ? 20u : 16u);
    return (uint32_t)std::max<uint64_t>(1u, std::min<uint64_t>({kFeatureRecordBytes / perPass, 0x7FFFFFFFull / numPixels, 64u}));
}

WindowPlan planWindow(uint32_t numPixels, uint32_t sppCount, uint32_t runLengthOverride) {
    WindowPlan w;
    w.workItems = numPixels * sppCount;                           // < 2^32: planWindows
    // passes per run (pt_kernels.h WorkItem): the largest power-of-two fraction of the default that divides the window's pass count
    w.runLength = runLengthOverride ? runLengthOverride : kDefaultRunLength;
    while (w.runLength > 1 && (sppCount % w.runLength) != 0) w.runLength /= 2;
    if (sppCount && sppCount % w.runLength) w.runLength = 1;
    w.numRuns = numPixels * (sppCount / std::max(w.runLength, 1u));
    return w;
}

PrimaryPlan planPrimary(uint32_t numPixels, uint32_t sppCount, uint32_t configFlags, bool instanced, bool spectral, bool environment,
                        bool quantized) {
    PrimaryPlan p;
    if ((configFlags & (SLRHIP_FLAG_NO_PRIMARY_PASS | SLRHIP_FLAG_COUNT_TRAVERSAL)) != 0 || numPixels == 0 || sppCount == 0 ||
        numPixels > kPrimaryMaxSamples)
        return p;
    if (spectral || environment) return p;      // measured slower with the pass: boxes_spectral 838 -> 850 ms, ibl 283 -> 330 ms per frame
    p.on = true;
    p.passesPerLaunch = std::min(sppCount, kPrimaryMaxSamples / numPixels);
    p.numLaunches = (sppCount + p.passesPerLaunch - 1) / p.passesPerLaunch;
    p.instanceEntries = instanced ? (uint64_t)numPixels * sppCount : 0u;
    // 16 B per sample, what an RGB result entry takes: the plane is as large as the window's results, whatever planWindows made of the
    // budget (a single pass may exceed it, and so may its plane).  Not where the pass's producer wave is the limit (render_plan.h).
    p.rngEntries = instanced || quantized ? 0u : (uint64_t)numPixels * sppCount;
    p.kernel = p.rngEntries && !(configFlags & SLRHIP_FLAG_PRIMARY_RING) ? PrimaryKernel::Direct : PrimaryKernel::Ring;
    return p;
}

ShadeVariant planShadeVariant(bool spectral, bool shadeTables, bool hasMicrofacet, bool hasMulti, uint32_t numTextures, bool primary, bool primaryRng) {
    const bool allLobes = hasMulti || numTextures != 0;
    ShadeVariant v;
    v.spectral = spectral;
    v.ldsTables = shadeTables && !allLobes;
    // The microfacet (GGX) code costs ~45 VGPRs, so scenes without such lobes get kernels without it.
    v.glossy = hasMicrofacet || allLobes;
    v.multi = allLobes;
    v.textures = numTextures != 0;
    v.primary = primary && !spectral;
    v.resume = v.primary && primaryRng;
    return v;
}

ShadeVariant tailVariant(ShadeVariant v) {
    v.primary = v.resume = false;
    return v;
}

// The end of the window (pt_tail_kernels.h): once at most tailSlots slots are alive the traversal kernel raises the tail-mode word
// instead of tracing, the rest of the block of iterations is no-ops, and the tail kernel finishes every remaining path and sample
// in one launch.  The image does not depend on who finishes a sample (the sensor adds in pass order).  On with the automatic slot
// count (slrhip_config::stripes = 0) and on request (SLRHIP_FLAG_TAIL_KERNEL, SLRHIP_TAIL_SLOTS=n); a caller who fixes the slot
// count gets the pure wavefront schedule unless he asks (the parity tests compare the two).  Never for more than numSlots /
// divisor, an eighth of the slots (the wavefront kernels are the efficient way to advance many paths) and not in the counting
// build (its per-ray figures come from the wavefront kernels).  SLRHIP_TAIL_SLOTS=0 turns it off.
uint32_t tailSlots(uint32_t numSlots, uint32_t divisor, bool asked, long envTail, bool available) {
    if (!(asked || envTail > 0) || envTail == 0 || !available) return 0u;
    const uint32_t bound = envTail > 0 ? (uint32_t)std::min<long>(envTail, 0x7FFFFFFFL) : kDefaultTailSlots;
    return std::min(bound, numSlots / divisor);
}

uint32_t adaptiveBlock(uint32_t sppMin, uint32_t sppStep, uint32_t sppMax, uint32_t done) {
    if (sppMin < 2 || sppStep == 0 || sppMax < sppMin || done >= sppMax) return 0u;
    return done == 0 ? sppMin : std::min(sppStep, sppMax - done);
}

std::vector<uint32_t> planAdaptiveBlocks(uint32_t sppMin, uint32_t sppStep, uint32_t sppMax) {
    std::vector<uint32_t> blocks;
    for (uint32_t done = 0, n; (n = adaptiveBlock(sppMin, sppStep, sppMax, done)) != 0; done += n) blocks.push_back(n);
    return blocks;
}

DenoiseScratch denoiseScratch(uint32_t width, uint32_t height, uint32_t components) {
    DenoiseScratch s;
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels == 0 || pixels >= (1ull << 31) || (components != 3 && components != 16)) return s;
    const size_t plane = (size_t)pixels * (components == 3 ? 16u : 64u);
    s.guides = 0;
    s.planes[0] = (size_t)pixels * 16u;
    s.planes[1] = s.planes[0] + plane;
    s.yv[0] = s.planes[1] + plane;
    s.yv[1] = s.yv[0] + (size_t)pixels * 8u;
    s.bytes = s.yv[1] + (size_t)pixels * 8u;               // = pixels x (32 + 2 x (16 or 64)) <= 2^31 x 160
    return s;
}

bool rangesOverlap(const void* a, size_t aBytes, const void* b, size_t bBytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    if (aBytes == 0 || bBytes == 0) return false;
    // a0 < b0 + bBytes && b0 < a0 + aBytes, written without a sum that could wrap
    return a0 < b0 ? b0 - a0 < aBytes : a0 - b0 < bBytes;
}

const char* denoiseRefusal(const slrhip_denoise_desc& d) {
    if (d.reserved != 0) return "reserved must be 0";
    if (d.components != 3 && d.components != 16) return "components must be 3 or 16";
    if (d.iterations < 1 || d.iterations > 8) return "iterations must be 1 .. 8";
    if (d.normal_power_log2 > 7) return "normal_power_log2 must be 0 .. 7";
    if (d.sigma_luminance != d.sigma_luminance || d.sigma_distance != d.sigma_distance) return "a sigma is NaN";
    if (denoiseScratch(d.width, d.height, d.components).bytes == 0) return "width and height must be >= 1 and width * height < 2^31";
    if (!d.color || !d.output) return "null color or output";
    const size_t pixels = (size_t)d.width * d.height, plane = pixels * sizeof(float), frame = plane * d.components;
    struct Range { const void* p; size_t bytes; };
    const Range inputs[5] = {{d.color, frame}, {d.variance, plane}, {d.normal, 3 * plane}, {d.distance, plane}, {d.coverage, plane}};
    const Range outputs[2] = {{d.output, frame}, {d.output_variance, plane}};
    for (const Range& r : inputs) if ((uintptr_t)r.p & 3u) return "a misaligned pointer (4 bytes)";
    for (const Range& r : outputs) if ((uintptr_t)r.p & 3u) return "a misaligned pointer (4 bytes)";
    if ((d.normal || d.distance) && !d.coverage) return "normal and distance need coverage";
    for (const Range& o : outputs)
        for (const Range& in : inputs)
            if (o.p && in.p && rangesOverlap(o.p, o.bytes, in.p, in.bytes)) return "an output overlaps an input";
    if (d.output_variance && rangesOverlap(d.output, frame, d.output_variance, plane)) return "output and output_variance overlap";
    return nullptr;
}

size_t tonemapBytes(uint32_t width, uint32_t height, uint32_t format) {
    const uint64_t pixels = (uint64_t)width * height;
    if (pixels == 0 || pixels >= (1ull << 31)) return 0;
    // 3 * width + width % 4 <= 4 * width: at most 2^33 bytes
    if (format == SLRHIP_IMAGE_BGR8_BMP) return (size_t)(3ull * width + width % 4u) * height;
    if (format == SLRHIP_IMAGE_RGBA8) return (size_t)pixels * 4u;
    return 0;
}

const char* tonemapRefusal(const slrhip_tonemap_desc& d) {
    if (d.reserved != 0) return "reserved must be 0";
    if (d.components != 3 && d.components != 16) return "components must be 3 or 16";
    if (d.format != SLRHIP_IMAGE_BGR8_BMP && d.format != SLRHIP_IMAGE_RGBA8) return "unknown format";
    const size_t bytes = tonemapBytes(d.width, d.height, d.format);
    if (bytes == 0) return "width and height must be >= 1 and width * height < 2^31";
    if (!d.color || !d.output) return "null color or output";
    if (((uintptr_t)d.color | (uintptr_t)d.output) & 3u) return "a misaligned pointer (4 bytes)";
    if (d.output_bytes < bytes) return "output_bytes is less than slrhip_tonemap_bytes";
    const size_t frame = (size_t)d.width * d.height * d.components * sizeof(float);
    if (rangesOverlap(d.output, bytes, d.color, frame)) return "output overlaps color";
    return nullptr;
}

const char* modulateRefusal(const slrhip_modulate_desc& d) {
    if (d.reserved != 0) return "reserved must be 0";
    if (d.components != 3 && d.components != 16) return "components must be 3 or 16";
    if (d.op != SLRHIP_MODULATE_DIVIDE && d.op != SLRHIP_MODULATE_MULTIPLY) return "unknown op";
    const uint64_t pixels = (uint64_t)d.width * d.height;
    if (pixels == 0 || pixels >= (1ull << 31)) return "width and height must be >= 1 and width * height < 2^31";
    if (d.albedo_passes == 0) return "albedo_passes must be >= 1";
    if (!(d.floor > 0.0f) || !(d.floor <= 3.402823466e+38f)) return "floor must be finite and > 0";
    if (!d.color || !d.albedo || !d.output) return "null color, albedo or output";
    if (((uintptr_t)d.color | (uintptr_t)d.variance | (uintptr_t)d.albedo | (uintptr_t)d.output | (uintptr_t)d.output_variance) & 3u)
        return "a misaligned pointer (4 bytes)";
    if (d.output_variance && !d.variance) return "output_variance needs variance";
    const size_t plane = (size_t)pixels * sizeof(float), frame = plane * d.components;
    // an output may be exactly its own input (in place); every other overlap of an output with a buffer of the call is refused
    if (d.output != d.color && rangesOverlap(d.output, frame, d.color, frame)) return "output overlaps color without being equal to it";
    if (rangesOverlap(d.output, frame, d.albedo, frame)) return "output overlaps albedo";
    if (d.variance && rangesOverlap(d.output, frame, d.variance, plane)) return "output overlaps variance";
    if (d.output_variance) {
        if (d.output_variance != d.variance && rangesOverlap(d.output_variance, plane, d.variance, plane)) return "output_variance overlaps variance without being equal to it";
        if (rangesOverlap(d.output_variance, plane, d.color, frame)) return "output_variance overlaps color";
        if (rangesOverlap(d.output_variance, plane, d.albedo, frame)) return "output_variance overlaps albedo";
        if (rangesOverlap(d.output_variance, plane, d.output, frame)) return "output_variance overlaps output";
    }
    return nullptr;
}

// the layouts the Python mirrors (slr_amd/abi.py) restate
static_assert(sizeof(slrhip_reproject_desc) == 168 && offsetof(slrhip_reproject_desc, color) == 16 && offsetof(slrhip_reproject_desc, prev_color) == 64 &&
              offsetof(slrhip_reproject_desc, output) == 120 && offsetof(slrhip_reproject_desc, max_history) == 144 &&
              offsetof(slrhip_reproject_desc, reserved) == 160, "slrhip_reproject_desc's layout");
static_assert(sizeof(slrhip_motion_desc) == 24 && offsetof(slrhip_motion_desc, previous_transforms) == 8 && offsetof(slrhip_motion_desc, reserved) == 16,
              "slrhip_motion_desc's layout");

const char* reprojectRefusal(const slrhip_reproject_desc& d) {
    if (d.reserved[0] != 0 || d.reserved[1] != 0) return "reserved must be 0";
    if (d.components != 3 && d.components != 16) return "components must be 3 or 16";
    const uint64_t pixels = (uint64_t)d.width * d.height;
    if (pixels == 0 || pixels >= (1ull << 31)) return "width and height must be >= 1 and width * height < 2^31";
    if (d.max_history != d.max_history || d.min_alpha != d.min_alpha || d.sigma_distance != d.sigma_distance || d.min_normal_dot != d.min_normal_dot)
        return "a parameter is NaN";
    if (!(d.max_history >= 1.0f)) return "max_history must be >= 1";
    if (!(d.min_alpha >= 0.0f) || !(d.min_alpha <= 1.0f)) return "min_alpha must be 0 .. 1";
    if (!d.color || !d.motion || !d.coverage) return "null color, motion or coverage";
    if (!d.prev_color || !d.prev_length || !d.prev_distance || !d.prev_coverage) return "null prev_color, prev_length, prev_distance or prev_coverage";
    if (!d.output || !d.output_length) return "null output or output_length";
    if ((d.variance != nullptr) != (d.prev_variance != nullptr)) return "variance and prev_variance go together";
    if ((d.ids != nullptr) != (d.prev_ids != nullptr)) return "ids and prev_ids go together";
    if ((d.normal != nullptr) != (d.prev_normal != nullptr)) return "normal and prev_normal go together";
    if (d.output_variance && !d.variance) return "output_variance needs variance";
    const size_t plane = (size_t)pixels * sizeof(float), frame = plane * d.components;
    struct Range { const void* p; size_t bytes; };
    const Range inputs[13] = {{d.color, frame}, {d.variance, plane}, {d.motion, 4 * plane}, {d.coverage, plane}, {d.ids, 3 * plane}, {d.normal, 3 * plane},
                              {d.prev_color, frame}, {d.prev_variance, plane}, {d.prev_length, plane}, {d.prev_distance, plane}, {d.prev_coverage, plane},
                              {d.prev_ids, 3 * plane}, {d.prev_normal, 3 * plane}};
    const Range outputs[3] = {{d.output, frame}, {d.output_variance, plane}, {d.output_length, plane}};
    for (const Range& r : inputs) if ((uintptr_t)r.p & 3u) return "a misaligned pointer (4 bytes)";
    for (const Range& r : outputs) if ((uintptr_t)r.p & 3u) return "a misaligned pointer (4 bytes)";
    for (const Range& o : outputs)
        for (const Range& in : inputs)
            if (o.p && in.p && rangesOverlap(o.p, o.bytes, in.p, in.bytes)) return "an output overlaps an input";
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (outputs[a].p && outputs[b].p && rangesOverlap(outputs[a].p, outputs[a].bytes, outputs[b].p, outputs[b].bytes)) return "two outputs overlap";
    return nullptr;
}

int motionRefusal(bool haveRender, uint32_t numInstances, const slrhip_motion_desc* d, uint32_t sppBegin, uint32_t sppCount, const char** what) {
    *what = nullptr;
    if (!d) { *what = "null descriptor"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (d->reserved[0] != 0 || d->reserved[1] != 0) { *what = "reserved must be 0"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if ((uintptr_t)d->previous_transforms & 15u) { *what = "misaligned previous_transforms (16 bytes)"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if ((uint64_t)sppBegin + sppCount > 0xFFFFFFFFull) { *what = "pass range beyond 2^32"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (!haveRender) { *what = "call slrhip_render_begin first"; return SLRHIP_ERR_NO_SCENE; }
    if (d->previous_transforms && numInstances == 0) { *what = "previous_transforms given, but the scene has no instances"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    return SLRHIP_OK;
}

static_assert(sizeof(slrhip_motion_vertices_desc) == 40 && offsetof(slrhip_motion_vertices_desc, frame) == 0 &&
              offsetof(slrhip_motion_vertices_desc, previous_vertices) == 24 && offsetof(slrhip_motion_vertices_desc, reserved) == 32,
              "slrhip_motion_vertices_desc's layout");

int motionVerticesRefusal(bool haveRender, uint32_t numInstances, uint32_t flags, uint32_t treeBuilder, const slrhip_motion_vertices_desc* d,
                          uint32_t sppBegin, uint32_t sppCount, const char** what) {
    *what = nullptr;
    if (!d) { *what = "null descriptor"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (d->reserved != 0) { *what = "reserved must be 0"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if ((uintptr_t)d->previous_vertices & 3u) { *what = "misaligned previous_vertices (4 bytes)"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (const int rc = motionRefusal(haveRender, numInstances, &d->frame, sppBegin, sppCount, what)) return rc;
    if (!d->previous_vertices) return SLRHIP_OK;
    // the context keeps the vertex and index arrays exactly where slrhip_set_vertices works (geometryUpdateRefusal2)
    if (!(flags & SLRHIP_FLAG_DYNAMIC_GEOMETRY)) {
        *what = "previous_vertices given, but the context was created without SLRHIP_FLAG_DYNAMIC_GEOMETRY";
        return SLRHIP_ERR_UNSUPPORTED;
    }
    if ((numInstances != 0 || treeBuilder == 3u) && !(flags & SLRHIP_FLAG_DYNAMIC_INSTANCED)) {
        *what = "previous_vertices given, but the scene has instances and the context was created without SLRHIP_FLAG_DYNAMIC_INSTANCED";
        return SLRHIP_ERR_UNSUPPORTED;
    }
    if (treeBuilder == 1u) { *what = "previous_vertices given, but the tree was built with spatial splits"; return SLRHIP_ERR_UNSUPPORTED; }
    return SLRHIP_OK;
}

const char* environmentRefusal(const slrhip_environment_desc& d) {
    if (d.reserved[0] != 0 || d.reserved[1] != 0) return "reserved must be 0";
    if (d.flags & ~(SLRHIP_ENV_TEXELS_RGB | SLRHIP_ENV_STORE_HALF)) return "unknown flag bits";
    if (d.width < 4 || d.height < 4 || d.width > 32768 || d.height > 32768 || d.width % 4 || d.height % 4)
        return "width and height must be multiples of 4 in 4 .. 32768";
    if (!d.texels) return "null texels";
    if ((uintptr_t)d.texels & 15u) return "misaligned texels (16 bytes)";
    if (!(d.scale >= 0.0f) || !(d.scale <= 3.402823466e+38f)) return "scale must be finite and >= 0";
    return nullptr;
}

int instanceUpdateRefusal(bool haveScene, uint32_t numInstances, const void* deviceSrc, uint32_t first, uint32_t count, const char** what) {
    if (!deviceSrc) { *what = "null device_src"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if ((uintptr_t)deviceSrc & 15u) { *what = "misaligned device_src (16 bytes)"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (count == 0) { *what = "count must be >= 1"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (!haveScene) { *what = "no scene uploaded"; return SLRHIP_ERR_NO_SCENE; }
    if (numInstances == 0) { *what = "the scene has no instances"; return SLRHIP_ERR_UNSUPPORTED; }
    if (first >= numInstances || count > numInstances - first) { *what = "first_instance + count is beyond the scene's instances"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    *what = nullptr;
    return SLRHIP_OK;
}

int topLevelRebuildRefusal(bool haveScene, uint32_t numInstances, const char** what) {
    if (!haveScene) { *what = "no scene uploaded"; return SLRHIP_ERR_NO_SCENE; }
    if (numInstances == 0) { *what = "the scene has no instances"; return SLRHIP_ERR_UNSUPPORTED; }
    *what = nullptr;
    return SLRHIP_OK;
}

int geometryUpdateRefusal(bool haveScene, bool dynamic, uint32_t treeBuilder, uint32_t numInstances, uint32_t numVertices, const void* deviceSrc,
                          uint32_t first, uint32_t count, const char** what) {
    return geometryUpdateRefusal2(haveScene, dynamic, false, treeBuilder, numInstances, numVertices, deviceSrc, first, count, what);
}

int geometryUpdateRefusal2(bool haveScene, bool dynamic, bool instancedKept, uint32_t treeBuilder, uint32_t numInstances, uint32_t numVertices,
                           const void* deviceSrc, uint32_t first, uint32_t count, const char** what) {
    if (!deviceSrc) { *what = "null device_src"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if ((uintptr_t)deviceSrc & 3u) { *what = "misaligned device_src (4 bytes)"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (count == 0) { *what = "count must be >= 1"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    if (!haveScene) { *what = "no scene uploaded"; return SLRHIP_ERR_NO_SCENE; }
    if (!dynamic) { *what = "the context was created without SLRHIP_FLAG_DYNAMIC_GEOMETRY"; return SLRHIP_ERR_UNSUPPORTED; }
    if ((numInstances != 0 || treeBuilder == 3u) && !instancedKept) { *what = "the scene has instances"; return SLRHIP_ERR_UNSUPPORTED; }
    if (treeBuilder == 1u) { *what = "the tree was built with spatial splits"; return SLRHIP_ERR_UNSUPPORTED; }
    if (first >= numVertices || count > numVertices - first) { *what = "first_vertex + count is beyond the scene's vertices"; return SLRHIP_ERR_INVALID_ARGUMENT; }
    *what = nullptr;
    return SLRHIP_OK;
}

} // namespace slrhip

extern "C" size_t slrhip_tonemap_bytes(uint32_t width, uint32_t height, uint32_t format) {
    return slrhip::tonemapBytes(width, height, format);
}

extern "C" size_t slrhip_denoise_scratch_bytes(uint32_t width, uint32_t height, uint32_t components) {
    return slrhip::denoiseScratch(width, height, components).bytes;
}
