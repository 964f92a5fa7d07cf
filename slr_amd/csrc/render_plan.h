// render_plan.h — the host half of the render set-up: every decision of slrhip_render_begin / slrhip_render that is integer
// arithmetic (the shard's pixel list, the slot count, the result windows, their run lengths, the tail-kernel bound), with no device
// call, no context state and no environment variable: every override comes in as an argument (see render_plan.cpp).
// slrhip_api.hip and slrhip_buffers.hip allocate and launch from the result; slrhip_debug_render_plan (include/slrhip_debug.h) shows it to the tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/slrhip.h"
#include "device_types.h"

namespace slrhip {

const uint32_t kDefaultRunLength = 64;         // SLRHIP_RUN_LENGTH: passes of a pixel a wave takes in a row (pt_kernels.h WorkItem; measured: DESIGN.md)
const uint64_t kFeatureRecordBytes = 512ull << 20;      // the record window of the feature and the albedo passes (featureWindow)
const uint32_t kDefaultTailSlots = 1u << 18;   // SLRHIP_TAIL_SLOTS: measured on the headline frame and its N = 8 shard

struct FramePlan {
    uint32_t width = 0, height = 0;
    uint32_t shardIndex = 0, shardCount = 1;
    bool spectral = false;
    uint32_t numPixels = 0;                    // pixels of this shard; 0 = the shard owns no tile
    uint32_t stripes = 1;                      // slots per pixel: the caller's, or the automatic choice
    uint32_t numSlots = 0;                     // paths in flight, a multiple of 256; 0 for an empty shard
    size_t slotCapacity = 256;                 // elements of the per-slot arrays: numSlots, or one block for an empty shard
    uint32_t numBlocks = 1;                    // slotCapacity / 256
    uint32_t shardCapacity = 256;              // entries per queue region = ceil(numBlocks / kShards) * 256
    uint32_t rayStride = 1, spStride = 1, hdrStride = 1;      // PathBuffers: 2 = the pair shares one array
};

// The checks of slrhip_render_begin on the frame and the shard, then the sizes.  `configStripes` is slrhip_config::stripes (0 =
// automatic), `autoStripesOverride` replaces the automatic choice when it is in 1 .. 64, `pairs` is the SLRHIP_PAIRS mask.
// Returns SLRHIP_OK, or SLRHIP_ERR_INVALID_ARGUMENT with the message in *err.  Costs one step per row of tiles: the shard's
// pixels are counted, not listed, so a frame that will be refused is refused before anything of its size exists.
int planFrame(int32_t width, int32_t height, uint32_t shardIndex, uint32_t shardCount, uint32_t configStripes, bool spectral,
              long autoStripesOverride, int pairs, FramePlan* out, std::string* err);

// The shard's pixels as x | y << 16 (plan.numPixels entries), or the single placeholder 0xFFFFFFFF for an empty shard.
std::vector<uint32_t> shardPixels(const FramePlan& plan);

// Passes per result window of a call of `sppCount` passes over `numPixels` (> 0) pixels with `budgetBytes` for the window.
uint32_t planWindows(uint32_t numPixels, bool spectral, uint32_t sppCount, uint64_t budgetBytes);

// Passes per launch of slrhip_render_features / slrhip_render_albedo over `numPixels` (> 0) pixels: the length of their record window.
uint32_t featureWindow(uint32_t numPixels, bool wantB2);

struct WindowPlan {
    uint32_t workItems;                        // numPixels x sppCount
    uint32_t runLength;                        // passes per run (divides sppCount)
    uint32_t numRuns;                          // numPixels x sppCount / runLength
};
// One window of `sppCount` passes; `runLengthOverride` (0 = none) replaces kDefaultRunLength as the longest run.
WindowPlan planWindow(uint32_t numPixels, uint32_t sppCount, uint32_t runLengthOverride);

// The primary pass of a window (pt_kernels.h launchPrimary): the camera ray of every sample of the window traced before its first
// iteration, the hit record kept in the sample's entry of the result window.  Off with SLRHIP_FLAG_NO_PRIMARY_PASS, and with
// SLRHIP_FLAG_COUNT_TRAVERSAL: the nodes and triangles per ray are counted by the wavefront kernels, and they are properties of the
// rays, not of the schedule.  A launch numbers its samples in 31 bits, so the window's passes go in groups of passesPerLaunch.
const uint32_t kPrimaryMaxSamples = 0x7FFFFFFFu;        // ring indices of one launch (pt_trace_ws.h, wsProduceIndexed)
struct PrimaryPlan {
    bool on = false;
    PrimaryKernel kernel = PrimaryKernel::None;      // the kernel of the pass's launches (below); None: the pass is off
    uint32_t passesPerLaunch = 0;              // numPixels x passesPerLaunch <= kPrimaryMaxSamples
    uint32_t numLaunches = 0;                  // ceil(sppCount / passesPerLaunch)
    uint64_t instanceEntries = 0;              // int32 entries of PathBuffers::primaryInstance: numPixels x sppCount in instanced scenes, else 0
    uint64_t rngEntries = 0;                   // uint4 entries of PathBuffers::primaryRng: numPixels x sppCount when the pass is on and keeps the plane, else 0
};
// Two classes of render keep the pass off because it measured slower there: spectral contexts (`spectral`) and
// scenes with an environment light (`environment`: many camera rays leave the scene, their paths end in the fused visit and the
// slot waits for the next launch).
// `quantized`: the scene's tree is the quantized one (large scenes).  There and in instanced scenes the pass runs 15 (or 7) consumer waves
// per producer and the producer wave is its limit: the stream plane stays off (rngEntries 0), the fused start seeds its own stream as
// before — with the plane grid10m rendered 0.6 % slower, the producer's +30 ms against k_shade's -20 ms.
// The kernel: exactly where the pass keeps the stream plane — no instances, tree not quantized — it is the direct kernel
// (pt_primary_direct.hip: the lane that traces a camera ray makes it; the 64 samples of a wave are passes of one pixel and walk the
// tree together), unless SLRHIP_FLAG_PRIMARY_RING keeps the ring kernel on (the comparator); everywhere else the ring
// kernel (pt_trace_indexed.hip) as before: the direct kernel's traversal has no quantized-node path, and on large and instanced trees
// the rays of a pixel part ways at the leaves.
PrimaryPlan planPrimary(uint32_t numPixels, uint32_t sppCount, uint32_t configFlags, bool instanced, bool spectral, bool environment,
                        bool quantized = false);

// The k_shade instantiation of a window, from what the scene and the window's plan say: the context's mode, DevScene::shadeTables
// != nullptr (the tables fit the LDS limits), ::hasMicrofacet, ::hasMulti, ::numTextures, RenderParams::primary and
// PathBuffers::primaryRng != nullptr (the pass keeps the stream plane).  MultiBSDF and textured scenes run one all-lobes kernel per
// mode with the tables in HBM (a component is re-read per use), and the textured one has the MultiBSDF code too; the fused start is
// built for RGB only (planPrimary keeps the pass off in spectral contexts), and only it can resume a stream.
ShadeVariant planShadeVariant(bool spectral, bool shadeTables, bool hasMicrofacet, bool hasMulti, uint32_t numTextures, bool primary, bool primaryRng);
// ... and the k_tail instantiation that finishes its window: the same code without a start of its own.
ShadeVariant tailVariant(ShadeVariant v);

// RenderParams::tailSlots of a window: 0 = the tail kernel stays off.  `asked`: the caller's flag or the automatic slot count;
// `envTail`: SLRHIP_TAIL_SLOTS (-1 = unset, 0 = off, n = the bound); `available`: the context does not count traversal steps
// (every shade kernel has its tail kernel); never more than numSlots / `divisor` (SLR_TAIL_DIVISOR of slrhip_api.hip).
uint32_t tailSlots(uint32_t numSlots, uint32_t divisor, bool asked, long envTail, bool available);

// The blocks of a slrhip_render_adaptive call, as pass counts: sppMin (>= 2), then sppStep (>= 1) as often as it fits, the last one
// cut so that the sum is sppMax (>= sppMin).  A retirement check follows every block; the windows of a block come from
// planWindows / planWindow with the active pixel count.  adaptiveBlock: the block that follows `done` passes of the call (0: the
// call is complete, or the triple is one the entry point refuses) — what the render loop asks for, block by block;
// planAdaptiveBlocks: the whole list from the same function (one entry per block: for the tests and tools, not for 2^32 passes).
uint32_t adaptiveBlock(uint32_t sppMin, uint32_t sppStep, uint32_t sppMax, uint32_t done);
std::vector<uint32_t> planAdaptiveBlocks(uint32_t sppMin, uint32_t sppStep, uint32_t sppMax);

// The scratch of slrhip_denoise, in the order it is cut up: guide records (16 B per pixel), the two colour planes (16 B per pixel
// for 3 components, 64 B for 16), the two {Y, v} planes (8 B per pixel): every offset is a multiple of the record that lives there.
// bytes = 0 for a size the entry point refuses (a zero side, width * height >= 2^31, components other than 3 or 16).
struct DenoiseScratch {
    size_t guides = 0, planes[2] = {0, 0}, yv[2] = {0, 0};   // byte offsets
    size_t bytes = 0;
};
DenoiseScratch denoiseScratch(uint32_t width, uint32_t height, uint32_t components);

// The argument checks of slrhip_denoise on the descriptor: nullptr if the call goes ahead, else what is wrong with it.
const char* denoiseRefusal(const slrhip_denoise_desc& d);

// Do the byte ranges [a, a + aBytes) and [b, b + bBytes) share a byte?  An empty range shares none.
bool rangesOverlap(const void* a, size_t aBytes, const void* b, size_t bBytes);

// The image slrhip_tonemap writes (= slrhip_tonemap_bytes): rows of 3 * width + width % 4 bytes (SLRHIP_IMAGE_BGR8_BMP) or of
// 4 * width bytes (SLRHIP_IMAGE_RGBA8).  0 for what the entry point refuses: a zero side, width * height >= 2^31, an unknown format.
size_t tonemapBytes(uint32_t width, uint32_t height, uint32_t format);
// The argument checks of slrhip_tonemap on the descriptor: nullptr if the call goes ahead, else what is wrong with it.
const char* tonemapRefusal(const slrhip_tonemap_desc& d);
// The argument checks of slrhip_modulate on the descriptor: nullptr if the call goes ahead, else what is wrong with it.
const char* modulateRefusal(const slrhip_modulate_desc& d);
// The argument checks of slrhip_reproject on the descriptor (the pointers are only compared, never followed): nullptr if the call goes
// ahead, else what is wrong with it.
const char* reprojectRefusal(const slrhip_reproject_desc& d);
// The argument checks of slrhip_render_motion against what the context holds (a render state or none, the scene's number of instances;
// the pointers are only compared, never followed, `d` may be null): SLRHIP_OK if the call goes ahead, else the code it returns with
// *what = what is wrong.
int motionRefusal(bool haveRender, uint32_t numInstances, const slrhip_motion_desc* d, uint32_t sppBegin, uint32_t sppCount, const char** what);
// The argument checks of slrhip_render_motion_vertices: the outer descriptor's own, then motionRefusal on its `frame`, then — only where
// previous_vertices is given — whether the context keeps the vertex and index arrays (flags: its slrhip_config::flags; treeBuilder: the
// builder behind the scene's tree as include/slrhip_debug.h numbers them).  Codes and *what as above.
int motionVerticesRefusal(bool haveRender, uint32_t numInstances, uint32_t flags, uint32_t treeBuilder, const slrhip_motion_vertices_desc* d,
                          uint32_t sppBegin, uint32_t sppCount, const char** what);
// The argument checks of slrhip_set_environment on the descriptor (the pointer is only compared, never followed): nullptr if the
// call goes ahead, else what is wrong with it.  What depends on the context (no scene, no upsampling tables) is the entry point's.
const char* environmentRefusal(const slrhip_environment_desc& d);
// The argument checks of slrhip_set_instance_transforms against what the context holds (a scene or none, its number of instances; the
// pointer is only compared, never followed): SLRHIP_OK if the call goes ahead, else the code it returns with *what = what is wrong.
int instanceUpdateRefusal(bool haveScene, uint32_t numInstances, const void* deviceSrc, uint32_t first, uint32_t count, const char** what);
// The checks of slrhip_rebuild_top_level and slrhip_top_level_cost against what the context holds (a scene or none, its number of
// instances): SLRHIP_OK if the call goes ahead, else the code it returns with *what = what is wrong.
int topLevelRebuildRefusal(bool haveScene, uint32_t numInstances, const char** what);
// The argument checks of slrhip_set_vertices against what the context holds (a scene or none, created with SLRHIP_FLAG_DYNAMIC_GEOMETRY
// or not, the builder behind the scene's tree as include/slrhip_debug.h numbers them, its numbers of instances and vertices; the pointer
// is only compared, never followed): SLRHIP_OK if the call goes ahead, else the code it returns with *what = what is wrong.
int geometryUpdateRefusal(bool haveScene, bool dynamic, uint32_t treeBuilder, uint32_t numInstances, uint32_t numVertices, const void* deviceSrc,
                          uint32_t first, uint32_t count, const char** what);
// The same checks for a context that may keep what the call needs of a scene WITH instances (instancedKept: created with
// SLRHIP_FLAG_DYNAMIC_INSTANCED as well): then instances are no refusal; everything else, and every message, is as above.  This is the
// one slrhip_set_vertices calls; geometryUpdateRefusal is it with instancedKept = false.
int geometryUpdateRefusal2(bool haveScene, bool dynamic, bool instancedKept, uint32_t treeBuilder, uint32_t numInstances, uint32_t numVertices,
                           const void* deviceSrc, uint32_t first, uint32_t count, const char** what);

} // namespace slrhip
