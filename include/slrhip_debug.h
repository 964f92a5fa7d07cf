/*
 * slrhip_debug.h — diagnostic exports of libslrhip.so that are NOT part of the drop-in boundary (include/slrhip.h).
 * They exist for the parity tests: function-level checks of the device code against the reference's own answers.
 */
#ifndef SLRHIP_DEBUG_H
#define SLRHIP_DEBUG_H

#include "slrhip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Function-level BSDF queries against material `material` of the uploaded scene,
 * through the same device functions the shading kernel calls: BSDF::sample / evaluate /
 * evaluatePDF (libSLR/Core/directional_distribution_functions.h:231-279; flags = All, non-adjoint) on the
 * BSDF that SurfaceMaterial::getBSDF (libSLR/Core/surface_material.h:22) builds for wavelengths
 * WavelengthSamples::createWithEqualOffsets(wl_offset, u_lambda) (libSLR/BasicTypes/SpectrumTypes.h:54-64).
 *   queries[12 i ..]     = dirOut_sn[3], gNormal_sn[3], dirIn_sn[3], uComponent, uDir[2]
 *   out[(6 + 2C) i ..]   = sampled dir_sn[3], dirPDF, dirType, fs(sample)[C], fs(evaluate)[C],
 *                          evaluatePDF        (C = slrhip_components; zeros when dirPDF == 0)
 * Directions are in the shading frame (z = shading normal).  Host arrays; synchronises.        */
int slrhip_bsdf_queries(slrhip_ctx* ctx, uint32_t material, uint32_t n, const float* queries,
                        float wl_offset, float u_lambda, float* out);

/* The work distribution of a render window (slr_amd/csrc/pt_kernels.h, WorkItem), evaluated on the HOST with the very function
 * the kernels call: the samples (pixel, pass) of a window of `num_passes` passes over `num_pixels` pixels are dealt to the
 * `num_slots / 64` wave queues in runs of `run_length` passes of a pixel.  counts[pass * num_pixels + pixel] receives how many
 * times the sample comes up over all queues (the caller checks: exactly once); queue_lengths[wave] the samples of each queue.
 * No GPU is touched.  Returns SLRHIP_OK, or SLRHIP_ERR_INVALID_ARGUMENT when run_length does not divide num_passes.            */
int slrhip_debug_work_distribution(uint32_t num_pixels, uint32_t num_slots, uint32_t num_passes, uint32_t run_length,
                                   uint32_t* counts, uint32_t* queue_lengths);

/* The render plan (slr_amd/csrc/render_plan.h), evaluated on the HOST with the very functions slrhip_render_begin and slrhip_render
 * call: a frame of width x height, shard shard_index of shard_count, slrhip_config::stripes (0 = automatic) and mode, then a call
 * of `num_passes` passes with `budget_bytes` for the result window.  plan[0..3] receive the shard's pixel count, the stripes, the
 * path slots and the passes per window; *num_windows the number of windows of the call; windows[2 k], windows[2 k + 1] the pass
 * count and the run length of window k, for the first `max_windows` windows.  If `pixels` is not NULL it receives the shard's pixel
 * list (x | y << 16, plan[0] entries; `max_pixels` is its capacity).  No GPU is touched.  Returns SLRHIP_OK, or what
 * slrhip_render_begin returns for the same frame and shard, with its message.                                                  */
int slrhip_debug_render_plan(int32_t width, int32_t height, uint32_t shard_index, uint32_t shard_count, uint32_t stripes, int32_t mode,
                             uint32_t num_passes, uint64_t budget_bytes, uint32_t* plan, uint32_t* windows, uint32_t max_windows,
                             uint32_t* num_windows, uint32_t* pixels, uint32_t max_pixels);

/* The primary pass of a result window (slr_amd/csrc/render_plan.h, planPrimary), evaluated on the HOST with the very function the render
 * calls: a window of `num_passes` passes over `num_pixels` pixels in a context with slrhip_config::flags `config_flags`; `scene_class`
 * bit 0: the scene has instanced meshes, bit 1: the context is spectral, bit 2: the scene has an environment light (the last two keep the
 * pass off).  plan[0] = 1 if the pass runs (0: off, and the rest is 0), plan[1] = passes per launch
 * (num_pixels x plan[1] < 2^31), plan[2] = launches, plan[3] = 1 if the int32 instance plane is allocated.  No GPU is touched.          */
int slrhip_debug_primary_plan(uint32_t num_pixels, uint32_t num_passes, uint32_t config_flags, int32_t scene_class, uint32_t* plan);

/* How many samples since slrhip_render_begin took their first hit from the primary pass's record (counted on the device by the kernels
 * that start samples): equal to slrhip_counters::samples when the pass is on, 0 when it is off — a silently disabled pass cannot pass
 * for a working one.  Synchronises.                                                                                                 */
int slrhip_debug_primary_samples(slrhip_ctx* ctx, uint64_t* samples);

/* How many light samples since slrhip_render_begin the shade kernel did not trace because they decide nothing (a contribution of exact
 * zeros that leaves the path's Kahan sum as it is).  They are part of slrhip_counters::shadow_rays — the rays the
 * algorithm casts — and of no traversal figure.  0 in spectral contexts, with SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS and with
 * SLRHIP_FLAG_COUNT_TRAVERSAL.  Synchronises.                                                                                        */
int slrhip_debug_shadow_skipped(slrhip_ctx* ctx, uint64_t* rays);

/* The predicate the shade kernel decides that with (slr_amd/csrc/pt_device.h, deadLightSample), on device `device`, for `n` triples:
 * triples[9 i ..] = the path's radiance sum r[3], its compensation c[3], the light sample's contribution[3]; dead[i] = 1 where every
 * component of the contribution is +0 or -0 AND the compensated add of it leaves all six words of (r, c) bit for bit as they are,
 * else 0.  Host arrays; synchronises.                                                                                                */
int slrhip_debug_dead_light_samples(int32_t device, uint32_t n, const float* triples, uint32_t* dead);

/* Where a launch of the primary pass puts its samples (slr_amd/csrc/pt_kernels.h, primaryLaunchEntry), evaluated on the HOST with the very
 * function its kernel calls: the launch takes the passes [first_pass, first_pass + num_passes) of a window of `window_passes` passes over
 * `num_pixels` pixels and numbers its samples with the pass fastest; entries[i] = the entry of sample i in the result window and in the
 * planes beside it (num_pixels x num_passes of them; expected: pixel x window_passes + first_pass + pass).  No GPU is touched.
 * SLRHIP_ERR_INVALID_ARGUMENT for a null pointer, no pass, passes outside the window, or 2^31 samples and more.                       */
int slrhip_debug_primary_entries(uint32_t num_pixels, uint32_t first_pass, uint32_t num_passes, uint32_t window_passes, uint64_t* entries);

/* The plan of that plane (slr_amd/csrc/render_plan.h, planPrimary), evaluated on the HOST with the function the render calls: the
 * arguments of slrhip_debug_primary_plan, with bit 3 of `scene_class` for a scene whose tree is the quantized one (65 536 nodes and more).
 * *entries = num_pixels x num_passes where the pass runs AND keeps the plane (scenes without instances on a tree that is not quantized),
 * else 0.  No GPU is touched.                                                                                                         */
int slrhip_debug_primary_stream_plan(uint32_t num_pixels, uint32_t num_passes, uint32_t config_flags, int32_t scene_class, uint64_t* entries);

/* The entries of the plane that carries every sample's stream from the primary pass to the launch that starts the sample, as the last
 * window of the context bound it: pixels x passes of that window when it ran the pass, 0 when it did not (no plane is bound then).    */
int slrhip_debug_primary_stream_entries(slrhip_ctx* ctx, uint64_t* entries);

/* The kernel of a window's primary pass (slr_amd/csrc/render_plan.h, PrimaryPlan::kernel), evaluated on the HOST with the function the
 * render calls: the arguments of slrhip_debug_primary_stream_plan.  *direct = 1 where the pass runs the direct kernel (one lane makes,
 * traces and stores a sample: scenes without instances whose tree is not the quantized one, without SLRHIP_FLAG_PRIMARY_RING), 0 where it
 * runs the ring kernel or does not run at all (slrhip_debug_primary_plan's plan[0] tells the two apart).  No GPU is touched.              */
int slrhip_debug_primary_kernel_plan(uint32_t num_pixels, uint32_t num_passes, uint32_t config_flags, int32_t scene_class, uint32_t* direct);

/* The kernel the primary pass of the context's last window was launched with: 0 = that window ran no pass, 1 = the ring kernel, 2 = the
 * direct kernel — so that a test can tell that it compared what it meant to.                                                             */
int slrhip_debug_primary_kernel(slrhip_ctx* ctx, uint32_t* kernel);

/* The k_shade instantiation of a window (slr_amd/csrc/render_plan.h, planShadeVariant), evaluated on the HOST with the function the render
 * calls, from what the render looks at: the context's mode (`spectral`), whether the scene's shading tables fit the LDS limits
 * (`shade_tables`), whether it has a microfacet lobe, a MultiBSDF material, how many textures, whether the window runs the primary pass
 * (`primary`) and keeps its stream plane (`primary_rng`).  plan[0..6] = the instantiation: spectral, tables in LDS, glossy lobes,
 * MultiBSDF code, texture code, fused start (PRIMARY), resumed stream (RESUME), 0 or 1 each; plan[7] = 1 where the table of built kernels
 * (slr_amd/csrc/pt_shade.hip) has that k_shade, plan[8] = 1 where it has the k_tail that finishes its windows.  No GPU is touched.      */
int slrhip_debug_shade_plan(uint32_t spectral, uint32_t shade_tables, uint32_t has_microfacet, uint32_t has_multi, uint32_t num_textures,
                            uint32_t primary, uint32_t primary_rng, uint32_t* plan);

/* The k_shade instantiation of the context's last window, recorded on the host where it is launched: kernel[0..6] as plan[0..6] above,
 * kernel[7] = 1 once that window launched it, kernel[8] = 1 once the tail kernel, its twin without a start of its own, finished the
 * window — so that a test can tell which kernels it compared.                                                                          */
int slrhip_debug_shade_kernel(slrhip_ctx* ctx, uint32_t* kernel);

/* One launch of the primary pass of the render last begun on `ctx` (slrhip_render_begin: its pixel list, seed, camera and image size),
 * with the kernel named: `kernel` 0 = ring, 1 = direct.  The launch takes the passes [first_pass, first_pass + num_passes) of a window of
 * `window_passes` passes that starts at pass 0 of the render, and writes into the caller's DEVICE memory laid out as the window is:
 * records[pixel x window_passes + pass] = {triangle, t, b1, b2} (16 bytes; in a spectral context the first 16 of 64), and — unless
 * `streams` is null — streams[the same entry] = the sample's xorshift128 state behind the camera draws (16 bytes).  Entries outside the
 * launch's passes are not touched.  The rays are counted as any primary launch counts them (slrhip_counters::extension_rays).
 * Synchronises; a device-side error word set by the launch is SLRHIP_ERR_HIP.  SLRHIP_ERR_UNSUPPORTED: `kernel` = 1 on a scene with
 * instances or on the quantized tree.  SLRHIP_ERR_INVALID_ARGUMENT as slrhip_debug_primary_entries.                                      */
int slrhip_debug_primary_pass(slrhip_ctx* ctx, uint32_t kernel, uint32_t first_pass, uint32_t num_passes, uint32_t window_passes, void* records,
                              void* streams);

/* The camera draws of `n` samples on device `device`, forward and recovered (slr_amd/csrc/pt_camera.h): tuples[4 i ..] = seed, pixel x,
 * pixel y, pass; out[16 i ..] = the draws drawCameraSample makes (p.x, p.y, wavelength offset, wavelength selection, two lens draws; float
 * bits), the four words of the stream it leaves, and the same six draws as recoverCameraDraws rebuilds them from that stream and the
 * pixel.  Host arrays; synchronises.                                                                                                */
int slrhip_debug_camera_draws(int32_t device, uint32_t n, const uint32_t* tuples, uint32_t* out);

/* The blocks of a slrhip_render_adaptive call(slr_amd/csrc/render_plan.h, planAdaptiveBlocks), evaluated on the HOST with the
 * function the call asks for its next block: blocks[k] = passes of block k for the first `max_blocks` blocks, *num_blocks = their number (0 for a
 * triple the entry point refuses).  No GPU is touched.                                                                          */
int slrhip_debug_adaptive_blocks(uint32_t spp_min, uint32_t spp_step, uint32_t spp_max, uint32_t* blocks, uint32_t max_blocks,
                                 uint32_t* num_blocks);

/* The argument checks of slrhip_modulate on a descriptor (slr_amd/csrc/render_plan.h, modulateRefusal), evaluated on the HOST with the
 * function the entry point calls: SLRHIP_OK if the call would go ahead, else SLRHIP_ERR_INVALID_ARGUMENT with the reason in
 * slrhip_last_error_string.  The pointers are only compared, never followed.  No GPU is touched.                                  */
int slrhip_debug_modulate_check(const slrhip_modulate_desc* desc);

/* The argument checks of slrhip_reproject on a descriptor (slr_amd/csrc/render_plan.h, reprojectRefusal), evaluated on the HOST with the
 * function the entry point calls: SLRHIP_OK if the call would go ahead, else SLRHIP_ERR_INVALID_ARGUMENT with the reason in
 * slrhip_last_error_string.  The pointers are only compared, never followed.  No GPU is touched.                                  */
int slrhip_debug_reproject_check(const slrhip_reproject_desc* desc);

/* The argument checks of slrhip_render_motion (slr_amd/csrc/render_plan.h, motionRefusal), evaluated on the HOST with the function the
 * entry point calls, for a context that has a render state (have_render != 0) or none and whose scene has `num_instances` instances:
 * SLRHIP_OK if the call would go ahead, else the code it returns, with the reason in slrhip_last_error_string.  The descriptor's
 * pointers are only compared, never followed.  No GPU is touched.                                                                   */
int slrhip_debug_motion_check(int32_t have_render, uint32_t num_instances, const slrhip_motion_desc* desc, uint32_t spp_begin, uint32_t spp_count);

/* The same for slrhip_render_motion_vertices (motionVerticesRefusal), for a context created with slrhip_config::flags `config_flags`
 * whose tree came from builder `tree_builder` (SLRHIP_TREE_*, below): the outer descriptor's checks, those of its `frame`, and — where
 * previous_vertices is given — whether such a context keeps the vertex and index arrays.  No GPU is touched.                        */
int slrhip_debug_motion_vertices_check(int32_t have_render, uint32_t num_instances, uint32_t config_flags, uint32_t tree_builder,
                                       const slrhip_motion_vertices_desc* desc, uint32_t spp_begin, uint32_t spp_count);

/* The argument checks of slrhip_set_environment on a descriptor (slr_amd/csrc/render_plan.h, environmentRefusal), evaluated on the HOST
 * with the function the entry point calls: SLRHIP_OK if the descriptor would pass, else SLRHIP_ERR_INVALID_ARGUMENT with the reason in
 * slrhip_last_error_string.  The pointer is only compared, never followed.  No GPU is touched.                                      */
int slrhip_debug_environment_check(const slrhip_environment_desc* desc);

/* The environment of the context's scene, read back to HOST memory.  what: 0 the stored texels (width * height * 3 floats), 1 the
 * importance map (map_width * map_height), 2 the top PDF (map_height), 3 the top CDF (map_height + 1), 4 the row PDFs
 * (map_height * map_width), 5 the row CDFs (map_height * (map_width + 1)).  num_floats: room at host_dst, at least that many.
 * Synchronises.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene; SLRHIP_ERR_INVALID_ARGUMENT for a null argument, a scene without an
 * environment, an unknown `what`, too little room, and for what == 1 when the environment came from slrhip_upload_scene (the host
 * path keeps no map).                                                                                                              */
int slrhip_debug_environment(slrhip_ctx* ctx, uint32_t what, float* host_dst, size_t num_floats);

/* The argument checks of slrhip_set_instance_transforms (slr_amd/csrc/render_plan.h, instanceUpdateRefusal), evaluated on the HOST with
 * the function the entry point calls, for a context that holds a scene (have_scene != 0) of `num_instances` instances or none: SLRHIP_OK
 * if the call would go ahead, else the code it returns, with the reason in slrhip_last_error_string.  The pointer is only compared,
 * never followed.  No GPU is touched.                                                                                               */
int slrhip_debug_instance_update_check(int32_t have_scene, uint32_t num_instances, const void* device_src, uint32_t first_instance,
                                       uint32_t count);

/* The top level of the context's instanced scene, read back to HOST memory as 32-bit words.  what:
 *   0  the top-level QNodes, 32 words each: minx[4] miny[4] minz[4] maxx[4] maxy[4] maxz[4] (floats), child[4], pad[4]
 *   1  32 words: [0] levels of the top-level tree, [1] its nodes, [2] all nodes of the scene (the mesh trees follow the top level),
 *      [3] instances, [4] distinct meshes, [5] the widest level one workgroup of the refit takes (wider levels: a launch each),
 *      [8 .. 8 + levels] the first node of each level, then [1] again
 *   2  the DevInstance records, 36 words each: local_to_world[16], world_to_local[16] (floats), root node, first triangle,
 *      triangle count, mesh
 *   3  the instances' world boxes, 8 words each: lo[3], 0, hi[3], 0 (floats)
 *   4  every QNode of the scene (what 0's layout)
 *   5  the meshes' local boxes (what 3's layout)
 * num_words: room at host_dst, at least that many.  Synchronises.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene,
 * SLRHIP_ERR_UNSUPPORTED for a scene without instances, SLRHIP_ERR_INVALID_ARGUMENT for a null argument, an unknown `what` or too
 * little room.                                                                                                                      */
int slrhip_debug_top_level(slrhip_ctx* ctx, uint32_t what, void* host_dst, size_t num_words);

/* The checks of slrhip_rebuild_top_level (slr_amd/csrc/render_plan.h, topLevelRebuildRefusal), evaluated on the HOST with the function
 * the entry point calls, for a context that holds a scene (have_scene != 0) of `num_instances` instances or none: SLRHIP_OK if the call
 * would go ahead, else the code it returns, with the reason in slrhip_last_error_string.  No GPU is touched.                        */
int slrhip_debug_top_level_rebuild_check(int32_t have_scene, uint32_t num_instances);

/* The plan slrhip_rebuild_top_level's first call builds (slr_amd/csrc/top_level.cpp — the function it calls), on the HOST, from QNode
 * records (slrhip_debug_top_level's what 0 layout) whose first `top_nodes` are a top level: slots[i] = node * 4 + child of the leaf
 * slots depth-first from node 0 (child slots 0 .. 3 in order, an inner child's whole subtree before the next slot), refs[i] = the
 * child words of those slots ASCENDING (the canonical order of the primitives: instances 0 .. n - 1, then the packets), *count their
 * number.  capacity: room at slots and at refs (4 x top_nodes always suffice).  No GPU is touched.  SLRHIP_ERR_INVALID_ARGUMENT, with
 * *count = 0, for a null pointer, too little room, or nodes that are no top level (an inner child outside (its node, top_nodes), no
 * leaf, instance leaves that are not 0 .. n - 1 once each).                                                                         */
int slrhip_debug_top_level_plan(const void* nodes, uint32_t top_nodes, uint32_t* slots, uint32_t* refs, uint32_t capacity, uint32_t* count);

/* The WHOLE operation of slrhip_rebuild_top_level on a host copy of QNode records, in place, through the same header as the kernels
 * (slr_amd/csrc/pt_toplevel.h): plan, boxes (instance_boxes: slrhip_debug_top_level's what 3 layout, `num_instances` of them; a packet's
 * box is its slot's), scene box, keys, stable order, seat, refit.  keys_out[p] = the key of primitive p, order_out[i] = the primitive
 * slot i received; room for every primitive each, or NULL.  Works on slrhip_debug_host_tree's nodes and on a slrhip_debug_top_level
 * read-out; nodes at or behind top_nodes are not touched.  No GPU is touched.  SLRHIP_ERR_INVALID_ARGUMENT, with nothing changed, as
 * slrhip_debug_top_level_plan, and when the plan's instances are not `num_instances`.                                               */
int slrhip_debug_top_level_reseat(void* nodes, uint32_t top_nodes, const float* instance_boxes, uint32_t num_instances, uint64_t* keys_out,
                                  uint32_t* order_out);

/* slrhip_top_level_cost's value of QNode records on the HOST, with the function it calls.  No GPU is touched.                      */
int slrhip_debug_top_level_cost(const void* nodes, uint32_t top_nodes, double* cost);

/* The tables and the last call of slrhip_rebuild_top_level, read back to HOST memory as 32-bit words.  what:
 *   0  8 words: [0] primitives (0 before the first call after an upload: the tables are built by it), [1] SLRHIP_TOP_SEAT_GROUP,
 *      [2] the path of the last call (0 none yet, 1 one launch of one workgroup, 2 keys + device radix sort + seat), [3] its launches,
 *      the refit's included and the radix sort counted as one, [4] instances, [5] 1 if the tables are built, the rest 0
 *   1  the slot table, one word a primitive (node * 4 + child)         2  the canonical references, one word a primitive
 *   3  the keys of the last call by primitive, two words each (low, high)
 *   4  the order of the last call: word i = the primitive slot i received
 * num_words: room at host_dst, at least that many.  Synchronises; changes nothing.  The refusals of slrhip_rebuild_top_level;
 * SLRHIP_ERR_INVALID_ARGUMENT for a null argument, an unknown `what` or too little room.                                             */
int slrhip_debug_top_level_rebuild(slrhip_ctx* ctx, uint32_t what, void* host_dst, size_t num_words);

/* The argument checks of slrhip_set_vertices (slr_amd/csrc/render_plan.h, geometryUpdateRefusal), evaluated on the HOST with the
 * function the entry point calls, for a context that holds a scene (have_scene != 0) or none, created with SLRHIP_FLAG_DYNAMIC_GEOMETRY
 * (dynamic != 0) or without, whose tree came from builder `tree_builder` (SLRHIP_TREE_*, below) and whose scene has `num_instances`
 * instances and `num_vertices` vertices: SLRHIP_OK if the call would go ahead, else the code it returns, with the reason in
 * slrhip_last_error_string.  The pointer is only compared, never followed.  No GPU is touched.                                      */
int slrhip_debug_geometry_update_check(int32_t have_scene, int32_t dynamic, uint32_t tree_builder, uint32_t num_instances, uint32_t num_vertices,
                                       const void* device_src, uint32_t first_vertex, uint32_t count);

/* The same checks with one more input (geometryUpdateRefusal2, the function slrhip_set_vertices itself calls): instanced_kept != 0 for a
 * context created with SLRHIP_FLAG_DYNAMIC_INSTANCED as well, which keeps what the call needs of a scene with instances.  Then
 * `num_instances` != 0 and SLRHIP_TREE_INSTANCED are no refusal; every other answer, code and message is the check's above, and with
 * instanced_kept == 0 so are all of them.  No GPU is touched.                                                                         */
int slrhip_debug_geometry_update_check2(int32_t have_scene, int32_t dynamic, int32_t instanced_kept, uint32_t tree_builder, uint32_t num_instances,
                                        uint32_t num_vertices, const void* device_src, uint32_t first_vertex, uint32_t count);

/* What slrhip_set_vertices keeps and rewrites beyond the tree (slrhip_debug_tree reads that), read back to HOST memory as 32-bit
 * words.  what:
 *   0  the summary, 32 words: [0] levels of the tree, [1] nodes, [2] vertices, [3] triangles, [4] lights, [5] 1 if the shade tables are
 *      staged (the lights have a second copy there), [6] the widest level one workgroup of the refit takes (wider levels: a launch
 *      each), [7 .. 7 + levels] the first node of each level, then [1] again; after those: the float4 count of triUV (0 for a scene
 *      without textures), the number of alpha records, the launches of the last slrhip_set_vertices call (0: none yet)
 *   1  the kept vertices, 11 words each (slrhip_vertex)
 *   2  the LightTri records, 36 words each: p0[3] (floats), triangle, p1[3], material, p2[3], 1 / area, n0[3], gn.x, n1[3], gn.y,
 *      n2[3], gn.z, t0[3], 0, t1[3], 0, t2[3], 0
 *   3  the same records as staged in the shade tables; SLRHIP_ERR_UNSUPPORTED when the tables are not staged
 *   4  triUV, 8 words per triangle: u0 v0 u1 v1, u2 v2 0 0 (floats)
 *   5  the alpha records, 8 words each: u0 v0 u1 v1, u2 v2 (floats), the texture's index, 0
 *   6  the summary of a scene with instances, 48 words: [0] 1 if the scene has instances and is kept (else the words [1 .. 6], [9] and
 *      [16 ..] are 0), [1] levels of the top level, [2] merged levels of the mesh trees (the depth of the deepest mesh), [3] meshes,
 *      [4] instances, [5] nodes of the top level, [6] mesh nodes (the entries of the merged list), [7] LeafTri records (the boxes of
 *      what 8), [8] the launches of the last slrhip_set_vertices call, [9] the loose packets whose boxes the call refreshes for
 *      slrhip_rebuild_top_level (0 before that call has built its tables), [16 .. 16 + [2]] the first entry of each merged level,
 *      then [6] again
 *   7  the merged mesh-level list, one word per mesh node: the node indices of level 0 (the roots) of every mesh, then level 1, ..
 *   8  the leaf-box scratch as the last call left it, 8 words (floats) per LeafTri record: lo[3], 0, hi[3], 0 (before any call: not
 *      initialised)
 *   9  the root node of each mesh, one word each       10  slrhip_rebuild_top_level's packet boxes, 8 words (floats) per loose packet
 *      in its canonical order: lo[3], 0, hi[3], 0
 * For a scene with instances, what 0 describes the TOP level: [0] its levels, [7 .. 7 + levels] the first node of each, then the
 * number of top-level nodes ([1] stays the number of all nodes).
 * num_words: room at host_dst, at least that many.  Synchronises.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene,
 * SLRHIP_ERR_UNSUPPORTED for a context without SLRHIP_FLAG_DYNAMIC_GEOMETRY or a scene slrhip_set_vertices does not cover (spatial
 * splits; instances in a context without SLRHIP_FLAG_DYNAMIC_INSTANCED),
 * SLRHIP_ERR_INVALID_ARGUMENT for a null argument, an unknown `what` or too little room.                                          */
int slrhip_debug_geometry(slrhip_ctx* ctx, uint32_t what, void* host_dst, size_t num_words);

/* The checks of slrhip_set_materials (slr_amd/csrc/materials_prep.h, prepareMaterialsUpdate — the function the entry point calls),
 * evaluated on the HOST without a context: `desc` against the state a context of mode `mode` (SLRHIP_MODE_*) would keep after
 * uploading `uploaded` (NULL: a context without a scene), which keeps its geometry (geometry_kept != 0) or not; the environment is
 * `uploaded`'s.  SLRHIP_OK if the call would go ahead, else the code it returns, with the reason in slrhip_last_error_string.  With
 * facts != NULL and a scene, facts[3 m .. 3 m + 2] receive material m's triangle count, its "used by an instanced triangle" bit and its
 * alpha-map texture (0xFFFFFFFF: none) — num_facts: room at facts, at least 3 x uploaded->num_materials.  A descriptor the upload's own
 * material passes refuse returns their code and message.  No GPU is touched and no tree is built.                                    */
int slrhip_debug_materials_update_check(int32_t mode, const slrhip_scene_desc* uploaded, int32_t geometry_kept, const slrhip_materials_desc* desc,
                                        uint32_t* facts, size_t num_facts);

/* The tables slrhip_set_materials and slrhip_set_texture_texels replace, read back to HOST memory as 32-bit words.  what:
 *   0  the summary, 32 words: [0] lights, [1] 1 if the shade tables are staged (they fit the LDS limits), [2 .. 7] the ends of the
 *      blob's six segments in float4, [8] hasMicrofacet, [9] hasMulti, [10] materials, [11] spectra, [12] floats of the spectrum pool,
 *      [13] textures, [14] image texels, [15] the largest power of two <= lights, [16] the lights' total importance (float bits),
 *      [17] float4 of the blob; [24] the launches of the last slrhip_set_materials call (0: none since the upload), [25] 1 if that call
 *      rebuilt the light list; the rest 0
 *   1  the material records of the context's mode: DevMaterial, 20 words each (RGB), or DevMaterialS, 8 words each (spectral)
 *   2  the spectrum records, 8 words each          3  the spectrum pool          4  the lights' PMF, one float each
 *   5  the lights' CDF, lights + 1 floats           6  the shade-table blob (nothing when the tables are not staged)
 *   7  the image textures' texels, 3 floats each    8  the texture records, 16 words each      9  the materials' texture slots, 4 words each
 * The light records and ShadeTri::light have read-outs already (slrhip_debug_geometry what 2 and 3, slrhip_debug_tree what 4).
 * num_words: room at host_dst, at least that many.  Synchronises; changes nothing.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene,
 * SLRHIP_ERR_INVALID_ARGUMENT for a null argument, an unknown `what` or too little room.                                             */
int slrhip_debug_materials(slrhip_ctx* ctx, uint32_t what, void* host_dst, size_t num_words);

/* The tree builders (slr_amd/csrc/bvh.cpp, sbvh.cpp, bvh_device.hip), as the summary of the two read-outs below names them. */
#define SLRHIP_TREE_HOST_SAH 0u              /* binned SAH over object partitions, on the host                                    */
#define SLRHIP_TREE_HOST_SPATIAL_SPLITS 1u   /* the same with spatial splits (SLRHIP_FLAG_BVH_SPATIAL_SPLITS, SLRHIP_BVH=sbvh)   */
#define SLRHIP_TREE_DEVICE 2u                /* LBVH on the GPU (SLRHIP_FLAG_BVH_DEVICE_BUILD where the scene allows it)          */
#define SLRHIP_TREE_INSTANCED 3u             /* the two-level build of a scene with instances, on the host                        */

/* The tree of the context's scene — any scene, instanced or not — read back to HOST memory as 32-bit words.  what:
 *   0  the summary, 16 words: [0] the builder that ran (SLRHIP_TREE_*), [1] nodes, [2] levels as slrhip_counters::bvh_depth reports
 *      them, [3] leaf references (LeafTri records), [4] triangles, [5] 1 if the quantized nodes are in use, [6] instances,
 *      [7] nodes of the top level (instanced scenes; else 0), the rest 0
 *   1  the QNode records, 32 words each (slrhip_debug_top_level's layout)
 *   2  the QNodeQ records, 16 words each: origin[3], scale[3] (floats), qlo x, y, z, qhi x, y, z (one byte per child, child 0 lowest),
 *      child[4]; SLRHIP_ERR_UNSUPPORTED when the quantized nodes are not in use
 *   3  the LeafTri records, 12 words each: v0[3] (floats), triangle, e1[3], alpha record, e2[3], 0
 *   4  the ShadeTri records, 24 words each: n0[3] (floats), material, n1[3], light, n2[3], 1 / area, t0[3], gn.x, t1[3], gn.y, t2[3], gn.z
 *   5  the DevInstance records (slrhip_debug_top_level's what 2)        6  the instances' world boxes (its what 3)
 * num_words: room at host_dst, at least that many.  Synchronises; changes nothing, slrhip_debug_top_level included.
 * SLRHIP_ERR_NO_SCENE before slrhip_upload_scene, SLRHIP_ERR_INVALID_ARGUMENT for a null argument, an unknown `what` or too little room. */
int slrhip_debug_tree(slrhip_ctx* ctx, uint32_t what, void* host_dst, size_t num_words);

/* The tree the HOST builds for a scene descriptor in an RGB context with slrhip_config::flags `config_flags`, through the prepareScene
 * that slrhip_upload_scene calls (slr_amd/csrc/scene_prep.h).  `what` and the layouts are slrhip_debug_tree's.  what = 0 prepares the
 * scene and keeps the result for the calling thread; every other `what` copies from the result kept last (`desc` is not read then, and
 * may be NULL), so a tree is built once however many arrays are read.  No GPU is touched.  Returns what slrhip_upload_scene would for the
 * descriptor, with its message; SLRHIP_ERR_UNSUPPORTED, and a message that says so, for a descriptor whose tree prepareScene leaves to
 * the device build; SLRHIP_ERR_NO_SCENE for what != 0 before a successful what = 0.                                                     */
int slrhip_debug_host_tree(const slrhip_scene_desc* desc, uint32_t config_flags, uint32_t what, void* host_dst, size_t num_words);

/* The host quantizer (slr_amd/csrc/bvh.cpp, quantizeNodes — the function the upload calls) on the caller's nodes: `n` QNode records in,
 * `n` QNodeQ records out (the layouts above).  No GPU is touched.                                                                       */
int slrhip_debug_quantize_nodes(const void* nodes, uint32_t n, void* nodes_q);

/* The caller's samples through the fold: host_samples is [passes][height][width][components] float32 (HOST memory), passes 1 .. 64.
 * The shard's pixels are reordered with the context's own pixel list into a result window (pixel-major, as the render kernels
 * write it: a pixel's passes side by side; pixels outside the shard are ignored), the window is uploaded, and the fold the render would launch in the context's
 * current state — statistics on or off, clamp on or off — adds it to the sensor, the noise records and the clamp records, after
 * whatever the render has added so far.  Blocking (synchronises the device).  The render's counters and its error word are
 * untouched.  The call counts as the render having begun (slrhip_statistics_begin and slrhip_clamp_begin are refused after it),
 * and as the first such call it clears the sensor.  This is how NaN, infinite and huge samples reach the kernel at tiny sizes.
 * SLRHIP_ERR_INVALID_ARGUMENT for a null argument or a pass count out of range; SLRHIP_ERR_NO_SCENE before slrhip_render_begin.   */
int slrhip_debug_fold(slrhip_ctx* ctx, const float* host_samples, uint32_t passes);

#ifdef __cplusplus
}
#endif
#endif /* SLRHIP_DEBUG_H */
