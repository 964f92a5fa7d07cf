"""ctypes binding of libslrhip.so (include/slrhip.h).  There is no fallback: if the HIP
library is missing or no GPU is present, creating a Context raises."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
LIB_PATH = os.path.join(CSRC, "libslrhip.so")

EXPORTS = ["slrhip_create", "slrhip_destroy", "slrhip_upload_scene", "slrhip_render_begin", "slrhip_render",
           "slrhip_resolve_framebuffer", "slrhip_reduce_framebuffer", "slrhip_read_framebuffer", "slrhip_synchronize", "slrhip_get_counters",
           "slrhip_components", "slrhip_get_profile", "slrhip_trace_rays", "slrhip_intersect_rays", "slrhip_test_visibility",
           "slrhip_query_status", "slrhip_render_features", "slrhip_resolve_features", "slrhip_read_features", "slrhip_camera_rays", "slrhip_features_status",
           "slrhip_statistics_begin", "slrhip_resolve_statistics", "slrhip_read_statistics", "slrhip_statistics_summary", "slrhip_render_until", "slrhip_sample_luminance",
           "slrhip_render_adaptive", "slrhip_resolve_framebuffer_mean", "slrhip_read_framebuffer_mean", "slrhip_adaptive_active", "slrhip_debug_adaptive_blocks",
           "slrhip_denoise", "slrhip_denoise_scratch_bytes", "slrhip_tonemap", "slrhip_tonemap_bytes",
           "slrhip_render_albedo", "slrhip_resolve_albedo", "slrhip_read_albedo", "slrhip_modulate", "slrhip_debug_modulate_check",
           "slrhip_clamp_begin", "slrhip_resolve_clamp", "slrhip_read_clamp", "slrhip_clamp_summary", "slrhip_clamp_sample", "slrhip_debug_fold",
           "slrhip_set_environment", "slrhip_env_importance", "slrhip_env_texels_to_uvs", "slrhip_debug_environment_check", "slrhip_debug_environment",
           "slrhip_set_instance_transforms", "slrhip_instances_status", "slrhip_instance_world_box", "slrhip_set_camera",
           "slrhip_debug_instance_update_check", "slrhip_debug_top_level",
           "slrhip_rebuild_top_level", "slrhip_top_level_cost", "slrhip_top_level_key", "slrhip_debug_top_level_rebuild_check",
           "slrhip_debug_top_level_plan", "slrhip_debug_top_level_reseat", "slrhip_debug_top_level_cost", "slrhip_debug_top_level_rebuild",
           "slrhip_render_motion", "slrhip_resolve_motion", "slrhip_read_motion", "slrhip_motion_camera", "slrhip_motion_sample", "slrhip_reproject",
           "slrhip_debug_motion_check", "slrhip_debug_reproject_check",
           "slrhip_render_motion_vertices", "slrhip_motion_sample_vertices", "slrhip_debug_motion_vertices_check",
           "slrhip_debug_tree", "slrhip_debug_host_tree", "slrhip_debug_quantize_nodes",
           "slrhip_set_vertices", "slrhip_geometry_status", "slrhip_debug_geometry_update_check", "slrhip_debug_geometry",
           "slrhip_debug_geometry_update_check2",
           "slrhip_set_materials", "slrhip_set_texture_texels", "slrhip_debug_materials_update_check", "slrhip_debug_materials",
           "slrhip_bsdf_queries", "slrhip_debug_work_distribution", "slrhip_debug_render_plan", "slrhip_debug_primary_plan", "slrhip_debug_primary_samples", "slrhip_debug_shadow_skipped", "slrhip_debug_dead_light_samples", "slrhip_debug_primary_entries", "slrhip_debug_primary_stream_entries", "slrhip_debug_primary_stream_plan", "slrhip_debug_primary_kernel_plan", "slrhip_debug_primary_kernel", "slrhip_debug_shade_plan", "slrhip_debug_shade_kernel", "slrhip_debug_primary_pass", "slrhip_debug_camera_draws", "slrhip_sample_seed", "slrhip_upsample", "slrhip_resolve_upsampled", "slrhip_spectrum_to_rgb", "slrhip_tonemap_bgr8", "slrhip_save_bmp",
           "slrhip_last_error_string", "slrhip_version"]


class HipLibraryMissing(RuntimeError):
    pass


class SlrHipError(RuntimeError):
    pass


_lib = None


def build_library():
    subprocess.check_call(["make", "-s", "-C", CSRC])


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SLRHIP_LIBRARY", LIB_PATH)      # development: an alternate build of the same ABI (tools/build_variant.sh)
    if not os.path.exists(path):
        raise HipLibraryMissing("%s not built: run `make -C slr_amd/csrc` (or __graft_entry__.build())" % path)
    lib = C.CDLL(path)
    lib.slrhip_create.argtypes = [C.POINTER(abi.Config), C.POINTER(C.c_void_p)]
    lib.slrhip_destroy.argtypes = [C.c_void_p]
    lib.slrhip_upload_scene.argtypes = [C.c_void_p, C.POINTER(abi.SceneDesc)]
    lib.slrhip_render_begin.argtypes = [C.c_void_p, C.POINTER(abi.RenderSettings), abi.Shard]
    lib.slrhip_render.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    lib.slrhip_resolve_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.slrhip_reduce_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.slrhip_read_framebuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    lib.slrhip_synchronize.argtypes = [C.c_void_p]
    lib.slrhip_get_counters.argtypes = [C.c_void_p, C.POINTER(abi.Counters)]
    lib.slrhip_components.argtypes = [C.c_void_p]
    lib.slrhip_get_profile.argtypes = [C.c_void_p, C.POINTER(abi.Profile)]
    lib.slrhip_trace_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.slrhip_intersect_rays.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.slrhip_test_visibility.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.slrhip_query_status.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    # (an alternate build from before the feature buffers lacks these five: calling one there is an AttributeError)
    for name, argtypes in (("slrhip_render_features", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
                           ("slrhip_resolve_features", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
                           ("slrhip_read_features", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
                           ("slrhip_camera_rays", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p]),
                           ("slrhip_features_status", [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the noise statistics lacks these six)
    for name, argtypes in (("slrhip_statistics_begin", [C.c_void_p]),
                           ("slrhip_resolve_statistics", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
                           ("slrhip_read_statistics", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
                           ("slrhip_statistics_summary", [C.c_void_p, C.POINTER(abi.StatisticsSummary), C.c_void_p]),
                           ("slrhip_render_until", [C.c_void_p, C.c_uint32, C.POINTER(abi.NoiseTarget), C.POINTER(C.c_uint32),
                                                    C.POINTER(abi.StatisticsSummary), C.c_void_p]),
                           ("slrhip_sample_luminance", [C.c_int32, C.c_void_p])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before adaptive sampling lacks these five)
    for name, argtypes in (("slrhip_render_adaptive", [C.c_void_p, C.c_uint32, C.POINTER(abi.AdaptiveTarget), C.POINTER(C.c_uint32),
                                                       C.POINTER(C.c_uint64), C.c_void_p]),
                           ("slrhip_resolve_framebuffer_mean", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
                           ("slrhip_read_framebuffer_mean", [C.c_void_p, C.c_void_p, C.c_size_t]),
                           ("slrhip_adaptive_active", [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
                           ("slrhip_debug_adaptive_blocks", [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the denoiser lacks these two)
    if path == LIB_PATH or hasattr(lib, "slrhip_denoise"):
        lib.slrhip_denoise.argtypes = [C.c_void_p, C.POINTER(abi.DenoiseDesc), C.c_void_p]
        lib.slrhip_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.slrhip_denoise_scratch_bytes.restype = C.c_size_t
    # (and one from before the device image export lacks these two)
    if path == LIB_PATH or hasattr(lib, "slrhip_tonemap"):
        lib.slrhip_tonemap.argtypes = [C.c_void_p, C.POINTER(abi.TonemapDesc), C.c_void_p]
        lib.slrhip_tonemap_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.slrhip_tonemap_bytes.restype = C.c_size_t
    # (and one from before the albedo buffer lacks these five)
    for name, argtypes in (("slrhip_render_albedo", [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
                           ("slrhip_resolve_albedo", [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p]),
                           ("slrhip_read_albedo", [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32)]),
                           ("slrhip_modulate", [C.c_void_p, C.POINTER(abi.ModulateDesc), C.c_void_p]),
                           ("slrhip_debug_modulate_check", [C.POINTER(abi.ModulateDesc)])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the sample clamp lacks these six)
    for name, argtypes in (("slrhip_clamp_begin", [C.c_void_p, C.POINTER(abi.ClampDesc)]),
                           ("slrhip_resolve_clamp", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p]),
                           ("slrhip_read_clamp", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
                           ("slrhip_clamp_summary", [C.c_void_p, C.POINTER(abi.ClampSummary), C.c_void_p]),
                           ("slrhip_clamp_sample", [C.c_int32, C.c_void_p, C.c_float, C.c_uint32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
                           ("slrhip_debug_fold", [C.c_void_p, C.c_void_p, C.c_uint32])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the environment from device memory lacks these five)
    for name, argtypes in (("slrhip_set_environment", [C.c_void_p, C.POINTER(abi.EnvironmentDesc), C.c_void_p]),
                           ("slrhip_env_importance", [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
                           ("slrhip_env_texels_to_uvs", [C.c_void_p, C.c_size_t, C.c_void_p]),
                           ("slrhip_debug_environment_check", [C.POINTER(abi.EnvironmentDesc)]),
                           ("slrhip_debug_environment", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before instances and the camera could move lacks these six)
    for name, argtypes in (("slrhip_set_instance_transforms", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
                           ("slrhip_instances_status", [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
                           ("slrhip_instance_world_box", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                           ("slrhip_set_camera", [C.c_void_p, C.POINTER(abi.Camera)]),
                           ("slrhip_debug_instance_update_check", [C.c_int32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]),
                           ("slrhip_debug_top_level", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the top level could be re-seated lacks these eight)
    for name, argtypes in (("slrhip_rebuild_top_level", [C.c_void_p, C.c_void_p]),
                           ("slrhip_top_level_cost", [C.c_void_p, C.POINTER(C.c_double), C.c_void_p]),
                           ("slrhip_top_level_key", [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
                           ("slrhip_debug_top_level_rebuild_check", [C.c_int32, C.c_uint32]),
                           ("slrhip_debug_top_level_plan", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
                           ("slrhip_debug_top_level_reseat", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
                           ("slrhip_debug_top_level_cost", [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]),
                           ("slrhip_debug_top_level_rebuild", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before motion vectors and temporal reprojection lacks these eight)
    for name, argtypes in (("slrhip_render_motion", [C.c_void_p, C.POINTER(abi.MotionDesc), C.c_uint32, C.c_uint32, C.c_void_p]),
                           ("slrhip_resolve_motion", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
                           ("slrhip_read_motion", [C.c_void_p, C.c_void_p, C.c_size_t]),
                           ("slrhip_motion_camera", [C.POINTER(abi.Camera), C.c_void_p]),
                           ("slrhip_motion_sample", [C.POINTER(abi.Camera), C.POINTER(abi.Camera), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                     C.c_void_p, C.c_void_p]),
                           ("slrhip_reproject", [C.c_void_p, C.POINTER(abi.ReprojectDesc), C.c_void_p]),
                           ("slrhip_debug_motion_check", [C.c_int32, C.c_uint32, C.POINTER(abi.MotionDesc), C.c_uint32, C.c_uint32]),
                           ("slrhip_debug_reproject_check", [C.POINTER(abi.ReprojectDesc)])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before motion vectors of moved vertices lacks these three)
    for name, argtypes in (("slrhip_render_motion_vertices", [C.c_void_p, C.POINTER(abi.MotionVerticesDesc), C.c_uint32, C.c_uint32, C.c_void_p]),
                           ("slrhip_motion_sample_vertices", [C.POINTER(abi.Camera), C.POINTER(abi.Camera), C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                                              C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p]),
                           ("slrhip_debug_motion_vertices_check", [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(abi.MotionVerticesDesc),
                                                                   C.c_uint32, C.c_uint32])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the tree read-outs lacks these three)
    for name, argtypes in (("slrhip_debug_tree", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
                           ("slrhip_debug_host_tree", [C.POINTER(abi.SceneDesc), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
                           ("slrhip_debug_quantize_nodes", [C.c_void_p, C.c_uint32, C.c_void_p])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before vertices could move lacks these four)
    for name, argtypes in (("slrhip_set_vertices", [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
                           ("slrhip_geometry_status", [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]),
                           ("slrhip_debug_geometry_update_check", [C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                                                   C.c_uint32]),
                           ("slrhip_debug_geometry", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    # (and one from before the vertices of instanced scenes could move lacks this one)
    if path == LIB_PATH or hasattr(lib, "slrhip_debug_geometry_update_check2"):
        lib.slrhip_debug_geometry_update_check2.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32]
    # (and one from before materials could change without an upload lacks these four)
    for name, argtypes in (("slrhip_set_materials", [C.c_void_p, C.POINTER(abi.MaterialsDesc), C.c_void_p]),
                           ("slrhip_set_texture_texels", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
                           ("slrhip_debug_materials_update_check", [C.c_int32, C.POINTER(abi.SceneDesc), C.c_int32, C.POINTER(abi.MaterialsDesc),
                                                                    C.c_void_p, C.c_size_t]),
                           ("slrhip_debug_materials", [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t])):
        if path == LIB_PATH or hasattr(lib, name):
            getattr(lib, name).argtypes = argtypes
    if path == LIB_PATH or hasattr(lib, "slrhip_sample_luminance"):
        lib.slrhip_sample_luminance.restype = C.c_float
    # (and one from before the primary pass lacks these two)
    if path == LIB_PATH or hasattr(lib, "slrhip_debug_primary_plan"):
        lib.slrhip_debug_primary_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p]
        lib.slrhip_debug_primary_samples.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    # (and one from before the pass handed its streams to the fused start lacks these four)
    if path == LIB_PATH or hasattr(lib, "slrhip_debug_camera_draws"):
        lib.slrhip_debug_primary_entries.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.slrhip_debug_primary_stream_entries.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.slrhip_debug_primary_stream_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_uint64)]
        lib.slrhip_debug_camera_draws.argtypes = [C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    # (and one from before the direct kernel of the primary pass lacks these three)
    if path == LIB_PATH or hasattr(lib, "slrhip_debug_primary_pass"):
        lib.slrhip_debug_primary_kernel_plan.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.POINTER(C.c_uint32)]
        lib.slrhip_debug_primary_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
        lib.slrhip_debug_primary_pass.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    # (and one from before the table of shade kernels lacks these two)
    if path == LIB_PATH or hasattr(lib, "slrhip_debug_shade_kernel"):
        lib.slrhip_debug_shade_plan.argtypes = [C.c_uint32] * 7 + [C.POINTER(C.c_uint32)]
        lib.slrhip_debug_shade_kernel.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    # (and one from before dead light samples went untraced lacks these two)
    if path == LIB_PATH or hasattr(lib, "slrhip_debug_shadow_skipped"):
        lib.slrhip_debug_shadow_skipped.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        lib.slrhip_debug_dead_light_samples.argtypes = [C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.slrhip_bsdf_queries.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_float, C.c_float, C.c_void_p]
    lib.slrhip_sample_seed.argtypes = [C.c_int32, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.slrhip_sample_seed.restype = C.c_int32
    lib.slrhip_upsample.argtypes = [C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p]
    lib.slrhip_resolve_upsampled.argtypes = [C.POINTER(abi.UpsamplingTables), C.c_float, C.c_float, C.POINTER(C.c_uint32), C.c_void_p]
    lib.slrhip_spectrum_to_rgb.argtypes = [C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.slrhip_tonemap_bgr8.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_size_t]
    lib.slrhip_save_bmp.argtypes = [C.c_char_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.slrhip_last_error_string.restype = C.c_char_p
    _lib = lib
    return lib


_hip = None


def _hip_runtime():
    """The HIP runtime libslrhip.so is bound to: the first copy loaded under its soname (torch's own copy, if torch was imported
    before the library; else the system's)."""
    global _hip
    if _hip is None:
        load_library()
        h = C.CDLL("libamdhip64.so.7")
        h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        h.hipFree.argtypes = [C.c_void_p]
        _hip = h
    return _hip


def _hip_check(rc, what):
    if rc != 0:
        raise SlrHipError("%s failed (%d)" % (what, rc))


def _check(lib, rc, what):
    if rc != 0:
        raise SlrHipError("%s failed (%d): %s" % (what, rc, lib.slrhip_last_error_string().decode()))


class DeviceBlocks:
    """hipMalloc'ed blocks for staging host arrays through a call on device pointers, from the HIP runtime the library is bound to:
    `with DeviceBlocks() as dev:` frees every block on the way out.  Addresses are plain integers."""

    def __init__(self):
        self.hip, self.blocks = _hip_runtime(), []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.blocks:
            self.hip.hipFree(p)
        self.blocks = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        _hip_check(self.hip.hipMalloc(C.byref(p), max(nbytes, 16)), "hipMalloc")
        self.blocks.append(p.value)
        return p.value

    def put(self, array):
        """A block holding a copy of `array`."""
        a = np.ascontiguousarray(array)
        p = self.alloc(a.nbytes)
        _hip_check(self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1), "hipMemcpy")
        return p

    def get(self, ptr, shape, dtype=np.float32):
        """The device memory at `ptr` (anywhere inside a block) as a new numpy array."""
        out = np.empty(shape, dtype)
        _hip_check(self.hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2), "hipMemcpy")
        return out


class Context:
    """One rendering context on one GPU (slrhip_ctx)."""

    def __init__(self, device=0, mode=abi.MODE_RGB, stripes=0, flags=0):
        self.lib = load_library()
        self.device = device
        self.handle = C.c_void_p()
        cfg = abi.Config(device, mode, stripes, flags)
        _check(self.lib, self.lib.slrhip_create(C.byref(cfg), C.byref(self.handle)), "slrhip_create")
        self.components = self.lib.slrhip_components(self.handle)
        self.settings = None
        self.shard = (0, 1)
        self._env_size = None                     # (width, height, map width, map height) of the scene's environment, for debug_environment

    def close(self):
        if getattr(self, "handle", None):
            self.lib.slrhip_destroy(self.handle)
            self.handle = None

    def __del__(self):
        self.close()

    def upload_scene(self, scene, upsampling=False):
        """slrhip_upload_scene.  upsampling=True: a spectral context also gets the Meng-15 tables of a scene that does not need
        them yet, so that set_environment can give it an environment later."""
        desc = scene.desc(self.mode, upsampling) if upsampling else scene.desc(self.mode)
        self._env_size = None
        _check(self.lib, self.lib.slrhip_upload_scene(self.handle, C.byref(desc)), "slrhip_upload_scene")
        if desc.env:
            e = desc.env.contents
            self._env_size = (e.width, e.height, e.map_width, e.map_height)

    # ---- the environment light from device memory (slrhip_set_environment) ----
    def set_environment_into(self, device_ptr, width, height, scale, flags=0, stream=None):
        """slrhip_set_environment over a DEVICE pointer (an integer address): [height][width][3] float32 texels, 16-byte aligned,
        copied by the library in order on `stream`; returns at once."""
        d = abi.EnvironmentDesc(width, height, device_ptr, scale, flags, (C.c_uint32 * 2)(0, 0))
        _check(self.lib, self.lib.slrhip_set_environment(self.handle, C.byref(d), self._stream_handle(stream)), "slrhip_set_environment")
        self._env_size = (width, height, width // 4, height // 4)

    def set_environment(self, texels, scale, rgb=False, store_half=False, stream=None):
        """Replaces (or adds) the environment sphere of the uploaded scene (slrhip_set_environment): texels [H, W, 3] float32, what
        slrhip_envmap::texels holds for the context's mode, or with rgb=True linear (r, g, b) that a spectral context converts to
        (u, v, s); store_half=True rounds them to binary16 first.  The importance map and the sampling tables are built on the
        device.  A torch CUDA tensor (contiguous) is passed without a copy and read in order on `stream` (default:
        torch.cuda.current_stream()); a numpy array is copied to the device first, and that call synchronises."""
        flags = (abi.ENV_TEXELS_RGB if rgb else 0) | (abi.ENV_STORE_HALF if store_half else 0)
        if isinstance(texels, np.ndarray):
            a = np.ascontiguousarray(texels, np.float32)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("texels: a [height, width, 3] array expected")
            with DeviceBlocks() as dev:
                self.set_environment_into(dev.put(a), a.shape[1], a.shape[0], scale, flags, stream)
                self.synchronize()                     # the staging block is freed on the way out
            return
        import torch
        if not (isinstance(texels, torch.Tensor) and texels.is_cuda and texels.dtype == torch.float32 and texels.dim() == 3
                and texels.shape[2] == 3 and texels.is_contiguous()):
            raise ValueError("texels: a contiguous [height, width, 3] float32 CUDA tensor (or a numpy array) expected")
        if texels.device.index != self.device:
            raise SlrHipError("set_environment: the tensor is on device %r, the context on device %d" % (texels.device.index, self.device))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.set_environment_into(texels.data_ptr(), texels.shape[1], texels.shape[0], scale, flags, s)

    def debug_environment(self, what):
        """Diagnostic (slrhip_debug_environment): one array of the scene's environment as a numpy array.  what: 0 the stored texels
        [H, W, 3], 1 the importance map [mh, mw] (set_environment's only), 2 the top PDF [mh], 3 the top CDF [mh + 1], 4 the row
        PDFs [mh, mw], 5 the row CDFs [mh, mw + 1].  Synchronises."""
        if self._env_size is None:
            raise SlrHipError("debug_environment: the scene has no environment")
        w, h, mw, mh = self._env_size
        shape = {0: (h, w, 3), 1: (mh, mw), 2: (mh,), 3: (mh + 1,), 4: (mh, mw), 5: (mh, mw + 1)}.get(what)
        if shape is None:
            raise ValueError("what: 0 .. 5 expected")
        out = np.empty(shape, np.float32)
        _check(self.lib, self.lib.slrhip_debug_environment(self.handle, what, out.ctypes.data, out.size), "slrhip_debug_environment")
        return out

    # ---- moving instances and the camera without a scene upload (slrhip_set_instance_transforms / slrhip_set_camera) ----
    def set_instance_transforms_into(self, device_ptr, first, count, stream=None):
        """slrhip_set_instance_transforms over a DEVICE pointer (an integer address): `count` 128-byte records, 16-byte aligned, read in
        order on `stream`; returns at once."""
        _check(self.lib, self.lib.slrhip_set_instance_transforms(self.handle, device_ptr, first, count, self._stream_handle(stream)),
               "slrhip_set_instance_transforms")

    def set_instance_transforms(self, transforms, first=0, stream=None):
        """New matrices for the instances [first, first + n) of the uploaded scene (slrhip_set_instance_transforms): transforms is
        [n, 32] float32 — per row local_to_world then world_to_local, column-major — or n records of abi.instance_transform_dtype or
        abi.instance_dtype (its two matrices are taken).  The top-level tree is refitted on the device; nothing accumulated is reset.
        A torch CUDA tensor (contiguous [n, 32] float32) is passed without a copy and read in order on `stream` (default:
        torch.cuda.current_stream()); a numpy array is copied to the device first, and that call synchronises.  A record that is
        not finite or not affine leaves its instance where it was: see instances_status."""
        if isinstance(transforms, np.ndarray):
            a = transforms
            if a.dtype == abi.instance_dtype:
                a = np.concatenate([a["local_to_world"], a["world_to_local"]], axis=1)
            elif a.dtype == abi.instance_transform_dtype:
                a = np.ascontiguousarray(a).view(np.float32)
            a = np.ascontiguousarray(a, np.float32).reshape(-1, 32)
            with DeviceBlocks() as dev:
                self.set_instance_transforms_into(dev.put(a) if len(a) else None, first, len(a), stream)
                self.synchronize()                     # the staging block is freed on the way out
            return
        import torch
        if not (isinstance(transforms, torch.Tensor) and transforms.is_cuda and transforms.dtype == torch.float32 and transforms.dim() == 2
                and transforms.shape[1] == 32 and transforms.is_contiguous()):
            raise ValueError("transforms: a contiguous [n, 32] float32 CUDA tensor (or a numpy array) expected")
        if transforms.device.index != self.device:
            raise SlrHipError("set_instance_transforms: the tensor is on device %r, the context on device %d" % (transforms.device.index, self.device))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.set_instance_transforms_into(transforms.data_ptr(), first, transforms.shape[0], s)

    def instances_status(self, stream=None):
        """The abi.INSTANCE_* bits of the set_instance_transforms calls since the last read, then cleared (slrhip_instances_status);
        waits for `stream` (a torch stream, a raw handle; default: the null stream)."""
        bits = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_instances_status(self.handle, C.byref(bits), self._stream_handle(stream)), "slrhip_instances_status")
        return bits.value

    # ---- moving vertices without a scene upload (slrhip_set_vertices; contexts created with abi.FLAG_DYNAMIC_GEOMETRY) ----
    def set_vertices_into(self, device_ptr, first, count, stream=None):
        """slrhip_set_vertices over a DEVICE pointer (an integer address): `count` 44-byte slrhip_vertex records, 4-byte aligned, read in
        order on `stream`; returns at once."""
        _check(self.lib, self.lib.slrhip_set_vertices(self.handle, device_ptr, first, count, self._stream_handle(stream)), "slrhip_set_vertices")

    def set_vertices(self, vertices, first=0, count=None, stream=None):
        """New records for the vertices [first, first + n) of the uploaded flat scene (slrhip_set_vertices): position, normal, tangent
        and texcoord all take effect, and every record and box that depends on them is rebuilt on the device; the tree keeps its shape
        and nothing accumulated is reset.  A scene with instances is covered in a context created with abi.FLAG_DYNAMIC_INSTANCED as
        well: the mesh trees, the meshes' and instances' boxes and the top level are refitted too.  `vertices`: a DEVICE address (an integer; `count` records), n records of abi.vertex_dtype, or a
        contiguous [n, 11] float32 numpy array or torch CUDA tensor.  A tensor is passed without a copy and read in order on `stream`
        (default: torch.cuda.current_stream()); a numpy array is copied to the device first, and that call synchronises.  A record with a
        non-finite float leaves its vertex as it was: see geometry_status."""
        if vertices is None or isinstance(vertices, int):
            return self.set_vertices_into(vertices, first, 0 if count is None else count, stream)
        if isinstance(vertices, np.ndarray):
            a = np.ascontiguousarray(vertices)
            a = a.view(np.float32) if a.dtype == abi.vertex_dtype else np.ascontiguousarray(a, np.float32)
            a = a.reshape(-1, 11)
            with DeviceBlocks() as dev:
                self.set_vertices_into(dev.put(a) if len(a) else None, first, len(a), stream)
                self.synchronize()                     # the staging block is freed on the way out
            return
        import torch
        if not (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2
                and vertices.shape[1] == 11 and vertices.is_contiguous()):
            raise ValueError("vertices: a contiguous [n, 11] float32 CUDA tensor (or a numpy array, or a device address) expected")
        if vertices.device.index != self.device:
            raise SlrHipError("set_vertices: the tensor is on device %r, the context on device %d" % (vertices.device.index, self.device))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.set_vertices_into(vertices.data_ptr(), first, vertices.shape[0], s)

    def geometry_status(self, stream=None):
        """The abi.GEOMETRY_* bits of the set_vertices calls since the last read, then cleared (slrhip_geometry_status); waits for
        `stream` (a torch stream, a raw handle; default: the null stream)."""
        bits = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_geometry_status(self.handle, C.byref(bits), self._stream_handle(stream)), "slrhip_geometry_status")
        return bits.value

    def debug_geometry(self):
        """Diagnostic (slrhip_debug_geometry): what set_vertices keeps and rewrites beyond the tree, as a dict — levels (first node of
        each level, then the number of nodes), num_nodes, group_nodes (the widest level the refit takes in one workgroup), staged
        (the shade tables hold a second copy of the lights), launches (of the last set_vertices call), vertices (abi.vertex_dtype),
        light_tris [n, 36] uint32, light_tris_staged (the same, or None), tri_uv [2 t, 4] float32, alpha [2 a, 4] uint32,
        leaf_boxes [leaf records, 2, 4] float32 (the scratch as the last call left it).  For a scene with instances (instanced: True)
        `levels` is the top level's table, and there are also: top_levels, mesh_depth (merged levels of the mesh trees), num_meshes,
        num_instances, top_nodes, mesh_levels (first entry of each merged level, then the number of mesh nodes), mesh_level_nodes (the
        merged list: one node index per mesh node), mesh_roots, packet_boxes [p, 2, 4] float32 (slrhip_rebuild_top_level's, once its
        tables exist).  Synchronises."""
        def read(what, words, dtype=np.uint32):
            out = np.zeros(words, dtype)
            _check(self.lib, self.lib.slrhip_debug_geometry(self.handle, what, out.ctypes.data, out.nbytes // 4), "slrhip_debug_geometry")
            return out
        head = read(0, 32)
        levels, nodes, nv, nt, nl, staged, group = (int(v) for v in head[:7])
        uv4, alpha, launches = (int(v) for v in head[8 + levels:11 + levels])
        out = dict(levels=head[7:8 + levels].copy(), num_nodes=nodes, num_triangles=nt, group_nodes=group, staged=bool(staged), launches=launches,
                   vertices=read(1, nv, abi.vertex_dtype), light_tris=read(2, nl * 36).reshape(nl, 36),
                   light_tris_staged=read(3, nl * 36).reshape(nl, 36) if staged else None,
                   tri_uv=read(4, uv4 * 4, np.float32).reshape(uv4, 4), alpha=read(5, alpha * 8).reshape(alpha * 2, 4))
        more = read(6, 48)
        instanced, top_levels, depth, meshes, instances, top_nodes, mesh_nodes, leaves, _, packets = (int(v) for v in more[:10])
        out.update(instanced=bool(instanced), leaf_boxes=read(8, leaves * 8, np.float32).reshape(leaves, 2, 4))
        if instanced:
            out.update(top_levels=top_levels, mesh_depth=depth, num_meshes=meshes, num_instances=instances, top_nodes=top_nodes,
                       mesh_levels=more[16:17 + depth].copy(), mesh_level_nodes=read(7, mesh_nodes), mesh_roots=read(9, meshes),
                       packet_boxes=read(10, packets * 8, np.float32).reshape(packets, 2, 4))
        return out

    # ---- changing materials, spectra, textures and lights without a scene upload (slrhip_set_materials / slrhip_set_texture_texels) ----
    def set_materials(self, scene, stream=None):
        """Replaces the material, spectrum, spectrum-data and texture tables of the uploaded scene with those of `scene` (an abi.Scene; only
        its tables are used): slrhip_set_materials.  The tree, the kept geometry and everything accumulated stay; when the set of
        emitting materials changes the light list is rebuilt on the device, which needs a context that keeps its geometry
        (abi.FLAG_DYNAMIC_GEOMETRY).  Synchronises the device first."""
        d = scene.materials_desc()
        _check(self.lib, self.lib.slrhip_set_materials(self.handle, C.byref(d), self._stream_handle(stream)), "slrhip_set_materials")

    def set_texture_texels_into(self, texture, device_ptr, flags=0, stream=None):
        """slrhip_set_texture_texels over a DEVICE pointer (an integer address): [height][width][3] float32 of image texture `texture`,
        4-byte aligned, read in order on `stream`; returns at once."""
        _check(self.lib, self.lib.slrhip_set_texture_texels(self.handle, texture, device_ptr, flags, self._stream_handle(stream)),
               "slrhip_set_texture_texels")

    def set_texture_texels(self, texture, texels, store_half=False, stream=None):
        """New texels for image texture `texture` of the uploaded scene, in place (slrhip_set_texture_texels): [height, width, 3]
        float32 in the stored form of the context's mode — (r, g, b), or (u, v, s) in spectral mode; store_half=True rounds them to
        binary16 first.  A torch CUDA tensor (contiguous) is passed without a copy and read in order on `stream` (default:
        torch.cuda.current_stream()); a numpy array is copied to the device first, and that call synchronises.  The size must be the
        uploaded image's: the library reads width x height texels."""
        flags = abi.TEXELS_STORE_HALF if store_half else 0
        if isinstance(texels, np.ndarray):
            a = np.ascontiguousarray(texels, np.float32)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("texels: a [height, width, 3] array expected")
            with DeviceBlocks() as dev:
                self.set_texture_texels_into(texture, dev.put(a), flags, stream)
                self.synchronize()                     # the staging block is freed on the way out
            return
        import torch
        if not (isinstance(texels, torch.Tensor) and texels.is_cuda and texels.dtype == torch.float32 and texels.dim() == 3
                and texels.shape[2] == 3 and texels.is_contiguous()):
            raise ValueError("texels: a contiguous [height, width, 3] float32 CUDA tensor (or a numpy array) expected")
        if texels.device.index != self.device:
            raise SlrHipError("set_texture_texels: the tensor is on device %r, the context on device %d" % (texels.device.index, self.device))
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        self.set_texture_texels_into(texture, texels.data_ptr(), flags, s)

    def debug_materials(self):
        """Diagnostic (slrhip_debug_materials): the tables set_materials and set_texture_texels replace, as a dict — lights, staged (the
        shade tables fit the LDS limits), table_end [6], has_microfacet, has_multi, light_pow2, importance, launches (of the last
        set_materials call), rebuilt (that call rebuilt the light list), materials [m, 20 or 8] uint32, spectra [s, 8] uint32,
        pool float32, pmf, cdf, blob [b, 4] uint32, texels [t, 3] float32, textures [n, 16] uint32, mat_tex [m, 4] int32.  Synchronises."""
        def read(what, words, dtype=np.uint32):
            out = np.zeros(words, dtype)
            _check(self.lib, self.lib.slrhip_debug_materials(self.handle, what, out.ctypes.data, out.nbytes // 4), "slrhip_debug_materials")
            return out
        head = read(0, 32)
        lights, staged = int(head[0]), bool(head[1])
        nm, ns, pool, nt, texels, blob = int(head[10]), int(head[11]), int(head[12]), int(head[13]), int(head[14]), int(head[17])
        per = 8 if self.mode == abi.MODE_SPECTRAL else 20
        return dict(lights=lights, staged=staged, table_end=head[2:8].copy(), has_microfacet=bool(head[8]), has_multi=bool(head[9]),
                    light_pow2=int(head[15]), importance=head[16:17].view(np.float32)[0], launches=int(head[24]), rebuilt=bool(head[25]),
                    materials=read(1, nm * per).reshape(nm, per), spectra=read(2, ns * 8).reshape(ns, 8), pool=read(3, pool, np.float32),
                    pmf=read(4, lights, np.float32), cdf=read(5, lights + 1, np.float32), blob=read(6, blob * 4).reshape(blob, 4),
                    texels=read(7, texels * 3, np.float32).reshape(texels, 3), textures=read(8, nt * 16).reshape(nt, 16),
                    mat_tex=read(9, nm * 4, np.int32).reshape(nm, 4))

    def set_camera(self, camera):
        """Replaces the camera of the uploaded scene (slrhip_set_camera; an abi.Camera): later launches see it, nothing is reset."""
        _check(self.lib, self.lib.slrhip_set_camera(self.handle, C.byref(camera)), "slrhip_set_camera")

    def debug_top_level(self):
        """Diagnostic (slrhip_debug_top_level): the top level of the instanced scene as a dict of numpy arrays — levels (first node of
        each level, then the number of top-level nodes), group_nodes (the widest level the refit takes in one workgroup), nodes
        [all nodes, 32] uint32 (QNode words; the first top_nodes are the top level), instances [n, 36] uint32 (DevInstance words),
        boxes [n, 2, 4] float32 (lo, hi), mesh_boxes [m, 2, 4] float32.  Synchronises."""
        def read(what, words, dtype=np.uint32):
            out = np.zeros(words, dtype)
            _check(self.lib, self.lib.slrhip_debug_top_level(self.handle, what, out.ctypes.data, out.size), "slrhip_debug_top_level")
            return out
        head = read(1, 32)
        levels, top, total, n, meshes = (int(v) for v in head[:5])
        return dict(levels=head[8:8 + levels + 1].copy(), top_nodes=top, group_nodes=int(head[5]), nodes=read(4, total * 32).reshape(total, 32),
                    instances=read(2, n * 36).reshape(n, 36), boxes=read(3, n * 8, np.float32).reshape(n, 2, 4),
                    mesh_boxes=read(5, meshes * 8, np.float32).reshape(meshes, 2, 4))

    # ---- repairing the top level after instances have moved (slrhip_rebuild_top_level) ----
    def rebuild_top_level(self, stream=None):
        """Re-seats the leaves of the top-level tree in Morton order and refits it (slrhip_rebuild_top_level), ordered on `stream` (a
        torch stream, a raw handle, None = the null stream).  The first call after an upload builds its tables and synchronises; later
        calls return at once.  Hits, frames and counters do not change; speed does, in either direction: see top_level_cost()."""
        _check(self.lib, self.lib.slrhip_rebuild_top_level(self.handle, self._stream_handle(stream)), "slrhip_rebuild_top_level")

    def top_level_cost(self, stream=None):
        """The surface-area cost of the top level as it stands (slrhip_top_level_cost): the expected number of top-level nodes a
        random line through the root box visits.  Waits for `stream`."""
        cost = C.c_double(0.0)
        _check(self.lib, self.lib.slrhip_top_level_cost(self.handle, C.byref(cost), self._stream_handle(stream)), "slrhip_top_level_cost")
        return cost.value

    def debug_top_level_rebuild(self):
        """Diagnostic (slrhip_debug_top_level_rebuild): primitives (0 before the first rebuild after an upload), seat_group (the most
        primitives the one-workgroup path takes), path ("none", "group" or "radix": the last call's), launches (the last call's, the
        refit's included, the radix sort counted as one), num_instances, slots and refs [primitives] uint32, keys [primitives] uint64
        and order [primitives] uint32 of the last call.  Synchronises."""
        def read(what, count, dtype=np.uint32):
            out = np.zeros(count, dtype)
            _check(self.lib, self.lib.slrhip_debug_top_level_rebuild(self.handle, what, out.ctypes.data, out.nbytes // 4), "slrhip_debug_top_level_rebuild")
            return out
        head = read(0, 8)
        n = int(head[0])
        return dict(primitives=n, seat_group=int(head[1]), path=("none", "group", "radix")[int(head[2])], launches=int(head[3]),
                    num_instances=int(head[4]), slots=read(1, n), refs=read(2, n), keys=read(3, n, np.uint64), order=read(4, n))

    def debug_tree(self, summary_only=False):
        """Diagnostic (slrhip_debug_tree): the tree of the uploaded scene, whichever builder made it, as the dict _read_tree describes
        (summary_only: without the arrays, and without a synchronisation).  tree["builder_name"] says which builder ran."""
        return _read_tree(self.lib, lambda what, ptr, words: self.lib.slrhip_debug_tree(self.handle, what, ptr, words), "slrhip_debug_tree",
                          summary_only)

    def render_begin(self, settings, shard=(0, 1)):
        _check(self.lib, self.lib.slrhip_render_begin(self.handle, C.byref(settings), abi.Shard(*shard)), "slrhip_render_begin")
        self.settings = settings          # a refused call leaves the previous render state, and its frame size, in place
        self.shard = tuple(shard)

    def render(self, spp_begin, spp_count, stream=None):
        _check(self.lib, self.lib.slrhip_render(self.handle, spp_begin, spp_count, stream), "slrhip_render")

    def resolve_into(self, device_ptr, num_floats, stream=None):
        _check(self.lib, self.lib.slrhip_resolve_framebuffer(self.handle, device_ptr, num_floats, stream),
               "slrhip_resolve_framebuffer")

    def read_framebuffer(self):
        return self._read_frame("slrhip_read_framebuffer")

    def _read_frame(self, symbol, *more):
        """A [height, width, components] frame through slrhip_read_framebuffer, _mean or slrhip_read_albedo."""
        fb = np.zeros((self.settings.image_height, self.settings.image_width, self.components), np.float32)
        _check(self.lib, getattr(self.lib, symbol)(self.handle, fb.ctypes.data, fb.size, *more), symbol)
        return fb

    def _read_plane(self, symbol, channel):
        """One [height, width] channel through slrhip_read_statistics or slrhip_read_clamp."""
        out = np.empty((self.settings.image_height, self.settings.image_width), np.float32)
        _check(self.lib, getattr(self.lib, symbol)(self.handle, channel, out.ctypes.data, out.size), symbol)
        return out

    def _summary(self, symbol, summary, stream):
        """The fields of a slrhip_*_summary struct as a dict."""
        _check(self.lib, getattr(self.lib, symbol)(self.handle, C.byref(summary), self._stream_handle(stream)), symbol)
        return self._summary_dict(summary)

    def synchronize(self):
        _check(self.lib, self.lib.slrhip_synchronize(self.handle), "slrhip_synchronize")

    def counters(self):
        c = abi.Counters()
        _check(self.lib, self.lib.slrhip_get_counters(self.handle, C.byref(c)), "slrhip_get_counters")
        return c

    def primary_samples(self):
        """Diagnostic (slrhip_debug_primary_samples): samples since render_begin whose first hit came from the primary pass's record."""
        n = C.c_uint64()
        _check(self.lib, self.lib.slrhip_debug_primary_samples(self.handle, C.byref(n)), "slrhip_debug_primary_samples")
        return n.value

    def shadow_skipped(self):
        """Diagnostic (slrhip_debug_shadow_skipped): light samples since render_begin that were counted as shadow rays and not traced."""
        n = C.c_uint64()
        _check(self.lib, self.lib.slrhip_debug_shadow_skipped(self.handle, C.byref(n)), "slrhip_debug_shadow_skipped")
        return n.value

    def primary_kernel(self):
        """Diagnostic (slrhip_debug_primary_kernel): the kernel of the last window's primary pass: 0 = no pass, 1 = ring, 2 = direct."""
        k = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_debug_primary_kernel(self.handle, C.byref(k)), "slrhip_debug_primary_kernel")
        return int(k.value)

    def shade_kernel(self):
        """Diagnostic (slrhip_debug_shade_kernel): the last window's k_shade instantiation as a tuple (spectral, tables in LDS, glossy
        lobes, MultiBSDF, textures, PRIMARY, RESUME), whether it was launched, and whether the tail kernel, its twin, was."""
        k = (C.c_uint32 * 9)()
        _check(self.lib, self.lib.slrhip_debug_shade_kernel(self.handle, k), "slrhip_debug_shade_kernel")
        return tuple(int(x) for x in k[:7]), bool(k[7]), bool(k[8])

    def primary_pass(self, kernel, first_pass, num_passes, window_passes, records, streams=0):
        """Diagnostic (slrhip_debug_primary_pass): one launch of the primary pass of the render last begun, `kernel` 0 = ring, 1 = direct,
        into the caller's device memory (addresses as integers; streams 0 = no stream plane)."""
        _check(self.lib, self.lib.slrhip_debug_primary_pass(self.handle, kernel, first_pass, num_passes, window_passes, records, streams or None),
               "slrhip_debug_primary_pass")

    def primary_stream_entries(self):
        """Diagnostic (slrhip_debug_primary_stream_entries): entries of the stream plane the last window bound; 0 = it ran no primary pass."""
        n = C.c_uint64()
        _check(self.lib, self.lib.slrhip_debug_primary_stream_entries(self.handle, C.byref(n)), "slrhip_debug_primary_stream_entries")
        return n.value

    def profile(self):
        p = abi.Profile()
        _check(self.lib, self.lib.slrhip_get_profile(self.handle, C.byref(p)), "slrhip_get_profile")
        return p

    def trace_rays(self, org, direction, dist_min, dist_max):
        n = len(org)
        rays = np.zeros((n, 8), np.float32)
        rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = org, direction, dist_min, dist_max
        hits = np.zeros((n, 4), np.float32)
        _check(self.lib, self.lib.slrhip_trace_rays(self.handle, rays.ctypes.data, n, hits.ctypes.data), "slrhip_trace_rays")
        return hits[:, 0].copy().view(np.uint32), hits[:, 1], hits[:, 2], hits[:, 3]

    # ---- ray queries on device memory (slrhip_intersect_rays / slrhip_test_visibility) ----------------------------------
    # torch ships its own copy of the HIP runtime, and only one copy can open the device in a process.  libslrhip.so binds to
    # torch's copy when torch is imported before the library is loaded (bench.py's order); then torch tensors and streams are
    # passed straight through.  Numpy inputs go through the runtime the library itself is bound to, whichever copy that is.
    def _query(self, rays, stream, outs, call):
        """outs: [(name, shape, numpy dtype)]; call(rays_ptr, n, {name: ptr}, stream_handle)."""
        if isinstance(rays, np.ndarray):
            return self._query_host(rays, outs, call)
        import torch
        if not (isinstance(rays, torch.Tensor) and rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 8
                and rays.is_contiguous()):
            raise ValueError("rays: a contiguous [n, 8] float32 CUDA tensor (or a numpy array) expected")
        if not torch.cuda.is_available() or rays.device.index != self.device:
            raise SlrHipError("ray queries on torch tensors need libslrhip.so bound to torch's HIP runtime on the tensor's device: "
                              "import torch before the first Context, and pass tensors on device %d" % self.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            res = {name: torch.empty(shape(rays.shape[0]), dtype=getattr(torch, np.dtype(dt).name), device=rays.device) for name, shape, dt in outs}
            call(rays.data_ptr(), rays.shape[0], {k: v.data_ptr() for k, v in res.items()}, s.cuda_stream)
        return tuple(res[name] for name, _, _ in outs) if len(outs) > 1 else res[outs[0][0]]

    def _query_host(self, rays, outs, call):
        a = rays.view(np.float32) if rays.dtype == abi.ray_dtype else rays
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 8)
        n = len(a)
        shapes = {name: (shape(n), np.dtype(dt)) for name, shape, dt in outs}
        with DeviceBlocks() as dev:
            ptrs = {name: dev.alloc(int(np.prod(sh)) * dt.itemsize) for name, (sh, dt) in shapes.items()}
            call(dev.put(a), n, ptrs, None)
            bits = self.query_status(0)
            host = {name: dev.get(ptrs[name], sh, dt) for name, (sh, dt) in shapes.items()}
        if bits:
            raise SlrHipError("ray query: the query error word is 0x%x (a traversal gave up)" % bits)
        return tuple(host[name] for name, _, _ in outs) if len(outs) > 1 else host[outs[0][0]]

    def intersect_rays(self, rays, stream=None, want_instances=False):
        """Closest hits (slrhip_intersect_rays).  rays: a torch CUDA tensor [n, 8] float32 (slrhip_ray rows: org, dist_min, dir,
        dist_max), contiguous and 16-byte aligned, passed without a copy and queried in order on `stream` (default:
        torch.cuda.current_stream()); returns device tensors at once: hits [n, 4] float32 = slrhip_hit rows (column 0 holds the
        triangle index's bits, 0xFFFFFFFF = miss; dist; b0; b1) and, with want_instances, instances [n] int32 (-1: a loose triangle
        or a miss).  Check query_status(stream) before trusting them.  A numpy array of the same rows (or of abi.ray_dtype records)
        is COPIED to the device and the results back (numpy arrays); that call synchronises and raises if the query error word
        is set."""
        outs = [("hits", lambda n: (n, 4), np.float32)] + ([("instances", lambda n: (n,), np.int32)] if want_instances else [])

        def call(r, n, p, handle):
            _check(self.lib, self.lib.slrhip_intersect_rays(self.handle, r, n, p["hits"], p.get("instances"), handle), "slrhip_intersect_rays")
        return self._query(rays, stream, outs, call)

    def test_visibility(self, rays, stream=None):
        """Visibility (slrhip_test_visibility): [n] int32, 1 = no triangle in [dist_min, dist_max].  Same conventions as
        intersect_rays (device tensors in and out without a copy; numpy arrays copied both ways)."""
        def call(r, n, p, handle):
            _check(self.lib, self.lib.slrhip_test_visibility(self.handle, r, n, p["visible"], handle), "slrhip_test_visibility")
        return self._query(rays, stream, [("visible", lambda n: (n,), np.int32)], call)

    def query_status(self, stream=None):
        """The query error word after the queries ordered on `stream` (a torch stream, a raw handle, 0 = the null stream; default:
        torch.cuda.current_stream()); waits for that stream only."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)
        bits = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_query_status(self.handle, C.byref(bits), getattr(stream, "cuda_stream", stream) or None),
               "slrhip_query_status")
        return bits.value

    # ---- first-hit feature buffers and camera rays (slrhip_render_features / slrhip_resolve_features / slrhip_camera_rays) ----
    def _stream_handle(self, stream):
        return getattr(stream, "cuda_stream", stream) or None

    def _num_pixels(self):
        """Pixels of this context's shard, as the render plan counts them (slrhip_camera_rays reports it at the call)."""
        count = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_camera_rays(self.handle, 0, None, None, 0, C.byref(count), None), "slrhip_camera_rays")
        return count.value

    def render_features(self, channels, spp, spp_begin=0, stream=None):
        """Feature passes [spp_begin, spp_begin + spp) of every pixel of the shard (slrhip_render_features): ordered on `stream`
        (a torch stream, a raw handle, None = the null stream), returns at once."""
        _check(self.lib, self.lib.slrhip_render_features(self.handle, channels, spp_begin, spp, self._stream_handle(stream)), "slrhip_render_features")

    def features_status(self, stream=None):
        bits = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_features_status(self.handle, C.byref(bits), self._stream_handle(stream)), "slrhip_features_status")
        return bits.value

    def features_into(self, channel, device_ptr, num_elements, stream=None):
        """One channel into device memory at `device_ptr` (slrhip_resolve_features), ordered on `stream`."""
        _check(self.lib, self.lib.slrhip_resolve_features(self.handle, channel, device_ptr, num_elements, self._stream_handle(stream)),
               "slrhip_resolve_features")

    def features(self, channel):
        """One channel as a numpy array [height, width, k] (k = 3, or [height, width] for DISTANCE / COVERAGE; float32, IDS:
        uint32): the per-pixel sums in pass order, zeros (IDS: 0xFFFFFFFF) outside the shard.  Synchronises, and raises if the
        feature error word is set."""
        if channel not in abi.FEATURE_CHANNELS:
            raise ValueError("channel: one abi.FEATURE_* bit expected")
        _, k, dt = abi.FEATURE_CHANNELS[channel]
        h, w = self.settings.image_height, self.settings.image_width
        out = np.empty((h, w, k), dt)
        _check(self.lib, self.lib.slrhip_read_features(self.handle, channel, out.ctypes.data, out.size), "slrhip_read_features")
        return out if k == 3 else out[:, :, 0]

    # ---- the albedo buffer (slrhip_render_albedo / slrhip_resolve_albedo / slrhip_read_albedo) ----
    def render_albedo(self, spp, spp_begin=0, stream=None):
        """Albedo passes [spp_begin, spp_begin + spp) of every pixel of the shard (slrhip_render_albedo): the base colour of the
        camera ray's first hit, a miss counting as one.  Ordered on `stream`, returns at once."""
        _check(self.lib, self.lib.slrhip_render_albedo(self.handle, spp_begin, spp, self._stream_handle(stream)), "slrhip_render_albedo")

    def albedo_into(self, device_ptr, num_floats, stream=None):
        """The albedo SUMS into device memory at `device_ptr` ([height, width, components] float32; slrhip_resolve_albedo), ordered
        on `stream`; returns the number of passes accumulated since render_begin (the divisor of the mean)."""
        passes = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_resolve_albedo(self.handle, device_ptr, num_floats, C.byref(passes), self._stream_handle(stream)),
               "slrhip_resolve_albedo")
        return passes.value

    def albedo(self):
        """(sums [height, width, components] float32, passes): the per-pixel albedo sums in pass order, zeros outside the shard, and the
        passes accumulated; sums / passes is the mean albedo.  Synchronises, and raises if the feature error word is set."""
        passes = C.c_uint32(0)
        return self._read_frame("slrhip_read_albedo", C.byref(passes)), passes.value

    # ---- motion vectors (slrhip_render_motion / slrhip_resolve_motion / slrhip_read_motion) ----
    def render_motion(self, spp, previous_camera=None, previous_transforms=None, spp_begin=0, stream=None, previous_vertices=None):
        """Motion passes [spp_begin, spp_begin + spp) of every pixel of the shard (slrhip_render_motion): where on the PREVIOUS frame's
        image was the point each sample's camera ray hits now?  previous_camera: the abi.Camera of the previous frame (None: the
        camera did not move; taken by value).  previous_transforms: the matrices ALL instances had in the previous frame (None: no
        instance moved) — a numpy [n, 32] float32 array (or abi.instance_transform_dtype / abi.instance_dtype records), copied to
        the device first (that call synchronises); or a contiguous [n, 32] float32 torch CUDA tensor or a device address (int), read
        in order on `stream` without a copy.  previous_vertices: ALL vertices of the scene as the previous frame had them (None: no
        vertex moved); given, the call goes to slrhip_render_motion_vertices (contexts that keep the vertex array: set_vertices) —
        numpy records of abi.vertex_dtype or an [n, 11] float32 array, staged like previous_transforms; or a contiguous [n, 11] float32
        torch CUDA tensor or a device address (int).  Every call between two render_begin calls must name the same previous frame."""
        cam = C.pointer(previous_camera) if previous_camera is not None else None
        handle = self._stream_handle(stream)

        def device_address(t, columns, what):
            if t is None or isinstance(t, int):
                return t
            if not (t.is_cuda and t.dim() == 2 and t.shape[1] == columns and t.is_contiguous() and t.element_size() == 4 and t.is_floating_point()):
                raise ValueError("%s: a contiguous [n, %d] float32 CUDA tensor, a numpy array or a device address expected" % (what, columns))
            if t.device.index != self.device:
                raise SlrHipError("render_motion: the tensor is on device %r, the context on device %d" % (t.device.index, self.device))
            return t.data_ptr()

        host = [a for a in (previous_transforms, previous_vertices) if isinstance(a, np.ndarray)]
        if not host:
            return self._render_motion(cam, device_address(previous_transforms, 32, "previous_transforms"),
                                       device_address(previous_vertices, 11, "previous_vertices"), spp_begin, spp, handle)
        with DeviceBlocks() as dev:
            if isinstance(previous_transforms, np.ndarray):
                a = previous_transforms
                if a.dtype == abi.instance_dtype:
                    a = np.concatenate([a["local_to_world"], a["world_to_local"]], axis=1)
                elif a.dtype == abi.instance_transform_dtype:
                    a = np.ascontiguousarray(a).view(np.float32)
                previous_transforms = dev.put(np.ascontiguousarray(a, np.float32).reshape(-1, 32))
            if isinstance(previous_vertices, np.ndarray):
                a = np.ascontiguousarray(previous_vertices)
                a = a.view(np.float32) if a.dtype == abi.vertex_dtype else np.ascontiguousarray(a, np.float32)
                previous_vertices = dev.put(a.reshape(-1, 11))
            self._render_motion(cam, device_address(previous_transforms, 32, "previous_transforms"),
                                device_address(previous_vertices, 11, "previous_vertices"), spp_begin, spp, handle)
            self.synchronize()                         # the staging blocks are freed on the way out

    def _render_motion(self, cam, transforms, vertices, spp_begin, spp, handle):
        """The call on device addresses: slrhip_render_motion, or slrhip_render_motion_vertices where `vertices` is given."""
        frame = abi.MotionDesc(cam, transforms, (C.c_uint32 * 2)(0, 0))
        if vertices is None:
            _check(self.lib, self.lib.slrhip_render_motion(self.handle, C.byref(frame), spp_begin, spp, handle), "slrhip_render_motion")
        else:
            d = abi.MotionVerticesDesc(frame, vertices, 0)
            _check(self.lib, self.lib.slrhip_render_motion_vertices(self.handle, C.byref(d), spp_begin, spp, handle), "slrhip_render_motion_vertices")

    def motion_into(self, device_ptr, num_floats, stream=None):
        """The motion SUMS into device memory at `device_ptr` ([height, width, 4] float32; slrhip_resolve_motion), ordered on `stream`."""
        _check(self.lib, self.lib.slrhip_resolve_motion(self.handle, device_ptr, num_floats, self._stream_handle(stream)), "slrhip_resolve_motion")

    def motion(self):
        """The motion sums [height, width, 4] float32 {sum m.x, sum m.y, sum z', valid samples}, zeros outside the shard; [..., :3] /
        [..., 3:] is the mean vector in pixels and the mean distance in the previous frame.  Synchronises, and raises if the feature
        error word is set."""
        out = np.zeros((self.settings.image_height, self.settings.image_width, 4), np.float32)
        _check(self.lib, self.lib.slrhip_read_motion(self.handle, out.ctypes.data, out.size), "slrhip_read_motion")
        return out

    # ---- temporal reprojection (slrhip_reproject): a pure function of device buffers ----
    def reproject_into(self, width, height, components, color, motion, coverage, prev_color, prev_length, prev_distance, prev_coverage, output,
                       output_length, variance=None, ids=None, normal=None, prev_variance=None, prev_ids=None, prev_normal=None,
                       output_variance=None, max_history=abi.REPROJECT_MAX_HISTORY, min_alpha=0.0, sigma_distance=abi.REPROJECT_SIGMA_DISTANCE,
                       min_normal_dot=abi.REPROJECT_MIN_NORMAL_DOT, stream=None):
        """slrhip_reproject over DEVICE pointers (integer addresses; None = not given): the current frame's color [H][W][C] means,
        motion [H][W][4], coverage [H][W] (and variance [H][W], ids [H][W][3] uint32, normal [H][W][3]) and what was kept of the
        previous frame (prev_color: the accumulated history, prev_length, prev_distance, prev_coverage, ...) -> output, output_length
        and, if given, output_variance.  Ordered on `stream`, returns at once.  Needs no scene and no render_begin."""
        d = abi.ReprojectDesc(width, height, components, color, variance, motion, coverage, ids, normal, prev_color, prev_variance, prev_length,
                              prev_distance, prev_coverage, prev_ids, prev_normal, output, output_variance, output_length, max_history, min_alpha,
                              sigma_distance, min_normal_dot, (C.c_uint32 * 2)(0, 0))
        _check(self.lib, self.lib.slrhip_reproject(self.handle, C.byref(d), self._stream_handle(stream)), "slrhip_reproject")

    def reproject(self, color, motion, coverage, prev_color, prev_length, prev_distance, prev_coverage, variance=None, ids=None, normal=None,
                  prev_variance=None, prev_ids=None, prev_normal=None, **params):
        """slrhip_reproject over HOST arrays (the shapes of reproject_into; ids as uint32): the arrays are copied to the device and the
        result back: (output [H, W, C], length [H, W]) or, with a variance, (output, length, variance).  **params: max_history,
        min_alpha, sigma_distance, min_normal_dot.  Synchronises."""
        color = np.ascontiguousarray(color, np.float32)
        if color.ndim != 3:
            raise ValueError("color: a [height, width, components] array expected")
        h, w, comps = color.shape
        host = {"color": color, "motion": motion, "coverage": coverage, "prev_color": prev_color, "prev_length": prev_length,
                "prev_distance": prev_distance, "prev_coverage": prev_coverage, "variance": variance, "ids": ids, "normal": normal,
                "prev_variance": prev_variance, "prev_ids": prev_ids, "prev_normal": prev_normal}
        shapes = {"color": (h, w, comps), "prev_color": (h, w, comps), "motion": (h, w, 4), "ids": (h, w, 3), "prev_ids": (h, w, 3),
                  "normal": (h, w, 3), "prev_normal": (h, w, 3)}
        with DeviceBlocks() as dev:
            ptrs = {}
            for name, a in host.items():
                if a is None:
                    continue
                a = np.ascontiguousarray(a, np.uint32 if name.endswith("ids") else np.float32)
                if a.shape != shapes.get(name, (h, w)):
                    raise ValueError("%s: shape %r expected" % (name, shapes.get(name, (h, w))))
                ptrs[name] = dev.put(a)
            output, length = dev.alloc(4 * h * w * comps), dev.alloc(4 * h * w)
            out_variance = dev.alloc(4 * h * w) if variance is not None else None
            self.reproject_into(w, h, comps, output=output, output_length=length, output_variance=out_variance, **ptrs, **params)
            self.synchronize()
            res = (dev.get(output, (h, w, comps)), dev.get(length, (h, w)))
            return res + (dev.get(out_variance, (h, w)),) if variance is not None else res

    # ---- albedo demodulation (slrhip_modulate): a pure function of device buffers ----
    def modulate_into(self, width, height, components, op, color, albedo, albedo_passes, output, variance=None, output_variance=None,
                      floor=abi.MODULATE_FLOOR, stream=None):
        """slrhip_modulate over DEVICE pointers (integer addresses; None = not given): color [H][W][C] divided by (abi.MODULATE_DIVIDE)
        or multiplied with (abi.MODULATE_MULTIPLY) max(albedo / albedo_passes, floor) -> output, which may be `color` itself; the
        variance of the luminance [H][W] is scaled by the square of the albedo's luminance.  Ordered on `stream`, returns at once."""
        d = abi.ModulateDesc(width, height, components, op, color, variance, albedo, output, output_variance, albedo_passes, floor, 0)
        _check(self.lib, self.lib.slrhip_modulate(self.handle, C.byref(d), self._stream_handle(stream)), "slrhip_modulate")

    def modulate(self, color, albedo, passes, op, variance=None, floor=abi.MODULATE_FLOOR):
        """slrhip_modulate over HOST arrays: color and albedo sums [H, W, 3 or 16], variance [H, W] or None.  The arrays are copied to
        the device and the result back: the frame, or (frame, variance) when a variance is given.  Synchronises."""
        color, albedo = np.ascontiguousarray(color, np.float32), np.ascontiguousarray(albedo, np.float32)
        if color.ndim != 3 or albedo.shape != color.shape:
            raise ValueError("color and albedo: two [height, width, components] arrays of one shape expected")
        h, w, comps = color.shape
        if variance is not None:
            variance = np.ascontiguousarray(variance, np.float32)
            if variance.shape != (h, w):
                raise ValueError("variance: shape %r expected" % ((h, w),))
        with DeviceBlocks() as dev:
            pc, pa = dev.put(color), dev.put(albedo)
            pv = dev.put(variance) if variance is not None else None
            self.modulate_into(w, h, comps, op, pc, pa, passes, pc, pv, pv, floor)      # in place
            self.synchronize()
            out = dev.get(pc, color.shape)
            return out if variance is None else (out, dev.get(pv, variance.shape))

    def camera_rays(self, pass_, device=False, stream=None):
        """The camera rays of sample `pass_` of every pixel of the shard (slrhip_camera_rays): (rows, pixel_xy), rows [n, 8] float32
        in the format intersect_rays takes, pixel_xy [n] = x | y << 16.  Numpy arrays by default (the call synchronises);
        device=True: torch CUDA tensors (float32, int32) written in order on `stream` (default: torch.cuda.current_stream()),
        returned at once."""
        n = self._num_pixels()
        count = C.c_uint32(0)
        if device:
            import torch
            s = stream if stream is not None else torch.cuda.current_stream(self.device)
            with torch.cuda.stream(s):
                rows = torch.empty((n, 8), dtype=torch.float32, device="cuda:%d" % self.device)
                xy = torch.empty((n,), dtype=torch.int32, device="cuda:%d" % self.device)
                _check(self.lib, self.lib.slrhip_camera_rays(self.handle, pass_, rows.data_ptr(), xy.data_ptr(), n, C.byref(count), s.cuda_stream),
                       "slrhip_camera_rays")
            return rows, xy
        with DeviceBlocks() as dev:
            pr, px = dev.alloc(32 * n), dev.alloc(4 * n)
            _check(self.lib, self.lib.slrhip_camera_rays(self.handle, pass_, pr, px, n, C.byref(count), None), "slrhip_camera_rays")
            self.synchronize()
            return dev.get(pr, (n, 8)), dev.get(px, (n,), np.uint32)

    # ---- per-pixel noise statistics and rendering to a noise target (slrhip_statistics_begin ... slrhip_render_until) ----
    def statistics_begin(self):
        """Switches the noise statistics on for the render that render_begin just began (before its first render())."""
        _check(self.lib, self.lib.slrhip_statistics_begin(self.handle), "slrhip_statistics_begin")

    def statistics_into(self, channel, device_ptr, num_floats, stream=None):
        """One abi.STATISTICS_* channel into device memory at `device_ptr` ([height, width] float32), ordered on `stream`."""
        _check(self.lib, self.lib.slrhip_resolve_statistics(self.handle, channel, device_ptr, num_floats, self._stream_handle(stream)),
               "slrhip_resolve_statistics")

    def statistics(self, channel):
        """One abi.STATISTICS_* channel as a numpy array [height, width] float32, zeros outside the shard.  Synchronises."""
        return self._read_plane("slrhip_read_statistics", channel)

    @staticmethod
    def _summary_dict(s):
        return {name: getattr(s, name) for name, _ in s._fields_ if name != "reserved"}

    def statistics_summary(self, stream=None):
        """The shard's totals (slrhip_statistics_summary) as a dict; waits for `stream` only.  Dicts of shards add field by
        field, except max_sample (take the larger); abi.noise_metric evaluates the stop check on one."""
        return self._summary("slrhip_statistics_summary", abi.StatisticsSummary(), stream)

    def render_until(self, metric, target, step, spp_max, spp_begin=0, stream=None):
        """Renders blocks of `step` passes from `spp_begin` until abi.noise_metric(summary, metric) <= target (and every pixel has
        2 samples) or `spp_max` passes are done (slrhip_render_until): (spp_done, summary of the last stop check).  The frame
        is bit-identical to render(spp_begin, spp_done).  Needs statistics_begin()."""
        t = abi.NoiseTarget(metric, target, step, spp_max)
        done, last = C.c_uint32(0), abi.StatisticsSummary()
        _check(self.lib, self.lib.slrhip_render_until(self.handle, spp_begin, C.byref(t), C.byref(done), C.byref(last), self._stream_handle(stream)),
               "slrhip_render_until")
        return done.value, self._summary_dict(last)

    # ---- the sample clamp (slrhip_clamp_begin / slrhip_resolve_clamp / slrhip_clamp_summary) ----
    def clamp_begin(self, limit, drop_nonfinite=False):
        """Switches the sample clamp on for the render that render_begin just began (before its first render()): a sample whose
        luminance exceeds `limit` (un-normalised, the units of sample_luminance) is scaled down to it; with `drop_nonfinite` a
        sample whose luminance is NaN or infinite is replaced by zero.  limit = inf: drop only."""
        d = abi.ClampDesc(limit, abi.CLAMP_DROP_NONFINITE if drop_nonfinite else 0)
        _check(self.lib, self.lib.slrhip_clamp_begin(self.handle, C.byref(d)), "slrhip_clamp_begin")

    def clamp_into(self, channel, device_ptr, num_floats, stream=None):
        """One abi.CLAMP_* channel into device memory at `device_ptr` ([height, width] float32), ordered on `stream`."""
        _check(self.lib, self.lib.slrhip_resolve_clamp(self.handle, channel, device_ptr, num_floats, self._stream_handle(stream)), "slrhip_resolve_clamp")

    def clamp(self, channel):
        """One abi.CLAMP_* channel as a numpy array [height, width] float32, zeros outside the shard.  Synchronises."""
        return self._read_plane("slrhip_read_clamp", channel)

    def clamp_summary(self, stream=None):
        """The shard's totals (slrhip_clamp_summary) as a dict; waits for `stream` only.  Dicts of shards add field by field,
        except `largest` (take the larger)."""
        return self._summary("slrhip_clamp_summary", abi.ClampSummary(), stream)

    def debug_fold(self, samples):
        """Diagnostic (slrhip_debug_fold): `samples` [passes, height, width, components] float32 through the fold of the context's
        current state (statistics and clamp on or off), added to the sensor and the records.  Blocking."""
        h, w = self.settings.image_height, self.settings.image_width
        samples = np.ascontiguousarray(samples, np.float32)
        if samples.ndim != 4 or samples.shape[1:] != (h, w, self.components):
            raise ValueError("debug_fold: samples must be [passes, %d, %d, %d]" % (h, w, self.components))
        _check(self.lib, self.lib.slrhip_debug_fold(self.handle, samples.ctypes.data, samples.shape[0]), "slrhip_debug_fold")

    # ---- adaptive sampling (slrhip_render_adaptive / slrhip_read_framebuffer_mean / slrhip_adaptive_active) ----
    def render_adaptive(self, spp_begin, threshold, floor, spp_min, spp_step, spp_max, stream=None):
        """Renders blocks of passes from `spp_begin` (spp_min, then spp_step each, cut to spp_max) and retires, after each block,
        the pixels whose relative standard error of the mean luminance is at most `threshold` (relative to `floor` for darker
        pixels); later blocks render only the rest (slrhip_render_adaptive): (spp_done of the longest-lived pixel, samples
        rendered).  Needs statistics_begin(); the per-pixel counts are statistics(abi.STATISTICS_COUNT)."""
        t = abi.AdaptiveTarget(threshold, floor, spp_min, spp_step, spp_max)
        done, samples = C.c_uint32(0), C.c_uint64(0)
        _check(self.lib, self.lib.slrhip_render_adaptive(self.handle, spp_begin, C.byref(t), C.byref(done), C.byref(samples), self._stream_handle(stream)),
               "slrhip_render_adaptive")
        return done.value, samples.value

    def mean_into(self, device_ptr, num_floats, stream=None):
        """The mean frame into device memory at `device_ptr` (slrhip_resolve_framebuffer_mean), ordered on `stream`."""
        _check(self.lib, self.lib.slrhip_resolve_framebuffer_mean(self.handle, device_ptr, num_floats, self._stream_handle(stream)),
               "slrhip_resolve_framebuffer_mean")

    def read_framebuffer_mean(self):
        """The frame as per-pixel means [height, width, components]: sum / count with the count of the pixel's noise record, 0
        where no sample was rendered and outside the shard.  Needs statistics_begin(); synchronises."""
        return self._read_frame("slrhip_read_framebuffer_mean")

    def adaptive_active(self, stream=None):
        """Pixels of the shard that have not retired since render_begin (slrhip_adaptive_active)."""
        count = C.c_uint32(0)
        _check(self.lib, self.lib.slrhip_adaptive_active(self.handle, C.byref(count), self._stream_handle(stream)), "slrhip_adaptive_active")
        return count.value

    # ---- denoising (slrhip_denoise): a pure function of device buffers ----
    def denoise_into(self, width, height, components, iterations, color, output, variance=None, normal=None, distance=None, coverage=None,
                     output_variance=None, sigma_luminance=4.0, sigma_distance=abi.DENOISE_SIGMA_DISTANCE, normal_power_log2=7, stream=None):
        """The filter of include/slrhip.h over DEVICE pointers (integer addresses; None = not given): color [H][W][C] means,
        variance [H][W], normal [H][W][3] and distance [H][W] sums, coverage [H][W] -> output [H][W][C] and, if given,
        output_variance [H][W].  Ordered on `stream`, returns at once.  Needs no scene and no render_begin."""
        d = abi.DenoiseDesc(width, height, components, iterations, color, variance, normal, distance, coverage, output, output_variance,
                            sigma_luminance, sigma_distance, normal_power_log2, 0)
        _check(self.lib, self.lib.slrhip_denoise(self.handle, C.byref(d), self._stream_handle(stream)), "slrhip_denoise")

    def _denoise_staged(self, shape, fill, params, want_variance, image=None, demodulate=None):
        """hipMalloc the buffers of a denoise call, let `fill(name, device_ptr)` fill the inputs (a name it returns False for is
        passed as NULL), run the filter on the null stream and copy the result back; with image = (scale, format) the result stays
        on the device, is tone-mapped there (slrhip_tonemap) and only the 8-bit image comes back.  demodulate = floor: the albedo is
        resolved on the device as well (albedo_into), colour and variance are divided by it before the filter and its outputs
        multiplied with it afterwards (slrhip_modulate, in place)."""
        h, w, comps = shape
        sizes = {"color": h * w * comps, "variance": h * w, "normal": h * w * 3, "distance": h * w, "coverage": h * w}
        with DeviceBlocks() as dev:
            given = {name: dev.alloc(4 * n) for name, n in sizes.items() if fill(name, None)}
            for name, p in given.items():
                fill(name, p)
            if demodulate is not None:
                if want_variance and "variance" not in given:
                    raise ValueError("demodulate with want_variance needs a variance input: the filtered variance could not be multiplied back")
                albedo = dev.alloc(4 * sizes["color"])
                passes = self.albedo_into(albedo, sizes["color"])
                self.modulate_into(w, h, comps, abi.MODULATE_DIVIDE, given["color"], albedo, passes, given["color"], given.get("variance"),
                                   given.get("variance"), demodulate)
            output = dev.alloc(4 * sizes["color"])
            output_variance = dev.alloc(4 * h * w) if want_variance else None
            self.denoise_into(w, h, comps, color=given["color"], output=output, output_variance=output_variance,
                              **{k: given.get(k) for k in ("variance", "normal", "distance", "coverage")}, **params)
            if demodulate is not None:
                pv = output_variance if given.get("variance") else None
                self.modulate_into(w, h, comps, abi.MODULATE_MULTIPLY, output, albedo, passes, output, pv, pv, demodulate)
            if image is not None:
                return self._tonemap_staged(output, w, h, comps, *image)
            self.synchronize()
            out = dev.get(output, (h, w, comps))
            return (out, dev.get(output_variance, (h, w))) if want_variance else out

    def denoise(self, color, variance=None, normal=None, distance=None, coverage=None, iterations=5, sigma_luminance=4.0,
                sigma_distance=abi.DENOISE_SIGMA_DISTANCE, normal_power_log2=7, want_variance=False):
        """The filter over HOST arrays: color [H, W, 3 or 16] per-pixel means, the guides as the read-outs give them (variance of the
        mean luminance [H, W]; sums of shading normals [H, W, 3] and distances [H, W]; coverage [H, W]; None = not given).  The
        arrays are copied to the device and the result back: the filtered frame, or (frame, filtered variance) with
        want_variance.  Synchronises."""
        host = {"color": color, "variance": variance, "normal": normal, "distance": distance, "coverage": coverage}
        host = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in host.items() if v is not None}
        if host["color"].ndim != 3:
            raise ValueError("color: a [height, width, components] array expected")
        h, w, _ = shape = host["color"].shape
        for name, want in (("variance", (h, w)), ("normal", (h, w, 3)), ("distance", (h, w)), ("coverage", (h, w))):
            if name in host and host[name].shape != want:
                raise ValueError("%s: shape %r expected" % (name, want))
        hip = _hip_runtime()

        def fill(name, ptr):
            if ptr is not None:
                _hip_check(hip.hipMemcpy(ptr, host[name].ctypes.data, host[name].nbytes, 1), "hipMemcpy")
            return name in host
        params = dict(iterations=iterations, sigma_luminance=sigma_luminance, sigma_distance=sigma_distance, normal_power_log2=normal_power_log2)
        return self._denoise_staged(shape, fill, params, want_variance)

    def denoised(self, want_variance=False, image=None, demodulate=False, floor=abi.MODULATE_FLOOR, **params):
        """The current render's frame, denoised: after a render with statistics on and render_features(abi.FEATURE_SHADING_NORMAL |
        abi.FEATURE_DISTANCE | abi.FEATURE_COVERAGE, ...).  The mean frame, the variance of the mean and the three guides are
        resolved ON THE DEVICE and filtered there; only the result comes back.  **params: iterations, sigma_luminance,
        sigma_distance, normal_power_log2 of denoise().  A whole-image shard only: the taps of a pixel reach into other shards'
        tiles (a multi-GPU host reduces the five buffers onto one rank and denoises there).  image = (scale, abi.IMAGE_*): the
        filtered frame is tone-mapped on the device as well and the 8-bit image (as frame_image returns it) comes back in its place.
        demodulate=True (after render_albedo): the frame and its variance are divided by the mean first-hit albedo (never less than
        `floor`) before the filter and the results multiplied back, so that texture detail the guides do not see passes the filter."""
        if self.settings is None:
            raise SlrHipError("denoised: call render_begin first")
        if tuple(self.shard) != (0, 1):
            raise SlrHipError("denoised: the context renders shard %r; the filter needs the whole image (reduce the buffers, then denoise)" % (self.shard,))
        h, w = self.settings.image_height, self.settings.image_width
        resolve = {"color": lambda p, n: self.mean_into(p, n),
                   "variance": lambda p, n: self.statistics_into(abi.STATISTICS_VARIANCE_OF_MEAN, p, n),
                   "normal": lambda p, n: self.features_into(abi.FEATURE_SHADING_NORMAL, p, n),
                   "distance": lambda p, n: self.features_into(abi.FEATURE_DISTANCE, p, n),
                   "coverage": lambda p, n: self.features_into(abi.FEATURE_COVERAGE, p, n)}
        floats = {"color": h * w * self.components, "variance": h * w, "normal": h * w * 3, "distance": h * w, "coverage": h * w}

        def fill(name, ptr):
            if ptr is not None:
                resolve[name](ptr, floats[name])
            return True
        params.setdefault("iterations", 5)
        return self._denoise_staged((h, w, self.components), fill, params, want_variance, image, floor if demodulate else None)

    # ---- image export on the device (slrhip_tonemap): a pure function of device buffers ----
    def tonemap_into(self, width, height, components, color_ptr, output_ptr, output_bytes, scale, format, stream=None):
        """The image export of include/slrhip.h over DEVICE pointers (integer addresses): color [H][W][C] floats times `scale` ->
        the 8-bit image in `format` (abi.IMAGE_BGR8_BMP, abi.IMAGE_RGBA8) at output, which has room for output_bytes.  Ordered on
        `stream`, returns at once.  Needs no scene and no render_begin."""
        d = abi.TonemapDesc(width, height, components, format, color_ptr, output_ptr, output_bytes, scale, 0)
        _check(self.lib, self.lib.slrhip_tonemap(self.handle, C.byref(d), self._stream_handle(stream)), "slrhip_tonemap")

    def tonemap(self, color, scale, format=abi.IMAGE_RGBA8):
        """The image of a torch CUDA tensor [H, W, 3 or 16] float32 (contiguous), passed without a copy and tone-mapped in order on
        torch.cuda.current_stream(): a uint8 device tensor, [H, W, 4] for abi.IMAGE_RGBA8, the flat padded bottom-up rows
        (slrhip_save_bmp's input) for abi.IMAGE_BGR8_BMP.  Returns at once.  Needs libslrhip.so bound to torch's HIP runtime: import
        torch before the first Context."""
        import torch
        if not (isinstance(color, torch.Tensor) and color.is_cuda and color.dtype == torch.float32 and color.dim() == 3 and color.is_contiguous()):
            raise ValueError("color: a contiguous [height, width, components] float32 CUDA tensor expected")
        if color.device.index != self.device:
            raise SlrHipError("tonemap: the tensor is on device %r, the context on device %d" % (color.device.index, self.device))
        h, w, comps = color.shape
        size = self.lib.slrhip_tonemap_bytes(w, h, format)
        if size == 0:
            raise ValueError("tonemap: a non-empty image of less than 2^31 pixels and a format of abi.IMAGE_* expected")
        s = torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            out = torch.empty((size,), dtype=torch.uint8, device=color.device)
            self.tonemap_into(w, h, comps, color.data_ptr(), out.data_ptr(), size, scale, format, s)
        return out.view(h, w, 4) if format == abi.IMAGE_RGBA8 else out

    def _tonemap_staged(self, color_ptr, width, height, components, scale, format):
        """The image of the device floats at color_ptr as a numpy uint8 array: hipMalloc the image, tone-map on the null stream,
        copy the 8-bit rows back."""
        size = self.lib.slrhip_tonemap_bytes(width, height, format)
        with DeviceBlocks() as dev:
            p = dev.alloc(size)
            self.tonemap_into(width, height, components, color_ptr, p, size, scale, format)
            self.synchronize()
            out = dev.get(p, (size,), np.uint8)
        return out.reshape(height, width, 4) if format == abi.IMAGE_RGBA8 else out

    def frame_image(self, scale, mean=False, format=abi.IMAGE_BGR8_BMP):
        """The current render's frame as an 8-bit image, tone-mapped ON THE DEVICE: the frame of sums (or, with mean, of per-pixel
        means: needs statistics_begin()) is resolved into device memory and only the image comes back: a numpy uint8 array, the flat
        padded rows slrhip_save_bmp takes, or [H, W, 4] for abi.IMAGE_RGBA8.  Byte for byte what slrhip_tonemap_bgr8 makes of
        read_framebuffer() / read_framebuffer_mean(), up to the last bit of exp and pow (include/slrhip.h).  Synchronises."""
        if self.settings is None:
            raise SlrHipError("frame_image: call render_begin first")
        h, w = self.settings.image_height, self.settings.image_width
        floats = h * w * self.components
        with DeviceBlocks() as dev:
            p = dev.alloc(4 * floats)
            (self.mean_into if mean else self.resolve_into)(p, floats)
            return self._tonemap_staged(p, w, h, self.components, scale, format)

    def bsdf_queries(self, material, queries, wl_offset=0.5, u_lambda=0.5):
        """Function-level BSDF queries (slrhip_bsdf_queries): queries [n][12] -> [n][6 + 2C]."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 12)
        out = np.zeros((len(q), 6 + 2 * self.components), np.float32)
        _check(self.lib, self.lib.slrhip_bsdf_queries(self.handle, material, len(q), q.ctypes.data, wl_offset, u_lambda, out.ctypes.data),
               "slrhip_bsdf_queries")
        return out

    @property
    def mode(self):
        return abi.MODE_SPECTRAL if self.components == 16 else abi.MODE_RGB

    def render_image(self, scene, settings, spp, shard=(0, 1)):
        """Convenience: upload, render all passes, read back the linear float framebuffer."""
        self.upload_scene(scene)
        self.render_begin(settings, shard)
        self.render(0, spp)
        return self.read_framebuffer()


def _read_tree(lib, call, symbol, summary_only=False):
    """The arrays of a tree read-out as numpy structured arrays (abi.*_dtype): builder (an abi.TREE_* value) and builder_name, num_nodes,
    depth, leaf_references, num_triangles, quantized, num_instances, top_nodes; nodes, nodes_q (None unless quantized), leaf_tris,
    shade_tris, instances, instance_boxes [n, 2, 4] float32 (lo, hi)."""
    def read(what, count, dtype):
        out = np.zeros(count, dtype)
        _check(lib, call(what, out.ctypes.data, out.nbytes // 4), symbol)
        return out
    s = [int(v) for v in read(0, 16, np.uint32)]
    tree = dict(builder=s[0], builder_name=abi.TREE_BUILDERS[s[0]], num_nodes=s[1], depth=s[2], leaf_references=s[3], num_triangles=s[4],
                quantized=bool(s[5]), num_instances=s[6], top_nodes=s[7])
    if summary_only:
        return tree
    tree["nodes"] = read(1, s[1], abi.qnode_dtype)
    tree["nodes_q"] = read(2, s[1], abi.qnodeq_dtype) if s[5] else None
    tree["leaf_tris"] = read(3, s[3], abi.leaftri_dtype)
    tree["shade_tris"] = read(4, s[4], abi.shadetri_dtype)
    tree["instances"] = read(5, s[6], abi.devinstance_dtype)
    tree["instance_boxes"] = read(6, s[6] * 8, np.float32).reshape(s[6], 2, 4)
    return tree


def host_tree(scene, flags=0):
    """Diagnostic (slrhip_debug_host_tree): the tree the host builds for `scene` (an abi.Scene) in an RGB context with config flags
    `flags`, as the dict _read_tree describes.  No GPU is touched; raises SlrHipError (code 5) for a scene whose tree the upload leaves to
    the device build."""
    lib = load_library()
    desc = scene.desc(abi.MODE_RGB)
    return _read_tree(lib, lambda what, ptr, words: lib.slrhip_debug_host_tree(C.byref(desc) if what == 0 else None, flags, what, ptr, words),
                      "slrhip_debug_host_tree")


def quantize_nodes(nodes):
    """Diagnostic (slrhip_debug_quantize_nodes): the host quantizer on abi.qnode_dtype records -> abi.qnodeq_dtype records.  No GPU."""
    lib = load_library()
    a = np.ascontiguousarray(nodes, abi.qnode_dtype)
    out = np.zeros(len(a), abi.qnodeq_dtype)
    _check(lib, lib.slrhip_debug_quantize_nodes(a.ctypes.data, len(a), out.ctypes.data), "slrhip_debug_quantize_nodes")
    return out


def geometry_update_check(have_scene, dynamic, tree_builder, num_instances, num_vertices, device_src, first, count):
    """Diagnostic (slrhip_debug_geometry_update_check): the argument checks of Context.set_vertices without a context; raises SlrHipError
    with the code and the message the call would give.  No GPU."""
    lib = load_library()
    _check(lib, lib.slrhip_debug_geometry_update_check(int(have_scene), int(dynamic), tree_builder, num_instances, num_vertices, device_src, first, count),
           "slrhip_debug_geometry_update_check")


def geometry_update_check2(have_scene, dynamic, instanced_kept, tree_builder, num_instances, num_vertices, device_src, first, count):
    """Diagnostic (slrhip_debug_geometry_update_check2): the same checks for a context that may have been created with
    abi.FLAG_DYNAMIC_INSTANCED as well (instanced_kept) — the ones Context.set_vertices makes; raises SlrHipError with the call's own
    message.  No GPU is touched."""
    lib = load_library()
    _check(lib, lib.slrhip_debug_geometry_update_check2(int(have_scene), int(dynamic), int(instanced_kept), tree_builder, num_instances, num_vertices,
                                                        device_src, first, count), "slrhip_debug_geometry_update_check2")


def materials_update_check(mode, uploaded, geometry_kept, scene, reserved=(0, 0), want_facts=False):
    """slrhip_debug_materials_update_check: the checks of Context.set_materials on the HOST, without a context — the tables of `scene` (an
    abi.Scene, an abi.MaterialsDesc, or None) against a context of `mode` that uploaded `uploaded` (an abi.Scene, or None: no scene) and
    keeps its geometry or not.  Raises SlrHipError as the call would; with want_facts returns [materials, 3] uint32: triangle count, used by
    an instanced triangle, alpha-map texture (0xFFFFFFFF: none)."""
    lib = load_library()
    up = uploaded.desc(mode) if uploaded is not None else None
    d = scene.materials_desc() if isinstance(scene, abi.Scene) else scene
    if isinstance(scene, abi.Scene):
        d.reserved[0], d.reserved[1] = reserved
    facts = np.zeros((len(uploaded.materials) if uploaded is not None else 0, 3), np.uint32)
    _check(lib, lib.slrhip_debug_materials_update_check(mode, C.byref(up) if up is not None else None, int(bool(geometry_kept)),
                                                        C.byref(d) if d is not None else None, facts.ctypes.data if want_facts and facts.size else None,
                                                        facts.size), "slrhip_debug_materials_update_check")
    return facts if want_facts else None


def instance_world_box(mesh_lo, mesh_hi, local_to_world):
    """The world box the top-level tree holds for an instance (slrhip_instance_world_box: the function the upload and the kernel of
    set_instance_transforms call): (lo, hi), float32 [3] each, of the mesh's local box taken through the column-major matrix."""
    lib = load_library()
    lo, hi, m = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (mesh_lo, mesh_hi, local_to_world))
    if len(lo) != 3 or len(hi) != 3 or len(m) != 16:
        raise ValueError("instance_world_box: mesh_lo [3], mesh_hi [3], local_to_world [16] expected")
    out_lo, out_hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    if lib.slrhip_instance_world_box(lo.ctypes.data, hi.ctypes.data, m.ctypes.data, out_lo.ctypes.data, out_hi.ctypes.data) != 0:
        raise ValueError("instance_world_box: refused")
    return out_lo, out_hi


def top_level_key(lo, hi, scene_lo, scene_hi):
    """The sort key of a top-level primitive's box [lo, hi] in the scene box (slrhip_top_level_key: the function the kernels of
    rebuild_top_level call), as a Python int (63 bits)."""
    lib = load_library()
    a = [np.ascontiguousarray(v, np.float32).reshape(-1) for v in (lo, hi, scene_lo, scene_hi)]
    if any(len(v) != 3 for v in a):
        raise ValueError("top_level_key: four [3] arrays expected")
    key = C.c_uint64(0)
    if lib.slrhip_top_level_key(*(v.ctypes.data for v in a), C.byref(key)) != 0:
        raise ValueError("top_level_key: refused")
    return key.value


def _qnode_words(nodes):
    """QNode records (abi.qnode_dtype, or [n, 32] uint32 words) as a fresh contiguous [n, 32] uint32 array."""
    a = np.array(nodes, copy=True, order="C")
    if a.dtype == abi.qnode_dtype:
        a = a.view(np.uint32).reshape(len(a), 32)
    if a.dtype != np.uint32 or a.ndim != 2 or a.shape[1] != 32:
        raise ValueError("nodes: abi.qnode_dtype records or [n, 32] uint32 words expected")
    return a


def top_level_plan(nodes, top_nodes):
    """Diagnostic (slrhip_debug_top_level_plan): (slots, refs) of the first `top_nodes` QNode records — the leaf slots depth-first
    (node * 4 + child) and the primitives' child words ascending, uint32 each.  No GPU; raises SlrHipError for nodes that are no top
    level."""
    lib = load_library()
    a = _qnode_words(nodes)
    slots, refs, count = np.zeros(4 * top_nodes, np.uint32), np.zeros(4 * top_nodes, np.uint32), C.c_uint32(0)
    if top_nodes > len(a):
        raise ValueError("top_level_plan: top_nodes beyond the nodes given")
    _check(lib, lib.slrhip_debug_top_level_plan(a.ctypes.data, top_nodes, slots.ctypes.data, refs.ctypes.data, len(slots), C.byref(count)),
           "slrhip_debug_top_level_plan")
    return slots[:count.value].copy(), refs[:count.value].copy()


def top_level_reseat(nodes, top_nodes, instance_boxes):
    """Diagnostic (slrhip_debug_top_level_reseat): the whole of rebuild_top_level on a host copy of QNode records — (nodes after,
    in the form given; keys [primitives] uint64 by primitive; order [primitives] uint32 by slot).  instance_boxes: [n, 2, 4] float32
    (lo, hi) as debug_top_level()["boxes"] and a tree read-out's "instance_boxes" hold them.  No GPU."""
    lib = load_library()
    a = _qnode_words(nodes)
    boxes = np.ascontiguousarray(instance_boxes, np.float32)
    if boxes.ndim != 3 or boxes.shape[1:] != (2, 4) or top_nodes > len(a):
        raise ValueError("top_level_reseat: instance_boxes [n, 2, 4] and top_nodes <= len(nodes) expected")
    keys, order = np.zeros(4 * top_nodes, np.uint64), np.zeros(4 * top_nodes, np.uint32)
    _check(lib, lib.slrhip_debug_top_level_reseat(a.ctypes.data, top_nodes, boxes.ctypes.data, len(boxes), keys.ctypes.data, order.ctypes.data),
           "slrhip_debug_top_level_reseat")
    n = len(top_level_plan(a, top_nodes)[0])
    out = a.reshape(-1).view(abi.qnode_dtype) if np.asarray(nodes).dtype == abi.qnode_dtype else a
    return out, keys[:n].copy(), order[:n].copy()


def top_level_cost_of(nodes, top_nodes):
    """Diagnostic (slrhip_debug_top_level_cost): Context.top_level_cost()'s value of QNode records on the host.  No GPU."""
    lib = load_library()
    a = _qnode_words(nodes)
    cost = C.c_double(0.0)
    if top_nodes > len(a):
        raise ValueError("top_level_cost_of: top_nodes beyond the nodes given")
    _check(lib, lib.slrhip_debug_top_level_cost(a.ctypes.data, top_nodes, C.byref(cost)), "slrhip_debug_top_level_cost")
    return cost.value


def top_level_rebuild_check(have_scene, num_instances):
    """Diagnostic (slrhip_debug_top_level_rebuild_check): the checks of Context.rebuild_top_level without a context; raises SlrHipError
    with the code and the message the call would give.  No GPU."""
    lib = load_library()
    _check(lib, lib.slrhip_debug_top_level_rebuild_check(int(have_scene), num_instances), "slrhip_debug_top_level_rebuild_check")


def motion_camera(camera):
    """The constants the motion pass takes of an abi.Camera, from the upload's host arithmetic (slrhip_motion_camera): float32 [24] =
    world_to_local [16], the lens centre [3], opWidth, opHeight, objPlaneDistance, 0, 0."""
    lib = load_library()
    out = np.zeros(24, np.float32)
    if lib.slrhip_motion_camera(C.byref(camera), out.ctypes.data) != 0:
        raise ValueError("motion_camera: refused")
    return out


def motion_sample(now_camera, prev_camera, now_record, prev_record, width, height, point):
    """One sample's motion vector on the host, with the function the kernel calls (slrhip_motion_sample): now_record / prev_record
    are the 32 floats of an instance's transform now and in the previous frame (None: a loose triangle / the instance did not move),
    point the hit point now; float32 [4] = {m.x, m.y, z', 1}, or zeros for a sample that is not valid."""
    lib = load_library()
    recs = [None if r is None else np.ascontiguousarray(r, np.float32).reshape(32) for r in (now_record, prev_record)]
    p, out = np.ascontiguousarray(point, np.float32).reshape(3), np.zeros(4, np.float32)
    if lib.slrhip_motion_sample(C.byref(now_camera), C.byref(prev_camera), *(None if r is None else r.ctypes.data for r in recs), width, height,
                                p.ctypes.data, out.ctypes.data) != 0:
        raise ValueError("motion_sample: refused")
    return out


def motion_sample_vertices(now_camera, prev_camera, now_record, prev_record, width, height, now_positions, prev_positions, b1, b2):
    """One sample's motion vector where the vertices moved as well, on the host, with the function the kernel calls
    (slrhip_motion_sample_vertices): the records as for motion_sample; now_positions / prev_positions [3, 3] the positions of the hit
    triangle's vertices now and in the previous frame; b1, b2 the hit's barycentrics; float32 [4] as motion_sample's."""
    lib = load_library()
    recs = [None if r is None else np.ascontiguousarray(r, np.float32).reshape(32) for r in (now_record, prev_record)]
    pn, pp = (np.ascontiguousarray(p, np.float32).reshape(9) for p in (now_positions, prev_positions))
    out = np.zeros(4, np.float32)
    if lib.slrhip_motion_sample_vertices(C.byref(now_camera), C.byref(prev_camera), *(None if r is None else r.ctypes.data for r in recs), width, height,
                                         pn.ctypes.data, pp.ctypes.data, float(b1), float(b2), out.ctypes.data) != 0:
        raise ValueError("motion_sample_vertices: refused")
    return out


def env_importance(texels, mode=abi.MODE_RGB):
    """The importance map of an environment image [H, W, 3] float32 ((r, g, b) for abi.MODE_RGB, (u, v, s) for abi.MODE_SPECTRAL), on
    the host with the functions the kernels of set_environment call (slrhip_env_importance): [H / 4, W / 4] float32 =
    what slrhip_envmap::importance must hold."""
    lib = load_library()
    t = np.ascontiguousarray(texels, np.float32)
    if t.ndim != 3 or t.shape[2] != 3:
        raise ValueError("texels: a [height, width, 3] array expected")
    h, w, _ = t.shape
    out = np.empty((h // 4, w // 4), np.float32)
    if lib.slrhip_env_importance(mode, t.ctypes.data, w, h, out.ctypes.data, out.size) != 0:
        raise ValueError("env_importance: width and height must be multiples of 4 in 4 .. 32768, mode abi.MODE_RGB or abi.MODE_SPECTRAL")
    return out


def env_texels_to_uvs(rgb):
    """(r, g, b) -> (u, v, s) per texel as the reference's spectral build stores an RGB image, binary16-rounded, on the host with
    the function set_environment(rgb=True) calls on the device (slrhip_env_texels_to_uvs): an array of the shape given."""
    lib = load_library()
    t = np.ascontiguousarray(rgb, np.float32)
    if t.ndim < 1 or t.shape[-1] != 3:
        raise ValueError("rgb: an array of [..., 3] expected")
    out = np.empty_like(t)
    if lib.slrhip_env_texels_to_uvs(t.ctypes.data, t.size // 3, out.ctypes.data) != 0:
        raise ValueError("env_texels_to_uvs: bad arguments")
    return out


def clamp_sample(values, limit, flags=0):
    """The sample clamp on one sample of 3 or 16 float32 values, on the host with the function the kernels call
    (slrhip_clamp_sample): (what, values as the sensor receives them, Y as given, Y as received); what = 0 kept, 1 clamped, 2 dropped."""
    lib = load_library()
    v = np.ascontiguousarray(values, np.float32)
    out = np.empty_like(v)
    y_in, y_out = C.c_float(0), C.c_float(0)
    what = lib.slrhip_clamp_sample(v.size, v.ctypes.data, limit, flags, out.ctypes.data, C.byref(y_in), C.byref(y_out))
    if what < 0:
        raise ValueError("clamp_sample: 3 or 16 components")
    return what, out, np.float32(y_in.value), np.float32(y_out.value)
