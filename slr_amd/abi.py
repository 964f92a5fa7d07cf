"""ctypes mirror of include/slrhip.h (the C ABI of the path-tracing hot path).

Only plumbing lives here: struct layouts, library loading and a thin `Context`
wrapper.  The same scene structs are consumed by three implementations of one
interface: the HIP product library (slr_amd/csrc -> libslrhip.so), the CPU oracle
(oracle/ -> libslr_oracle.so, tests/bench only) and, when built in the container
that has /root/reference, the compiled reference itself (oracle/_ref).
"""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MODE_RGB, MODE_SPECTRAL = 0, 1
MAT_MATTE, MAT_METAL, MAT_GLASS, MAT_MF_METAL, MAT_MF_GLASS, MAT_WARD, MAT_ASHIKHMIN, MAT_MULTI = 0, 1, 2, 3, 4, 5, 6, 7
MULTI_INVERSE_0, MULTI_INVERSE_1 = 1, 2
SPEC_RGB_ONLY, SPEC_UPSAMPLED, SPEC_REGULAR, SPEC_IRREGULAR = 0, 1, 2, 3

# numpy dtypes with the exact layout of the C structs (checked in tests/test_abi.py)
vertex_dtype = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("tangent", "<f4", 3),
                         ("texcoord", "<f4", 2)])
triangle_dtype = np.dtype([("v", "<u4", 3), ("material", "<u4")])
material_dtype = np.dtype([("type", "<u4"), ("spectrum", "<i4", 3), ("param", "<f4"), ("emittance", "<i4"), ("param2", "<f4"), ("reserved", "<u4")])
spectrum_dtype = np.dtype([("kind", "<u4"), ("rgb", "<f4", 3), ("u", "<f4"), ("v", "<f4"), ("scale", "<f4"),
                           ("lambda_min", "<f4"), ("lambda_max", "<f4"), ("num_samples", "<u4"),
                           ("data_offset", "<u4"), ("reserved", "<u4")])


texture_dtype = np.dtype([("kind", "<u4"), ("offset", "<f4", 2), ("scale", "<f4", 2), ("spectrum", "<i4", 2), ("value", "<f4", 2),
                          ("reserved", "<u4", 3)])
instance_dtype = np.dtype([("first_triangle", "<u4"), ("num_triangles", "<u4"), ("local_to_world", "<f4", 16), ("world_to_local", "<f4", 16)])
# slrhip_set_instance_transforms: one 128-byte slrhip_instance_transform per moved instance (a [n, 32] float32 array has the same bytes)
instance_transform_dtype = np.dtype([("local_to_world", "<f4", 16), ("world_to_local", "<f4", 16)])
# the tree read-outs (slrhip_debug_tree / slrhip_debug_host_tree / slrhip_debug_quantize_nodes): the records of slr_amd/csrc/device_types.h.
# lo / hi are [axis][child]; qlo / qhi one byte per child; a leaf reference is LEAF_FLAG | count << 27 | first LeafTri (count 0: an instance)
qnode_dtype = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("child", "<u4", 4), ("pad", "<u4", 4)])
qnodeq_dtype = np.dtype([("origin", "<f4", 3), ("scale", "<f4", 3), ("qlo", "u1", (3, 4)), ("qhi", "u1", (3, 4)), ("child", "<u4", 4)])
leaftri_dtype = np.dtype([("v0", "<f4", 3), ("tri", "<u4"), ("e1", "<f4", 3), ("alpha", "<u4"), ("e2", "<f4", 3), ("pad", "<u4")])
shadetri_dtype = np.dtype([("n0", "<f4", 3), ("material", "<u4"), ("n1", "<f4", 3), ("light", "<i4"), ("n2", "<f4", 3), ("area_pdf", "<f4"),
                           ("t0", "<f4", 3), ("gnx", "<f4"), ("t1", "<f4", 3), ("gny", "<f4"), ("t2", "<f4", 3), ("gnz", "<f4")])
devinstance_dtype = np.dtype([("local_to_world", "<f4", 16), ("world_to_local", "<f4", 16), ("root", "<u4"), ("first_triangle", "<u4"),
                              ("num_triangles", "<u4"), ("mesh", "<u4")])
INVALID_CHILD, LEAF_FLAG, LEAF_COUNT_SHIFT, LEAF_INDEX_MASK, MAX_LEAF_TRIS = 0xFFFFFFFF, 0x80000000, 27, (1 << 27) - 1, 4
TREE_HOST_SAH, TREE_HOST_SPATIAL_SPLITS, TREE_DEVICE, TREE_INSTANCED = 0, 1, 2, 3
TOP_SEAT_GROUP = 4096          # SLRHIP_TOP_SEAT_GROUP: the most top-level primitives slrhip_rebuild_top_level sorts in one workgroup
TREE_BUILDERS = ("host SAH", "host spatial splits", "device", "instanced")
INSTANCE_BAD_TRANSFORM = 1     # slrhip_instances_status: a record was not finite or not affine; its instance did not move
GEOMETRY_BAD_VERTEX = 1        # slrhip_geometry_status: a record of set_vertices had a non-finite float; its vertex did not move
TEX_CHECKER_SPECTRUM, TEX_CHECKER_FLOAT, TEX_CHECKER_NORMAL, TEX_IMAGE_SPECTRUM = 0, 1, 2, 3
# ray queries on device memory (slrhip_intersect_rays / slrhip_test_visibility): one [n, 8] float32 row per slrhip_ray, one [n, 4]
# row per slrhip_hit (column 0 holds the triangle index's bits)
ray_dtype = np.dtype([("org", "<f4", 3), ("dist_min", "<f4"), ("dir", "<f4", 3), ("dist_max", "<f4")])
hit_dtype = np.dtype([("triangle", "<u4"), ("dist", "<f4"), ("b0", "<f4"), ("b1", "<f4")])
MISS = 0xFFFFFFFF
# bits of the query error word (slrhip_query_status)
QUERY_ERR_RING_SPACE, QUERY_ERR_RING_RELEASE, QUERY_ERR_CONSUMER_IDLE, QUERY_ERR_STACK_OVERFLOW = 1, 2, 4, 8
# first-hit feature buffers (slrhip_render_features): channel bits, and per channel (file / npz name, components, numpy dtype)
FEATURE_GEOMETRIC_NORMAL, FEATURE_SHADING_NORMAL, FEATURE_SHADING_TANGENT, FEATURE_DISTANCE, FEATURE_COVERAGE, FEATURE_IDS = 1, 2, 4, 8, 16, 32
FEATURE_ALL = 63
FEATURE_CHANNELS = {FEATURE_GEOMETRIC_NORMAL: ("geometric_normal", 3, np.float32), FEATURE_SHADING_NORMAL: ("shading_normal", 3, np.float32),
                    FEATURE_SHADING_TANGENT: ("shading_tangent", 3, np.float32), FEATURE_DISTANCE: ("distance", 1, np.float32),
                    FEATURE_COVERAGE: ("coverage", 1, np.float32), FEATURE_IDS: ("ids", 3, np.uint32)}
# per-pixel noise statistics (slrhip_statistics_begin): channel bits -> file / npz name; the metrics of slrhip_render_until
STATISTICS_MEAN, STATISTICS_VARIANCE, STATISTICS_VARIANCE_OF_MEAN, STATISTICS_COUNT, STATISTICS_MAX = 1, 2, 4, 8, 16
STATISTICS_ALL = 31
STATISTICS_CHANNELS = {STATISTICS_MEAN: "mean", STATISTICS_VARIANCE: "variance", STATISTICS_VARIANCE_OF_MEAN: "variance_of_mean",
                       STATISTICS_COUNT: "count", STATISTICS_MAX: "max"}
NOISE_RMSE, NOISE_RELATIVE = 0, 1
NOISE_METRICS = {"rmse": NOISE_RMSE, "relative": NOISE_RELATIVE}


def texture_ref(t):
    """SLRHIP_TEXTURE_REF: the value of a material's spectrum slot that names texture t."""
    return -2 - int(t)


class Camera(C.Structure):
    _fields_ = [("local_to_world", C.c_float * 16), ("world_to_local", C.c_float * 16),
                ("aspect", C.c_float), ("fov_y", C.c_float), ("lens_radius", C.c_float),
                ("img_plane_distance", C.c_float), ("obj_plane_distance", C.c_float),
                ("sensitivity", C.c_float)]


class Ray(C.Structure):
    _fields_ = [("org", C.c_float * 3), ("dist_min", C.c_float), ("dir", C.c_float * 3), ("dist_max", C.c_float)]


class Hit(C.Structure):
    _fields_ = [("triangle", C.c_uint32), ("dist", C.c_float), ("b0", C.c_float), ("b1", C.c_float)]


class EnvMap(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("texels", C.c_void_p), ("scale", C.c_float),
                ("map_width", C.c_uint32), ("map_height", C.c_uint32), ("importance", C.c_void_p)]


class UpsamplingTables(C.Structure):
    _fields_ = [("grid_width", C.c_uint32), ("grid_height", C.c_uint32), ("cells", C.c_void_p), ("num_points", C.c_uint32),
                ("point_uv", C.c_void_p), ("point_spectrum", C.c_void_p)]


class SceneDesc(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("num_vertices", C.c_uint32),
                ("triangles", C.c_void_p), ("num_triangles", C.c_uint32),
                ("materials", C.c_void_p), ("num_materials", C.c_uint32),
                ("spectra", C.c_void_p), ("num_spectra", C.c_uint32),
                ("spectrum_data", C.c_void_p), ("num_spectrum_data", C.c_uint32),
                ("camera", Camera),
                ("env", C.POINTER(EnvMap)),
                ("upsampling", C.POINTER(UpsamplingTables)),
                ("textures", C.c_void_p), ("num_textures", C.c_uint32),
                ("texture_texels", C.c_void_p), ("num_texture_texels", C.c_uint32),
                ("instances", C.c_void_p), ("num_instances", C.c_uint32)]


class RenderSettings(C.Structure):
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("time_start", C.c_float),
                ("time_end", C.c_float), ("brightness", C.c_float), ("rng_seed", C.c_int32)]


class Shard(C.Structure):
    _fields_ = [("shard_index", C.c_uint32), ("shard_count", C.c_uint32)]


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("mode", C.c_int32), ("stripes", C.c_uint32), ("flags", C.c_uint32)]


class Counters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("extension_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
                ("iterations", C.c_uint64), ("bvh_nodes", C.c_uint64), ("bvh_depth", C.c_uint64),
                ("build_seconds", C.c_double), ("bvh_leaf_references", C.c_uint64)]


class Profile(C.Structure):
    _fields_ = [("launches", C.c_uint64 * 3), ("milliseconds", C.c_double * 3), ("rays", C.c_uint64 * 2),
                ("nodes", C.c_uint64 * 2), ("triangles", C.c_uint64 * 2), ("slot_visits", C.c_uint64)]


class StatisticsSummary(C.Structure):
    _fields_ = [("pixels", C.c_uint64), ("samples", C.c_uint64), ("sum_mean", C.c_double), ("sum_mean_sq", C.c_double),
                ("sum_variance_of_mean", C.c_double), ("max_sample", C.c_float), ("reserved", C.c_uint32)]


# the sample clamp (slrhip_clamp_begin): the flag, the record channels -> npz name
CLAMP_DROP_NONFINITE = 1
CLAMP_CLAMPED, CLAMP_DROPPED, CLAMP_REMOVED, CLAMP_LARGEST = 1, 2, 4, 8
CLAMP_ALL = 15
CLAMP_CHANNELS = {CLAMP_CLAMPED: "clamped", CLAMP_DROPPED: "dropped", CLAMP_REMOVED: "removed", CLAMP_LARGEST: "largest"}


class ClampDesc(C.Structure):
    _fields_ = [("limit", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class ClampSummary(C.Structure):
    _fields_ = [("clamped", C.c_uint64), ("dropped", C.c_uint64), ("removed", C.c_double), ("largest", C.c_float), ("reserved", C.c_uint32)]


class NoiseTarget(C.Structure):
    _fields_ = [("metric", C.c_uint32), ("target", C.c_float), ("spp_step", C.c_uint32), ("spp_max", C.c_uint32)]


class AdaptiveTarget(C.Structure):
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("spp_min", C.c_uint32), ("spp_step", C.c_uint32), ("spp_max", C.c_uint32)]


class DenoiseDesc(C.Structure):
    """slrhip_denoise_desc: every pointer is a DEVICE pointer (an integer address, or None)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_uint32), ("iterations", C.c_uint32),
                ("color", C.c_void_p), ("variance", C.c_void_p), ("normal", C.c_void_p), ("distance", C.c_void_p), ("coverage", C.c_void_p),
                ("output", C.c_void_p), ("output_variance", C.c_void_p),
                ("sigma_luminance", C.c_float), ("sigma_distance", C.c_float), ("normal_power_log2", C.c_uint32), ("reserved", C.c_uint32)]


# slrhip_tonemap's image formats (SLRHIP_IMAGE_*)
IMAGE_BGR8_BMP = 0      # bottom-up rows of 3 * w + w % 4 bytes, B G R, padding 0: what slrhip_tonemap_bgr8 fills and slrhip_save_bmp takes
IMAGE_RGBA8 = 1         # top-down rows of 4 * w bytes, R G B 255


class TonemapDesc(C.Structure):
    """slrhip_tonemap_desc: color and output are DEVICE pointers (integer addresses)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_uint32), ("format", C.c_uint32),
                ("color", C.c_void_p), ("output", C.c_void_p), ("output_bytes", C.c_size_t), ("scale", C.c_float), ("reserved", C.c_uint32)]


# slrhip_modulate's operations (SLRHIP_MODULATE_*)
MODULATE_DIVIDE, MODULATE_MULTIPLY = 0, 1
# Context.modulate's default floor: the smallest mean albedo a pixel is divided by (a black texel, a NaN)
MODULATE_FLOOR = 1e-3


class ModulateDesc(C.Structure):
    """slrhip_modulate_desc: every pointer is a DEVICE pointer (an integer address, or None)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_uint32), ("op", C.c_uint32),
                ("color", C.c_void_p), ("variance", C.c_void_p), ("albedo", C.c_void_p), ("output", C.c_void_p), ("output_variance", C.c_void_p),
                ("albedo_passes", C.c_uint32), ("floor", C.c_float), ("reserved", C.c_uint32)]


class MotionDesc(C.Structure):
    """slrhip_motion_desc: previous_camera is a HOST pointer (None: the camera did not move), previous_transforms a DEVICE pointer (an
    integer address; None: no instance moved) to one 128-byte record per instance of the scene."""
    _fields_ = [("previous_camera", C.POINTER(Camera)), ("previous_transforms", C.c_void_p), ("reserved", C.c_uint32 * 2)]


class MotionVerticesDesc(C.Structure):
    """slrhip_motion_vertices_desc: `frame` as for slrhip_render_motion; previous_vertices a DEVICE pointer (an integer address; None: no
    vertex moved) to ALL slrhip_vertex records of the scene as the previous frame had them."""
    _fields_ = [("frame", MotionDesc), ("previous_vertices", C.c_void_p), ("reserved", C.c_uint64)]


# Context.reproject's defaults: the history is capped at 32 frames; a tap is taken if its distance is within 10 % of the expected one
# and its normal within about 25 degrees of the pixel's
REPROJECT_MAX_HISTORY, REPROJECT_SIGMA_DISTANCE, REPROJECT_MIN_NORMAL_DOT = 32.0, 0.1, 0.9


class ReprojectDesc(C.Structure):
    """slrhip_reproject_desc: every pointer is a DEVICE pointer (an integer address, or None)."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("components", C.c_uint32),
                ("color", C.c_void_p), ("variance", C.c_void_p), ("motion", C.c_void_p), ("coverage", C.c_void_p), ("ids", C.c_void_p),
                ("normal", C.c_void_p),
                ("prev_color", C.c_void_p), ("prev_variance", C.c_void_p), ("prev_length", C.c_void_p), ("prev_distance", C.c_void_p),
                ("prev_coverage", C.c_void_p), ("prev_ids", C.c_void_p), ("prev_normal", C.c_void_p),
                ("output", C.c_void_p), ("output_variance", C.c_void_p), ("output_length", C.c_void_p),
                ("max_history", C.c_float), ("min_alpha", C.c_float), ("sigma_distance", C.c_float), ("min_normal_dot", C.c_float),
                ("reserved", C.c_uint32 * 2)]


# slrhip_set_environment's flags (SLRHIP_ENV_*)
ENV_TEXELS_RGB = 1      # the texels are linear (r, g, b): a spectral context converts them per texel to (u, v, s); an RGB context ignores it
ENV_STORE_HALF = 2      # round every component to binary16 first, as the reference's RGBA16F image holds them


class EnvironmentDesc(C.Structure):
    """slrhip_environment_desc: texels is a DEVICE pointer (an integer address), [height][width][3] float32, 16-byte aligned."""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("texels", C.c_void_p), ("scale", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


# slrhip_set_texture_texels' flag (SLRHIP_TEXELS_*)
TEXELS_STORE_HALF = 1   # round every float to binary16 first


class MaterialsDesc(C.Structure):
    """slrhip_materials_desc: the four tables of slrhip_set_materials, HOST pointers, typed and counted as SceneDesc's fields of the same names."""
    _fields_ = [("materials", C.c_void_p), ("num_materials", C.c_uint32),
                ("spectra", C.c_void_p), ("num_spectra", C.c_uint32),
                ("spectrum_data", C.c_void_p), ("num_spectrum_data", C.c_uint32),
                ("textures", C.c_void_p), ("num_textures", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


# Context.denoise's default sigma_distance: the accepted relative change of the camera distance per pixel of tap offset
# (DESIGN.md records how it was picked on the Cornell scenes)
DENOISE_SIGMA_DISTANCE = 0.1


def noise_metric(summary, metric=NOISE_RMSE):
    """The stop check of slrhip_render_until on a statistics summary (a dict of Context.statistics_summary, or the sum of
    several shards' dicts): NOISE_RMSE = sqrt(sum_variance_of_mean / pixels), NOISE_RELATIVE = that over the mean luminance."""
    if summary["pixels"] == 0:
        return 0.0
    rmse = float(np.sqrt(np.float64(summary["sum_variance_of_mean"]) / np.float64(summary["pixels"])))
    if metric == NOISE_RMSE:
        return rmse
    mean = float(np.float64(summary["sum_mean"]) / np.float64(summary["pixels"]))
    return float("inf") if mean == 0.0 else rmse / mean


FLAG_TIME_KERNELS, FLAG_COUNT_TRAVERSAL, FLAG_BVH_DEVICE_BUILD, FLAG_TEST_DEVICE_ERROR, FLAG_BVH_SPATIAL_SPLITS, FLAG_TAIL_KERNEL = 1, 2, 4, 16, 64, 128
FLAG_NO_PRIMARY_PASS = 256      # the primary pass (camera rays traced before a window's iterations) is on by default; this turns it off
FLAG_DYNAMIC_GEOMETRY = 512     # keep the vertex and index arrays on the device, so that Context.set_vertices can move vertices without an upload
FLAG_DYNAMIC_INSTANCED = 1024   # with FLAG_DYNAMIC_GEOMETRY: also for scenes with instances (the mesh trees' level list and roots are kept as well)
FLAG_PRIMARY_RING = 2048        # keep the primary pass on the ring kernel where it would run the direct kernel (same frame; the tests' comparator)
FLAG_TRACE_ALL_SHADOW_RAYS = 4096  # trace the light samples that decide nothing as well (same frame, same counters; the tests' comparator)
MAX_STRIPES = 64
KERNEL_NAMES = ("trace", "shade", "tail")

DEFAULT_SEED = 1509761209  # libSLRSceneGraph/API.cpp:1080


class Scene:
    """Flat scene (numpy arrays) + the ctypes view handed across the ABI."""

    def __init__(self, vertices, triangles, materials, spectra, spectrum_data, camera, env=None, name="scene", textures=None,
                 texture_texels=None, texture_texels_uvs=None, instances=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=vertex_dtype)
        self.triangles = np.ascontiguousarray(triangles, dtype=triangle_dtype)
        mats = np.asarray(materials)
        if mats.dtype != material_dtype:           # e.g. fixtures written before param2 existed: copy the common fields
            conv = np.zeros(len(mats), dtype=material_dtype)
            for name in mats.dtype.names:
                conv[name] = mats[name]
            mats = conv
        self.materials = np.ascontiguousarray(mats, dtype=material_dtype)
        self.spectra = np.ascontiguousarray(spectra, dtype=spectrum_dtype)
        self.spectrum_data = np.ascontiguousarray(spectrum_data, dtype=np.float32)
        self.camera = camera
        self.textures = np.ascontiguousarray(textures if textures is not None else np.zeros(0, texture_dtype), dtype=texture_dtype)
        self.instances = np.ascontiguousarray(instances if instances is not None else np.zeros(0, instance_dtype), dtype=instance_dtype)
        # texels of the image textures (TEX_IMAGE_SPECTRUM): [n][3] as the RGB build stores them, and as (u, v, s) for the spectral build
        self.texture_texels = np.ascontiguousarray(texture_texels if texture_texels is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3)
        self.texture_texels_uvs = np.ascontiguousarray(texture_texels_uvs if texture_texels_uvs is not None else np.zeros((0, 3)), dtype=np.float32).reshape(-1, 3)
        self.env_texels = None
        self.env = None
        self.env_uvs = None
        self._tables = None
        if env is not None:
            # (texels rgb, scale, importance) or, for both modes, (texels rgb, scale, importance rgb, texels uvs, importance uvs)
            texels, scale, importance = env[:3]
            self.env_texels = np.ascontiguousarray(texels, dtype=np.float32)
            self.env_importance = np.ascontiguousarray(importance, dtype=np.float32)
            self.env_scale = float(scale)
            self.env = EnvMap(self.env_texels.shape[1], self.env_texels.shape[0], self.env_texels.ctypes.data, float(scale),
                              self.env_importance.shape[1], self.env_importance.shape[0], self.env_importance.ctypes.data)
            if len(env) == 5:
                self.env_texels_uvs = np.ascontiguousarray(env[3], dtype=np.float32)
                self.env_importance_uvs = np.ascontiguousarray(env[4], dtype=np.float32)
                self.env_uvs = EnvMap(self.env_texels_uvs.shape[1], self.env_texels_uvs.shape[0], self.env_texels_uvs.ctypes.data, float(scale),
                                      self.env_importance_uvs.shape[1], self.env_importance_uvs.shape[0], self.env_importance_uvs.ctypes.data)
        self.name = name
        self._validate()

    def _validate(self):
        nv, nm, ns = len(self.vertices), len(self.materials), len(self.spectra)
        if len(self.triangles) == 0:
            raise ValueError("scene has no triangles")
        if self.env is not None and (self.env_texels.ndim != 3 or self.env_texels.shape[2] != 3):
            raise ValueError("environment texels must be [height][width][3]")
        if self.triangles["v"].max() >= nv:
            raise ValueError("triangle references a vertex out of range")
        if self.triangles["material"].max() >= nm:
            raise ValueError("triangle references a material out of range")
        single = self.materials["type"] != MAT_MULTI      # a MULTI record's spectrum[] holds component material indices (checked by the library)
        if (single.any() and self.materials["spectrum"][single].max() >= ns) or self.materials["emittance"].max() >= ns:
            raise ValueError("material references a spectrum out of range")
        nt = len(self.textures)
        if single.any() and self.materials["spectrum"][single].min() < -1 - nt:
            raise ValueError("material references a texture out of range")
        if nt and (self.textures["spectrum"][self.textures["kind"] == TEX_CHECKER_SPECTRUM].max(initial=-1) >= ns):
            raise ValueError("texture references a spectrum out of range")

    def upsampling_tables(self):
        if self._tables is None:
            from . import spectra
            t = spectra.tables()
            cells = np.zeros((len(t["grid_inside"]), 8), np.uint8)
            cells[:, 0], cells[:, 1], cells[:, 2:8] = t["grid_inside"], t["grid_num_points"], t["grid_idx"]
            self._table_arrays = (np.ascontiguousarray(cells), np.ascontiguousarray(t["point_uv"], np.float32),
                                  np.ascontiguousarray(t["point_spectrum"], np.float32))
            self._tables = UpsamplingTables(spectra.GRID_WIDTH, spectra.GRID_HEIGHT, self._table_arrays[0].ctypes.data, len(self._table_arrays[1]),
                                            self._table_arrays[1].ctypes.data, self._table_arrays[2].ctypes.data)
        return self._tables

    def desc(self, mode=MODE_RGB, upsampling=False):
        """The ctypes descriptor.  upsampling=True names the Meng-15 tables in spectral mode even if the scene does not need them
        yet: Context.set_environment can then give it an environment."""
        d = SceneDesc()
        d.vertices, d.num_vertices = self.vertices.ctypes.data, len(self.vertices)
        d.triangles, d.num_triangles = self.triangles.ctypes.data, len(self.triangles)
        d.materials, d.num_materials = self.materials.ctypes.data, len(self.materials)
        d.spectra, d.num_spectra = self.spectra.ctypes.data, len(self.spectra)
        d.spectrum_data, d.num_spectrum_data = self.spectrum_data.ctypes.data, len(self.spectrum_data)
        d.camera = self.camera
        env = self.env_uvs if (mode == MODE_SPECTRAL and self.env_uvs is not None) else self.env
        d.env = C.pointer(env) if env is not None else None
        texels = self.texture_texels_uvs if mode == MODE_SPECTRAL else self.texture_texels
        d.upsampling = C.pointer(self.upsampling_tables()) if ((env is not None or len(texels) or upsampling) and mode == MODE_SPECTRAL) else None
        d.textures, d.num_textures = (self.textures.ctypes.data if len(self.textures) else None), len(self.textures)
        d.texture_texels, d.num_texture_texels = (texels.ctypes.data if len(texels) else None), len(texels)
        d.instances, d.num_instances = (self.instances.ctypes.data if len(self.instances) else None), len(self.instances)
        return d

    def materials_desc(self):
        """The ctypes descriptor of slrhip_set_materials: this scene's material, spectrum and texture tables."""
        d = MaterialsDesc()
        d.materials, d.num_materials = self.materials.ctypes.data, len(self.materials)
        d.spectra, d.num_spectra = self.spectra.ctypes.data, len(self.spectra)
        d.spectrum_data, d.num_spectrum_data = self.spectrum_data.ctypes.data, len(self.spectrum_data)
        d.textures, d.num_textures = (self.textures.ctypes.data if len(self.textures) else None), len(self.textures)
        return d


def sample_seed(rng_seed, px, py, sample):
    """Python restatement of slrhip_sample_seed (the per-(pixel,sample) seeding contract)."""
    def fmix(h):
        h &= 0xFFFFFFFF
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        return h
    h = rng_seed & 0xFFFFFFFF
    h = fmix(h ^ ((sample * 0x9E3779B1) & 0xFFFFFFFF))
    h = fmix(h ^ ((py * 0x85EBCA77 + 0x165667B1) & 0xFFFFFFFF))
    h = fmix(h ^ ((px * 0xC2B2AE3D + 0x27D4EB2F) & 0xFFFFFFFF))
    return h - (1 << 32) if h & 0x80000000 else h
