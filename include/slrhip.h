/*
 * slrhip.h — C ABI of the MI355X-native unidirectional path-tracing integrator.
 *
 * This is the drop-in boundary for ONE hot path of goofoo/SLR:
 *     SLR::PathTracingRenderer::render(const Scene&, const RenderSettings&) const
 *     (reference: libSLR/Renderers/PathTracingRenderer.cpp:27-98, entered from
 *      HostProgram/main.cpp:59 through the Renderer vtable libSLR/Core/Renderer.h:15-19).
 *
 * The reference's Scene is an opaque pointer graph with no accessor for its nodes,
 * triangles or materials (libSLR/Core/SurfaceObject.h:187-204,239-260), so the host
 * layer owns a FLAT scene description and hands it across this ABI.  Every struct
 * below names the reference type it flattens.  Plain pointers and sizes only; no
 * C++ or torch types; every entry point returns an int status (0 = OK) and never
 * throws.  One context per GPU; a context is single-caller (not re-entrant), like
 * the reference's render() (PathTracingRenderer.cpp:27, called once from main).
 */
#ifndef SLRHIP_H
#define SLRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLRHIP_VERSION 7   /* 2: slrhip_material::param2, slrhip_scene_desc::upsampling, Ward / Ashikhmin lobes;
                            * 3: SLRHIP_MATERIAL_MULTI, slrhip_bsdf_queries (additive: version-2 callers are unaffected);
                            * 4: stripes > 64 rejected, device error word, samples counted on the device (additive);
                            * 5: slrhip_texture (checkerboard textures, bump, alpha), appended to slrhip_scene_desc; host spectrum
                            *    construction; slrhip_reduce_framebuffer;
                            * 6: SLRHIP_KERNEL_TAIL (slrhip_profile grows by one kernel class), SLRHIP_FLAG_TAIL_KERNEL;
                            * 7: the measured-slower traversal / shading schedules, their flags and the measurement exports are gone
                            *    (TRACE_BATCH, TRACE_POOL, SPECTRAL_QUAD, QUAD_LAYOUT, slrhip_trace_rays_timed, slrhip_debug_read_rays);
                            *    kernel classes of slrhip_profile = {TRACE, SHADE, TAIL}: a wavefront iteration is two launches;
                            *    slrhip_bsdf_queries moved to slrhip_debug.h.  The number is frozen here: later additions append.
                            *    Appended since: SLRHIP_FLAG_NO_PRIMARY_PASS (bit 8; the primary pass is on by default),
                            *    SLRHIP_FLAG_PRIMARY_RING (bit 11), SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS (bit 12).                      */

/* ---- status codes -------------------------------------------------------------- */
enum {
    SLRHIP_OK = 0,
    SLRHIP_ERR_INVALID_ARGUMENT = 1,
    SLRHIP_ERR_NO_DEVICE = 2,      /* no HIP device / HIP runtime failure at create      */
    SLRHIP_ERR_HIP = 3,            /* a HIP call failed; see slrhip_last_error_string    */
    SLRHIP_ERR_NO_SCENE = 4,       /* render before upload_scene                         */
    SLRHIP_ERR_UNSUPPORTED = 5,    /* scene uses a feature outside the hot path          */
    SLRHIP_ERR_OUT_OF_MEMORY = 6
};

/* ---- colour representation ------------------------------------------------------- */
/* The reference selects RGB vs 16-sample spectral rendering at COMPILE time
 * (libSLR/defines.h:160 -> typedefs in libSLR/references.h:39-59).  Here it is a
 * per-context run-time mode.                                                         */
enum {
    SLRHIP_MODE_RGB = 0,           /* SampledSpectrum = RGBTemplate<float>, 3 components  */
    SLRHIP_MODE_SPECTRAL = 1       /* SampledSpectrumTemplate<float,16>, 16-bin storage   */
};
#define SLRHIP_RGB_COMPONENTS 3
#define SLRHIP_SPECTRAL_COMPONENTS 16   /* NumSpectralSamples / NumStrataForStorage, references.h:39-40 */

/* ---- geometry -------------------------------------------------------------------- */
/* SLR::Vertex, libSLR/Core/geometry.h:147-155 (44 bytes, same field order). */
typedef struct slrhip_vertex {
    float position[3];
    float normal[3];
    float tangent[3];
    float texcoord[2];
} slrhip_vertex;

/* One SLR::Triangle (libSLR/Surface/TriangleMesh.h:16-36) wrapped in its
 * SingleSurfaceObject (libSLR/Core/SurfaceObject.h:115-153): three vertex indices and
 * the material of the owning object.  The order of this array is the order in which
 * the reference would receive the objects (it defines light indices and the tie-break
 * among equal-distance hits).                                          */
typedef struct slrhip_triangle {
    uint32_t v[3];
    uint32_t material;
} slrhip_triangle;

/* ---- spectra --------------------------------------------------------------------- */
/* A scene-constant input spectrum (reference InputSpectrum, references.h:51,57).
 * RGB mode reads only `rgb` (RGBTemplate, libSLR/BasicTypes/RGBTypes.h:51-143).
 * Spectral mode evaluates at the path's wavelengths per hit like
 * ConstantSpectrumTexture::evaluate (libSLR/Textures/constant_textures.h:16-31):
 *   kind UPSAMPLED : UpsampledContinuousSpectrum(u, v, scale)  SpectrumTypes.h:180-339
 *   kind REGULAR   : RegularContinuousSpectrum(min,max,values) SpectrumTypes.h:70-118
 *   kind IRREGULAR : IrregularContinuousSpectrum(lambdas,values) SpectrumTypes.h:121-170
 * Sample tables live in slrhip_scene_desc::spectrum_data at [data_offset, +num_samples)
 * (IRREGULAR: num_samples wavelengths followed by num_samples values).
 * UPSAMPLED: the grid-cell lookup of evaluate() (SpectrumTypes.h:241-312) depends only on
 * (u, v), so the caller resolves it once: `reserved` = number of data points (0 = outside
 * the grid, 3 or 4), and the payload at data_offset (a multiple of 4 floats) is 4
 * interpolation weights followed by num_samples (= 95) records of 4 floats: the samples of
 * the data-point spectra interleaved per wavelength bin, [bin][point] (unused points 0).
 * slr_amd/spectra.py:resolve_upsampled builds it.                                       */
enum {
    SLRHIP_SPECTRUM_RGB_ONLY = 0,
    SLRHIP_SPECTRUM_UPSAMPLED = 1,
    SLRHIP_SPECTRUM_REGULAR = 2,
    SLRHIP_SPECTRUM_IRREGULAR = 3
};
typedef struct slrhip_spectrum {
    uint32_t kind;
    float rgb[3];
    float u, v, scale;          /* UPSAMPLED */
    float lambda_min, lambda_max; /* REGULAR */
    uint32_t num_samples;
    uint32_t data_offset;
    uint32_t reserved;
} slrhip_spectrum;

/* ---- materials ------------------------------------------------------------------- */
/* Material -> BSDF factories evaluated per hit in the reference
 * (SurfacePoint::createBSDF, libSLR/Core/geometry.cpp:56-58).                        */
enum {
    /* DiffuseReflection basic_SurfaceMaterials.cpp:15-25: sigma < 0 -> LambertianBRDF
     * (basic_BSDFs.cpp:12-57), sigma >= 0 -> OrenNayerBRDF (OrenNayerBRDF.cpp:12-73).
     * spectrum[0] = reflectance, param = sigma.                                       */
    SLRHIP_MATERIAL_MATTE = 0,
    /* SpecularReflection basic_SurfaceMaterials.cpp:29-34 -> SpecularBRDF + FresnelConductor.
     * spectrum = {coeffR, eta, k}.                                                    */
    SLRHIP_MATERIAL_METAL = 1,
    /* SpecularScattering basic_SurfaceMaterials.cpp:38-43 -> SpecularBSDF + FresnelDielectric.
     * spectrum = {coeff, etaExt, etaInt}.                                             */
    SLRHIP_MATERIAL_GLASS = 2,
    /* MicrofacetReflection MicrofacetSurfaceMaterial.cpp:14-19 -> MicrofacetBRDF(GGX, conductor).
     * spectrum = {-, eta, k}, param = alpha_g.                                        */
    SLRHIP_MATERIAL_MICROFACET_METAL = 3,
    /* MicrofacetScattering MicrofacetSurfaceMaterial.cpp:23-28 -> MicrofacetBSDF(GGX, dielectric).
     * spectrum = {-, etaExt, etaInt}, param = alpha_g.                                */
    SLRHIP_MATERIAL_MICROFACET_GLASS = 4,
    /* ModifiedWardDurReflection SurfaceMaterials/ModifiedWardDurReflection.cpp:14-19 -> ModifiedWardDurBRDF
     * (BSDFs/ModifiedWardDurBRDF.cpp:11-87).  spectrum = {R, -, -}, param = anisoX, param2 = anisoY.        */
    SLRHIP_MATERIAL_WARD = 5,
    /* AshikhminShirleyReflection SurfaceMaterials/AshikhminShirleyReflection.cpp:14-20 -> AshikhminShirleyBRDF
     * (BSDFs/AshikhminShirleyBRDF.cpp:12-170).  spectrum = {Rs, Rd, -}, param = nu, param2 = nv.            */
    SLRHIP_MATERIAL_ASHIKHMIN = 6,
    /* SummedSurfaceMaterial / MixedSurfaceMaterial (SurfaceMaterials/SummedSurfaceMaterial.cpp:13-20,
     * MixedSurfaceMaterial.cpp:14-22) -> MultiBSDF (BSDFs/MultiBSDF.cpp:12-217) over two component BSDFs, either
     * of which may be wrapped in InverseBSDF (InverseSurfaceMaterial basic_SurfaceMaterials.cpp:47-50,
     * basic_BSDFs.cpp:172-203).
     *   spectrum[0], spectrum[1] = indices of the two component MATERIALS: earlier entries of the material
     *                              table; single-lobe types, or MULTI records whose own components are
     *                              single lobes (one level of nesting = up to four lobes, MultiBSDF.h:17:
     *                              sum(mix(a, b), c), mix(sum(a, b), sum(c, d)), ...); their emittance is ignored
     *   spectrum[2]              = SLRHIP_MULTI_INVERSE_0 | SLRHIP_MULTI_INVERSE_1 bits
     *   param, param2            = the `scale` each component's getBSDF receives: 1, 1 for "sum";
     *                              1 - f, f for "mix" with a constant factor f
     * InverseBSDF is limited to single lobes of the reflection-only types (MATTE, METAL, MICROFACET_METAL, WARD, ASHIKHMIN):
     * the two-sided lobes read query.flags inside sampleInternal, which this path fixes at All.             */
    SLRHIP_MATERIAL_MULTI = 7
};
#define SLRHIP_MULTI_INVERSE_0 1
#define SLRHIP_MULTI_INVERSE_1 2
typedef struct slrhip_material {
    uint32_t type;
    int32_t spectrum[3];   /* indices into slrhip_scene_desc::spectra, -1 = unused, SLRHIP_TEXTURE_REF(t) = texture t */
    float param;
    /* EmitterSurfaceMaterial(mat, DiffuseEmission(emittance)) surface_material.h:55-69,
     * DiffuseEmission.cpp:15-21: index of the emittance spectrum, or -1 if not emitting. */
    int32_t emittance;
    float param2;          /* second scalar of the anisotropic lobes (Ward anisoY, Ashikhmin nv), else 0 */
    uint32_t reserved;     /* 0, or SLRHIP_MATERIAL_NORMAL_MAP(t) | SLRHIP_MATERIAL_ALPHA_MAP(t') */
} slrhip_material;

/* ---- textures ------------------------------------------------------- */
/* The procedural textures the reference's libSLR itself holds (Textures/checker_board_textures.{h,cpp}), evaluated per hit at
 * the hit's texture coordinate (Triangle::intersect interpolates it from the ORIGINAL barycentrics, TriangleMesh.cpp:160-161)
 * through a Texture2DMapping (Core/textures.h:16-42): (u, v) -> ((u + offset[0]) * scale[0], (v + offset[1]) * scale[1]);
 * offset 0 / scale 1 is the default mapping.
 *   CHECKER_SPECTRUM  CheckerBoardSpectrumTexture: spectrum[((int)(2 x) + (int)(2 y)) % 2]           checker_board_textures.h:15-27
 *   CHECKER_FLOAT     CheckerBoardFloatTexture:    value[...same index...]                           :43-53
 *   CHECKER_NORMAL    CheckerBoardNormal3DTexture(stepWidth = value[0], reverse = value[1] != 0)     checker_board_textures.cpp:16-43
 * A material's spectrum slot refers to a texture with SLRHIP_TEXTURE_REF(t); its normal map (BumpSingleSurfaceObject,
 * Core/SurfaceObject.cpp:123-134) and its alpha texture (Triangle::m_alphaTex, TriangleMesh.cpp:163-167: a hit where the alpha
 * value is 0 does not occur) ride in slrhip_material::reserved, as the material group of libSLRSceneGraph/TriangleMeshNode
 * pairs them.                                                                                                              */
/*   IMAGE_SPECTRUM    ImageSpectrumTexture: the texel nearest to the mapped coordinate, wrapped by fmod                Textures/image_textures.cpp:13-79
 *                     reserved[0], reserved[1] = width, height; reserved[2] = index of the image's first texel in
 *                     slrhip_scene_desc::texture_texels (3 floats per texel, row-major).  RGB mode: what the look-up of the
 *                     reference's RGB build returns (8-bit formats: byte / 255, RGBA16F: the halves).  Spectral mode: (u, v, s) as
 *                     the spectral build stores the image (Core/Image.h:39-40,265-310), evaluated per hit like
 *                     UpsampledContinuousSpectrum(u, v, s / EqualEnergyReflectance) (image_textures.cpp:23-32) — needs
 *                     slrhip_scene_desc::upsampling.  The image decoding and colour conversion stay with the caller (libSLRSceneGraph's
 *                     image loaders are outside this boundary).                                                                  */
enum { SLRHIP_TEXTURE_CHECKER_SPECTRUM = 0, SLRHIP_TEXTURE_CHECKER_FLOAT = 1, SLRHIP_TEXTURE_CHECKER_NORMAL = 2, SLRHIP_TEXTURE_IMAGE_SPECTRUM = 3 };
typedef struct slrhip_texture {
    uint32_t kind;
    float offset[2];
    float scale[2];
    int32_t spectrum[2];       /* CHECKER_SPECTRUM: indices into slrhip_scene_desc::spectra                    */
    float value[2];            /* CHECKER_FLOAT: the two values; CHECKER_NORMAL: stepWidth in (0, 1], reverse   */
    uint32_t reserved[3];      /* IMAGE_SPECTRUM: width, height, first texel; else 0                                 */
} slrhip_texture;
#define SLRHIP_TEXTURE_REF(t) (-2 - (int32_t)(t))              /* value of slrhip_material::spectrum[k] naming texture t */
#define SLRHIP_MATERIAL_NORMAL_MAP(t) ((uint32_t)(t) + 1u)      /* OR into slrhip_material::reserved: bits 0..15  */
#define SLRHIP_MATERIAL_ALPHA_MAP(t) (((uint32_t)(t) + 1u) << 16)   /* bits 16..31                              */

/* ---- camera ---------------------------------------------------------------------- */
/* SLR::PerspectiveCamera (libSLR/Cameras/PerspectiveCamera.cpp:15-24) with its
 * StaticTransform (libSLR/Core/Transform.h:38-87).  Matrices are column-major
 * (Matrix4x4Template: m[c*4+r], libSLR/BasicTypes/Matrix4x4.h:22-45); both the
 * matrix and its inverse are given because StaticTransform stores both.
 * sensitivity <= 0 selects 1/(pi r^2) as PerspectiveCamera.cpp:23 does.               */
typedef struct slrhip_camera {
    float local_to_world[16];
    float world_to_local[16];
    float aspect;
    float fov_y;
    float lens_radius;
    float img_plane_distance;
    float obj_plane_distance;
    float sensitivity;
} slrhip_camera;

/* ---- environment light ------------------------------------------------------------ */
/* InfiniteSphereSurfaceObject + IBLEmission over an image texture (SurfaceObject.cpp:137-222,
 * SurfaceMaterials/IBLEmission.cpp:15-25, Textures/image_textures.cpp:13-79): a lat-long radiance map looked up
 * at the nearest texel (row 0 = theta 0 = +Y; u = phi / 2 pi), times `scale`, times pi.
 *   texels     : width * height * 3 floats, row-major.  RGB mode: (r, g, b) — the reference stores RGBA16F, use
 *                half-representable values.  Spectral mode: (u, v, s) as the reference's spectral build stores an
 *                RGB image (Upsampling::sRGB_to_uvs per texel, BasicTypes/Spectrum.h:148-171, kept as halves:
 *                Core/Image.h:39-40); every look-up evaluates UpsampledContinuousSpectrum(u, v, s / EqualEnergyReflectance)
 *                at the path's wavelengths (image_textures.cpp:23-32), which needs `upsampling` in the scene description.
 *   importance : map_width * map_height floats = the area-averaged luminance of each map cell, i.e. what
 *                ImageSpectrumTexture::createIBLImportanceMap's pickFunc computes BEFORE the sin(theta) factor
 *                (image_textures.cpp:81-132; map = quarter resolution).  It is an input because it is image
 *                preprocessing (Image2D::areaAverage, Core/Image.cpp:19-120); the library applies sin(theta) and
 *                builds the RegularConstantContinuous2D exactly like Core/distributions.cpp:127-224.            */
typedef struct slrhip_envmap {
    uint32_t width, height;
    const float* texels;
    float scale;
    uint32_t map_width, map_height;
    const float* importance;
} slrhip_envmap;

/* The Meng-15 RGB-upsampling tables (BasicTypes/Spectrum.h:197-575) for spectra whose (u, v) is only known at run time,
 * i.e. environment-map texels in spectral mode: grid_width x grid_height cells of 8 bytes {inside, num_points, idx[6]}
 * (row-major), num_points data points with their (u, v) and their 95-sample spectra (360-830 nm).  Constant spectra do
 * not need it: their cell look-up is resolved by the caller (slrhip_spectrum, kind UPSAMPLED).                       */
typedef struct slrhip_upsampling_tables {
    uint32_t grid_width, grid_height;      /* 12 x 14 */
    const uint8_t* cells;                  /* grid_width * grid_height * 8 bytes */
    uint32_t num_points;
    const float* point_uv;                 /* num_points * 2 */
    const float* point_spectrum;           /* num_points * 95 */
} slrhip_upsampling_tables;

/* ---- instancing ------------------------------------------------------------------- */
/* TransformedSurfaceObject over a mesh's aggregate (libSLR/Core/SurfaceObject.cpp:303-392, StaticTransform only:
 * Transform.h:38-87): the mesh is a RANGE of slrhip_scene_desc::triangles given in the mesh's local space; a ray is taken to
 * local space with world_to_local (`invert(sampledTF) * ray`: origin as a point, direction as a vector, NOT renormalised, so
 * distances stay world distances), intersected with the mesh there, and the surface point comes back through local_to_world
 * (`sampledTF * surfPt`, geometry.cpp:63-78: p as a point, the geometric normal through the inverse transpose, the shading
 * frame's axes as vectors, each re-normalised).  Ranges of two instances are either equal (one mesh, many placements — the
 * mesh's tree is built once) or disjoint; triangles inside an instanced range are not objects of the top-level aggregate.
 * Instanced triangles must not emit.  Matrices are column-major like slrhip_camera's.                                       */
typedef struct slrhip_instance {
    uint32_t first_triangle, num_triangles;
    float local_to_world[16];
    float world_to_local[16];
} slrhip_instance;

/* ---- scene ----------------------------------------------------------------------- */
typedef struct slrhip_scene_desc {
    const slrhip_vertex* vertices;
    uint32_t num_vertices;
    const slrhip_triangle* triangles;
    uint32_t num_triangles;
    const slrhip_material* materials;
    uint32_t num_materials;
    const slrhip_spectrum* spectra;
    uint32_t num_spectra;
    const float* spectrum_data;
    uint32_t num_spectrum_data;
    slrhip_camera camera;
    const slrhip_envmap* env;     /* NULL = no environment sphere (Scene::build envSphere = nullptr) */
    const slrhip_upsampling_tables* upsampling;   /* needed only with an environment map in spectral mode, else may be NULL */
    const slrhip_texture* textures;               /* NULL / 0 = no textured material (version 5)                             */
    uint32_t num_textures;
    const float* texture_texels;                  /* texels of the IMAGE_SPECTRUM textures, 3 floats each (appended in version 7) */
    uint32_t num_texture_texels;                  /* number of TEXELS                                                        */
    const slrhip_instance* instances;             /* NULL / 0 = no instanced mesh (appended in version 7)                    */
    uint32_t num_instances;
} slrhip_scene_desc;

/* ---- render settings -------------------------------------------------------------- */
/* SLR::RenderSettings as read by the path tracer (libSLR/Core/RenderSettings.h:15-22;
 * read at PathTracingRenderer.cpp:33,54-59,88).                                       */
typedef struct slrhip_render_settings {
    int32_t image_width;
    int32_t image_height;
    float time_start;
    float time_end;
    float brightness;
    int32_t rng_seed;
} slrhip_render_settings;

/* ---- image-plane shard ------------------------------------------------------------ */
/* The tile partition of PathTracingRenderer.cpp:74-79 (8x8 tiles, ImageSensor.cpp:12-14)
 * generalised to N devices: this context renders the tiles whose row-major index t
 * satisfies t % shard_count == shard_index.  {0,1} = whole image.                     */
typedef struct slrhip_shard {
    uint32_t shard_index;
    uint32_t shard_count;
} slrhip_shard;

/* ---- context configuration -------------------------------------------------------- */
#define SLRHIP_MAX_STRIPES 64u
typedef struct slrhip_config {
    int32_t device;            /* HIP device ordinal                                         */
    int32_t mode;              /* SLRHIP_MODE_*                                              */
    uint32_t stripes;          /* paths kept in flight PER PIXEL of the shard (the number of path slots = pixels x stripes):
                                * 0 = auto, else 1 .. SLRHIP_MAX_STRIPES; larger values are rejected by slrhip_create with
                                * SLRHIP_ERR_INVALID_ARGUMENT.  It sizes memory and parallelism only: a slot is not bound to
                                * a pixel, and the image is the same to the last bit for every value                      */
    uint32_t flags;            /* SLRHIP_FLAG_*                                              */
} slrhip_config;

/* ---- counters --------------------------------------------------------------------- */
typedef struct slrhip_counters {
    uint64_t samples;            /* (pixel, sample) pairs rendered since slrhip_render_begin, counted on the device
                                  * (what the wave queues handed out)                                       */
    uint64_t extension_rays;     /* Scene::intersect calls         PathTracingRenderer.cpp:147,225 */
    uint64_t shadow_rays;        /* Scene::testVisibility calls    PathTracingRenderer.cpp:180     */
    uint64_t iterations;         /* wavefront iterations launched                            */
    uint64_t bvh_nodes;          /* 4-wide nodes in the flattened tree                       */
    uint64_t bvh_depth;
    double   build_seconds;      /* host BVH build + upload                                  */
    uint64_t bvh_leaf_references;/* triangles referenced from leaves: = triangle count, or more with spatial splits */
} slrhip_counters;

/* ---- per-kernel timing and traversal statistics (measurement) ------------- */
/* Kernel classes of one wavefront iteration. */
enum {
    SLRHIP_KERNEL_TRACE = 0,           /* k_trace_ws: Scene::intersect and Scene::testVisibility of an iteration, one launch */
    SLRHIP_KERNEL_SHADE = 1,           /* k_shade: getSurfacePoint .. bsdf->sample (PathTracingRenderer.cpp:149-258) and, for a path that
                                        * ends, its sample's contribution + Job::kernel's camera ray of the slot's next sample (:100-130) */
    SLRHIP_KERNEL_TAIL = 2,            /* k_tail: the last paths of a render window, each taken to its end by one lane (all of the above
                                        * in one launch, once few slots are live)                        */
    SLRHIP_KERNEL_COUNT = 3
};
typedef struct slrhip_profile {
    uint64_t launches[SLRHIP_KERNEL_COUNT];
    double   milliseconds[SLRHIP_KERNEL_COUNT];   /* sum of HIP-event durations on the render stream  */
    uint64_t rays[2];                             /* [0] extension (closest-hit), [1] shadow rays cast (all of them traced in a COUNT_TRAVERSAL context) */
    uint64_t nodes[2];                            /* 4-wide nodes fetched (128 B each; 64 B quantized)  */
    uint64_t triangles[2];                        /* leaf triangles tested (48 B each)                 */
    uint64_t slot_visits;                         /* live slots processed by SHADE                     */
} slrhip_profile;

/* config.flags */
#define SLRHIP_FLAG_TRACE_ALL_SHADOW_RAYS 4096u /* trace every shadow ray.  By default the RGB shade kernel does not trace a light sample that decides
                                         * nothing: one whose contribution is exactly zero in every component (the light seen from behind, the
                                         * sample below the surface's horizon) and whose compensated add would leave the path's sum bit for bit
                                         * as it is.  Such a ray is still counted in slrhip_counters::shadow_rays.  Same samples, same counters,
                                         * same frame to the last bit; the comparator of the tests.  (SLRHIP_FLAG_COUNT_TRAVERSAL contexts trace
                                         * every ray as well: their per-ray figures are defined over all of them.)                          */
#define SLRHIP_FLAG_PRIMARY_RING 2048u  /* keep the primary pass on the wave-specialised ring kernel (a producer wave makes the camera rays, consumer
                                         * waves trace them) where it would run the direct kernel (one lane makes, traces and stores a sample:
                                         * scenes without instances whose tree is not the quantized one).  Same records, same samples, same
                                         * counters, same frame to the last bit; the comparator of the tests.  Nothing changes where the ring
                                         * kernel runs anyway, or where the pass is off.                                                      */
#define SLRHIP_FLAG_DYNAMIC_INSTANCED 1024u /* together with SLRHIP_FLAG_DYNAMIC_GEOMETRY (alone it means nothing): also keep what slrhip_set_vertices
                                         * works from for a scene WITH instances, and accept the call on it.  Memory: as below (a leaf record is
                                         * the top level's or a mesh's) + 4 B per mesh node + 4 B per mesh.  With 512 alone a scene with
                                         * instances is refused as before; a flat scene behaves the same with or without this flag.                  */
#define SLRHIP_FLAG_DYNAMIC_GEOMETRY 512u /* keep what slrhip_set_vertices works from (see there): the scene's vertex and index arrays, one box per leaf
                                         * record and the tree's level table stay on the device after slrhip_upload_scene.  Memory: 44 B per vertex +
                                         * 16 B per triangle + 32 B per leaf record.  Without the flag nothing is kept and nothing else changes.      */
#define SLRHIP_FLAG_NO_PRIMARY_PASS 256u /* turn the primary pass OFF.  By default the camera ray of every sample of a result window is traced by one
                                         * pass before the window's iterations and a slot shades its new sample's first hit in the launch that
                                         * starts it; with this flag a new sample's camera ray goes through the slot state and the traversal
                                         * launch of the next iteration, as it did before.  Same samples, same counters, same frame to the last
                                         * bit; the comparator of the tests.  (SLRHIP_FLAG_COUNT_TRAVERSAL also keeps the pass off.)          */
#define SLRHIP_FLAG_TAIL_KERNEL 128u   /* with a FIXED slot count (slrhip_config::stripes > 0): also hand the last <= 2^18 live slots of a render
                                         * window (never more than an eighth of the slots) to the tail kernel — one launch instead of the
                                         * last wavefront iterations.  Same samples, same frame to the last bit (the sensor adds a pixel's
                                         * samples in pass order whoever rendered them).  Always on with the automatic slot count
                                         * (stripes = 0); a caller who fixes the count gets the pure wavefront schedule unless he asks      */
#define SLRHIP_FLAG_BVH_SPATIAL_SPLITS 64u /* build the tree with spatial splits (sbvh.cpp; the reference's SBVH, Accelerator/SBVH.h:57-348):
                                         * a triangle straddling a split plane is referenced from both sides with clipped boxes.
                                         * Same hits; fewer triangle tests, more node visits: measured slower with these kernels on
                                         * every BASELINE scene, so the object-split SAH tree stays the default          */
#define SLRHIP_FLAG_BVH_DEVICE_BUILD 4u /* build the accelerator AND the per-triangle records on the GPU (bvh_device.hip: LBVH over 63-bit Morton codes,
                                         * the host build's 4-wide collapse, quantized nodes): 10 M triangles in a fraction of a second instead of
                                         * seconds on the host cores, at the price of a tree of lower quality (more nodes per ray; DESIGN.md has both
                                         * figures).  Same hits.  Automatic from 2^20 triangles on (SLRHIP_BVH=host in the environment keeps the host build);
                                         * The flag is a request, honoured only for a scene of AT LEAST 1024 triangles, WITHOUT alpha-textured triangles
                                         * and WITHOUT instances; every other scene gets the host build, and the upload succeeds without a word.
                                         * Which builder ran is in the summary of slrhip_debug_tree (include/slrhip_debug.h)              */
#define SLRHIP_FLAG_TEST_DEVICE_ERROR 16u /* test hook: the next slrhip_render raises the device-side error word, so that the
                                         * error path (SLRHIP_ERR_HIP + message) can be exercised; renders nothing useful */
#define SLRHIP_FLAG_TIME_KERNELS   1u   /* bracket every launch with HIP events (a few us per launch)        */
#define SLRHIP_FLAG_COUNT_TRAVERSAL 2u  /* count nodes / triangles per ray (instrumented kernels, slower)    */

typedef struct slrhip_ctx slrhip_ctx;

/* Replaces: `new PathTracingRenderer(spp)` libSLRSceneGraph/API.cpp:1015-1020 (device side). */
int slrhip_create(const slrhip_config* config, slrhip_ctx** out_ctx);
int slrhip_destroy(slrhip_ctx* ctx);

/* Replaces: the Scene pointer graph handed to render() (SurfaceObjectAggregate ctor
 * SurfaceObject.cpp:226-250 builds the accelerator and light list; Scene::build :396-406).
 * Copies everything; the caller keeps ownership of the host arrays.
 * Failure: an upload refused by a check on the descriptor or on a host-built tree leaves
 * the context exactly as it was: the previous scene and render state stay usable.  An
 * upload that fails once it has begun to write the device (a HIP error, a device-built tree
 * beyond the traversal's limits) leaves the context with no scene: later calls return
 * SLRHIP_ERR_NO_SCENE until an upload succeeds.                                          */
int slrhip_upload_scene(slrhip_ctx* ctx, const slrhip_scene_desc* scene);

/* Replaces: sensor->init(W,H) PathTracingRenderer.cpp:67 (ImageSensor.cpp:35-51) plus the
 * per-render setup :33-61.  Clears the accumulation state of this context's shard.
 * Failure: a call refused by a check on its arguments (image size, shard, too many path
 * slots) leaves the context exactly as it was: the previous render state stays usable.  A
 * call that fails once it has begun to allocate (a HIP error) leaves the context with no
 * render state: slrhip_render and the resolve / reduce / read calls return
 * SLRHIP_ERR_NO_SCENE and the counters report no samples or rays until a render_begin
 * succeeds, while the scene and the ray queries stay usable.                               */
int slrhip_render_begin(slrhip_ctx* ctx, const slrhip_render_settings* settings, slrhip_shard shard);

/* Replaces: the pass loop PathTracingRenderer.cpp:72-81 for passes
 * [spp_begin, spp_begin+spp_count).  Sample s of pixel (x,y) draws from the xorshift128
 * stream seeded with slrhip_sample_seed(rng_seed, x, y, s), and the sensor adds the samples
 * of a pixel in pass order (ImageSensor::add's order for one thread), so the image does not
 * depend on the shard layout, the slot count or scheduling — not even in the last bit.  Every
 * sample's contribution is kept until its window of passes is complete (16 B per pixel and
 * pass, 64 B in spectral mode; windows of at most 16 GiB, SLRHIP_RESULT_WINDOW_MB overrides;
 * longer calls are rendered window after window).  The work is ORDERED on `stream` (a hipStream_t, or
 * NULL for the default stream): it starts after what the caller queued there before.  The
 * call itself BLOCKS the host until the passes are done — the number of wavefront iterations
 * is data dependent, so the host polls a device-side "live slots" word between blocks of
 * iterations — and returns SLRHIP_ERR_HIP if a kernel raised the device error word (a
 * bounded spin that gave up, a dropped stack push: never expected, never silent).         */
int slrhip_render(slrhip_ctx* ctx, uint32_t spp_begin, uint32_t spp_count, void* stream);

/* Resolve the accumulated radiance into a linear float framebuffer
 * [height][width][components] = un-normalised SUM over samples of weight*C, exactly what
 * ImageSensor holds (ImageSensor.cpp:124-129; spectral bins already carry the 16/470
 * factor of SpectrumTypes.h:826-835).  Pixels outside the shard are written as 0, so a
 * sum-reduce over shards equals the full image.  `device_dst` is a DEVICE pointer
 * (e.g. a torch tensor's data_ptr, which is how bench.py feeds RCCL).                     */
int slrhip_resolve_framebuffer(slrhip_ctx* ctx, float* device_dst, size_t num_floats, void* stream);

/* Same, to HOST memory (synchronises).  Replaces reading camera->getSensor()->pixel(x,y)
 * (ImageSensor.cpp:88-95).                                                                */
int slrhip_read_framebuffer(slrhip_ctx* ctx, float* host_dst, size_t num_floats);

/* The single exchange of the multi-GPU path: one process per GPU renders its tile shard (slrhip_render_begin's `shard`), then all
 * ranks call this: the resolved frames (zeros outside a rank's tiles) are sum-reduced onto rank `root` with ONE ncclReduce over
 * `nccl_comm` (an ncclComm_t of RCCL the caller created, e.g. ncclCommInitRank; the call is stream-ordered on `stream`).
 * `device_dst` (DEVICE memory, num_floats >= width * height * components) receives the full image on `root`; other ranks may pass
 * NULL.  The reference has no distributed path (one process, a thread pool over 8x8 tiles: PathTracingRenderer.cpp:72-81); this
 * replaces "all tiles of the sensor are filled by this process" (ImageSensor.cpp:124-129) for a sensor spread over ranks.
 * librccl.so is loaded on first use.                                                                                     */
int slrhip_reduce_framebuffer(slrhip_ctx* ctx, void* nccl_comm, int root, float* device_dst, size_t num_floats, void* stream);

int slrhip_synchronize(slrhip_ctx* ctx);
int slrhip_get_counters(slrhip_ctx* ctx, slrhip_counters* out);
int slrhip_components(const slrhip_ctx* ctx);   /* 3 or 16 */
/* Kernel times accumulate over the life of the context; ray / node / triangle totals restart at
 * slrhip_render_begin.  Needs the matching config.flags.                                       */
int slrhip_get_profile(slrhip_ctx* ctx, slrhip_profile* out);

/* Closest-hit queries against the uploaded scene, the aggregate part of
 * Scene::intersect (SurfaceObject.cpp:267-269,408-416).  rays: n x {org[3], dir[3], dist_min,
 * dist_max}; hits: n x {triangle index as uint32 bits (0xFFFFFFFF = miss), dist, b0, b1}
 * (Intersection::dist, ::u, ::v; TriangleMesh.cpp:169-173).  Host arrays; synchronises.        */
int slrhip_trace_rays(slrhip_ctx* ctx, const float* rays, uint32_t n, float* hits);

/* ---- ray queries on device memory ------------------------------------------------------------------------------------
 * The render's own traversal (the wave-specialised kernel of every frame, on whatever tree the upload built: float, quantized,
 * instanced, LBVH, spatial splits; alpha-cut triangles tested as the render tests them) over a caller's array of rays.
 *
 * Pointers: ALL are DEVICE pointers.  rays: 16-byte aligned; hits: 16-byte aligned; instances / visible: 4-byte aligned.
 * The call is ordered on `stream` (a hipStream_t; NULL = the null stream): it reads `rays` and writes the results after the
 * work the caller queued there before, and returns at once.  It allocates nothing, copies nothing between host and device and
 * does not synchronise, so it may be captured in a graph (hipStreamBeginCapture, torch.cuda.graph).  The results must not
 * overlap `rays` or each other.
 * Errors: bad arguments return SLRHIP_ERR_INVALID_ARGUMENT at the call (null context, a null or misaligned pointer with
 * n > 0, n >= 2^31); SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.  n == 0 does nothing.  A traversal that gives up on a
 * ray (a traversal stack overflow, a bounded wait that ran out: never expected) sets a bit in the context's QUERY error word,
 * which each call clears on its stream before it traces; slrhip_query_status reads it.  A call whose status is not 0 has no
 * trustworthy result.
 * Independence: a query touches neither the render's path state nor its counters nor its error word; a query between two
 * slrhip_render calls leaves the frame bit-identical.  slrhip_upload_scene and slrhip_destroy must not run while a query of
 * the context is in flight (synchronise its stream first), and two queries of one context in flight at the same time on
 * different streams share the query error word.                                                                          */
typedef struct slrhip_ray {
    float org[3];
    float dist_min;
    float dir[3];              /* not normalised by the library: dist is measured in units of |dir| (as slrhip_trace_rays) */
    float dist_max;
} slrhip_ray;                  /* 32 bytes */

typedef struct slrhip_hit {
    uint32_t triangle;         /* index into slrhip_scene_desc::triangles (the mesh-local one for an instanced hit); 0xFFFFFFFF = miss */
    float dist;                /* Intersection::dist (INFINITY on a miss) */
    float b0, b1;              /* Intersection::u, ::v (u = 1 - b1 - b2 of Moller-Trumbore, TriangleMesh.cpp:159,172-173); 0 on a miss */
} slrhip_hit;                  /* 16 bytes: the record of slrhip_trace_rays */

/* Closest hit: the aggregate part of Scene::intersect (SurfaceObject.cpp:267-269, 408-416); the same hits as slrhip_trace_rays
 * (equal-distance ties: the larger (instance, triangle) pair wins).  instances (may be NULL): index into
 * slrhip_scene_desc::instances of the placement that was hit, -1 for a loose triangle or a miss.  The environment sphere is
 * never hit.  Replaces slrhip_trace_rays for callers that hold their rays on the device.                                  */
int slrhip_intersect_rays(slrhip_ctx* ctx, const slrhip_ray* rays, uint32_t n, slrhip_hit* hits, int32_t* instances, void* stream);

/* Visibility: the aggregate part of Scene::testVisibility (SurfaceObject.cpp:418-430): visible[i] = 1 if no triangle is hit
 * in [dist_min, dist_max], else 0 (any hit ends the ray).  The environment sphere never occludes.                        */
int slrhip_test_visibility(slrhip_ctx* ctx, const slrhip_ray* rays, uint32_t n, uint32_t* visible, void* stream);

/* The query error word (ERR bits: 1 ring space, 2 ring release, 4 consumer idle, 8 stack overflow; 0 = every ray of the last
 * query call was traced), read in order on `stream` — pass the queries' stream — and written to HOST memory *bits.  Waits for
 * that stream only, not for the device.                                                                                  */
int slrhip_query_status(slrhip_ctx* ctx, uint32_t* bits, void* stream);

/* ---- first-hit feature buffers and camera rays ------------------------------------------------------------------------------
 * What a host needs next to the beauty frame (denoiser guides, picking / masking buffers, a "what does the camera see" view): the
 * reference's DebugRenderer (Renderers/DebugRenderer.cpp:132-216) — the path tracer's own camera sample, the closest hit of the
 * aggregate with the alpha test the render applies, the surface point in world space (bump map and instance transform as in the
 * path tracer) — accumulated per pixel.  One traversal per sample, fused: the camera rays are made inside the traversal kernel.
 *
 * Channels (bits; `channels` of slrhip_render_features is a set, `channel` of slrhip_resolve_features is ONE bit):           */
#define SLRHIP_FEATURE_GEOMETRIC_NORMAL 1u   /* 3 floats  SurfacePoint::gNormal          (DebugRenderer ExtraChannel::GeometricNormal) */
#define SLRHIP_FEATURE_SHADING_NORMAL   2u   /* 3 floats  shadingFrame.z, after bump     (ExtraChannel::ShadingNormal)                 */
#define SLRHIP_FEATURE_SHADING_TANGENT  4u   /* 3 floats  shadingFrame.x, after bump     (ExtraChannel::ShadingTangent)                */
#define SLRHIP_FEATURE_DISTANCE         8u   /* 1 float   Intersection::dist of the camera ray (ExtraChannel::Distance)                */
#define SLRHIP_FEATURE_COVERAGE        16u   /* 1 float   number of samples of the pixel that hit a triangle                          */
#define SLRHIP_FEATURE_IDS             32u   /* 3 uint32  triangle, instance (0xFFFFFFFF: loose), material; all 0xFFFFFFFF on a miss   */
#define SLRHIP_FEATURE_ALL             63u

/* Passes [spp_begin, spp_begin + spp_count) of every pixel of the shard (after slrhip_render_begin): the camera ray slrhip_render
 * traces for that (pixel, pass) -> closest hit -> surface point -> per-pixel accumulation.  The float channels are PLAIN float32
 * SUMS IN PASS ORDER; a miss (the environment sphere is a miss) adds nothing, so sum / COVERAGE is the mean over the hits and
 * COVERAGE / spp the alpha of the pixel.  IDS holds the record of the highest pass rendered so far.  The accumulation is cleared
 * by slrhip_render_begin and is apart from the beauty accumulation: feature passes and slrhip_render calls may interleave in any
 * order and neither changes the other's result in any bit, nor the render's counters or error word.  The result does not depend
 * on the shard split, on how the passes are cut into calls (ascending), on the tree kind or on scheduling, and RGB and spectral
 * contexts give the same buffers for the same seed.
 * Every feature call between two slrhip_render_begin calls names the SAME channel set (another set is
 * SLRHIP_ERR_INVALID_ARGUMENT): every channel then sums over the same passes.  DISTANCE and COVERAGE come with every set at no
 * cost, but only the channels of the set can be resolved.
 * Stream-ordered and NON-BLOCKING: the call queues its launches on `stream` and returns.  The first feature call after a
 * slrhip_render_begin allocates the sums (64 B per pixel) and the record window (a render that never asks for features pays
 * nothing) and is therefore not capturable in a graph; every later call allocates nothing, copies nothing and does not
 * synchronise, and may be captured.  The record window holds 16 B per (pixel, pass), 20 B with SHADING_NORMAL or SHADING_TANGENT:
 * as many passes as fit in 512 MiB (at most 64, at least one: a shard of more than 26 M pixels takes more than 512 MiB); a
 * longer call runs window after window.  The arrays are kept for the next slrhip_render_begin and freed with the context.
 * The feature calls of one context go on ONE stream, or the caller synchronises between them: the first call after a
 * slrhip_render_begin clears the reused sums on ITS stream, which is not ordered after feature work still in flight elsewhere.
 * Errors: SLRHIP_ERR_NO_SCENE before slrhip_render_begin; SLRHIP_ERR_INVALID_ARGUMENT for no or unknown channel bits, a channel
 * set that differs from the first call's, or a pass range beyond 2^32; spp_count == 0 does nothing.  A traversal that gives up
 * (never expected) sets a bit in the context's FEATURE error word, sticky until the next slrhip_render_begin:
 * slrhip_features_status reads it.                                                                                         */
int slrhip_render_features(slrhip_ctx* ctx, uint32_t channels, uint32_t spp_begin, uint32_t spp_count, void* stream);

/* One channel into DEVICE memory as [height][width][k] (k = 3 or 1; float32, IDS: uint32; 4-byte aligned), zeros (IDS:
 * 0xFFFFFFFF) outside the shard, so that shards sum / merge like the framebuffer.  num_elements: room at device_dst, in
 * elements; at least width x height x k.  Stream-ordered, non-blocking, allocates nothing.  A channel that no
 * slrhip_render_features call since slrhip_render_begin asked for is SLRHIP_ERR_INVALID_ARGUMENT.                          */
int slrhip_resolve_features(slrhip_ctx* ctx, uint32_t channel, void* device_dst, size_t num_elements, void* stream);

/* The same into HOST memory: resolves, waits for the device, and fails with SLRHIP_ERR_HIP if the feature error word is set.  */
int slrhip_read_features(slrhip_ctx* ctx, uint32_t channel, void* host_dst, size_t num_elements);

/* The camera ray of sample `pass` of every pixel of the shard (after slrhip_render_begin), in DEVICE memory: rays[i] (16-byte
 * aligned; dist_min = 0, dist_max = INFINITY) and pixel_xy[i] = x | y << 16 (4-byte aligned; may be NULL), i < *count.  It is
 * the ray slrhip_render and slrhip_render_features trace for that (pixel, pass): same seed (slrhip_sample_seed), same draws in
 * the same order (time, pixel x, pixel y, wavelength offset, wavelength selection, two lens draws), same float operations.
 * capacity: room at rays / pixel_xy in rays; smaller than the shard's pixel count is SLRHIP_ERR_INVALID_ARGUMENT.  *count (HOST
 * memory) is known from the render plan and written at the call; rays == pixel_xy == NULL with capacity 0 asks for the count alone.  Stream-ordered, non-blocking, allocates nothing, does not
 * synchronise: capturable like the ray queries.                                                                             */
int slrhip_camera_rays(slrhip_ctx* ctx, uint32_t pass, slrhip_ray* rays, uint32_t* pixel_xy, uint32_t capacity, uint32_t* count, void* stream);

/* The feature error word (the bits of slrhip_query_status; 0 = every sample of every feature call since slrhip_render_begin was
 * traced), read in order on `stream` and written to HOST memory *bits.  Waits for that stream only.                          */
int slrhip_features_status(slrhip_ctx* ctx, uint32_t* bits, void* stream);

/* ---- albedo: the first-hit base colour, accumulated like the feature channels ---------------------------------------------------
 * What a denoiser divides the frame by (slrhip_modulate below): per sample, the reference's BSDF::getBaseColor(DirectionType::All)
 * (Core/directional_distribution_functions.h:293-297) at the camera ray's first hit.  Its own calls, not a channel bit of
 * slrhip_render_features: the buffer has `components` floats per pixel and differs between the RGB and the spectral mode.
 *
 * The definition, per (pixel, pass) of the shard.
 *   Ray:      the camera ray slrhip_render and slrhip_render_features trace for that (pixel, pass): same seed, same draws.
 *   Hit:      the closest hit of the aggregate, with the alpha test the render applies.  A miss (the environment sphere is a miss)
 *             has the value 1.0 in every component: radiance that reaches the camera unscattered is divided by one.
 *   Material: the hit triangle's material record; each spectrum slot that names a texture is replaced by the texture's value at the
 *             hit's texture coordinate, interpolated from the ORIGINAL barycentrics (TriangleMesh.cpp:160-161), as the render does.
 *   Spectra:  RGB mode: the three record values.  Spectral mode: component i is the spectrum's value at lambda_i of
 *             WavelengthSamples::createWithEqualOffsets(offset, .) (lambda_i = 360 + 470 (i + offset) / 16), offset = the sample's
 *             wavelength-offset draw (the fourth draw of the camera sample); component i is indexed by i, not binned as the sensor bins.
 *   Colour:   by material type, every operation float32 and rounded on its own:
 *               MATTE (Lambert and Oren-Nayar)  R                                    basic_BSDFs.cpp:55, OrenNayerBRDF.cpp:71
 *               METAL                           coeffR                               basic_BSDFs.cpp:89
 *               GLASS                           coeff                                basic_BSDFs.cpp:167
 *               MICROFACET_METAL                FresnelConductor(eta, k).evaluate(1.0f) (the render's Fresnel function at cosine 1)
 *                                                                                    MicrofacetBSDF.cpp:108
 *               MICROFACET_GLASS                1 in every component                 MicrofacetBSDF.cpp:313
 *               WARD                            R                                    ModifiedWardDurBRDF.cpp:84
 *               ASHIKHMIN                       Rs + (1 - Rs) * Rd, in that order    AshikhminShirleyBRDF.cpp:167
 *               MULTI                           the lobes in order (nested groups flattened in order), each with the `scale * spectrum`
 *                                               its getBSDF receives; the first lobe whose colour has a non-zero component wins; zeros if
 *                                               there is none.  An inverted lobe has its base's colour.  MultiBSDF.cpp:210-218
 *             An emitting triangle is treated like any other: its BSDF's base colour.
 *   Sum:      plain float32 sums in pass order, one lane per pixel, like the feature channels.  sum / passes is the mean albedo, also of
 *             a partially covered pixel (a miss counts as one), so no coverage buffer is needed.
 *
 * The contract mirrors the feature calls.  Cleared by slrhip_render_begin; independent of the shard split, of how ascending passes are
 * cut into calls, of the tree kind and of scheduling.  Stream-ordered and NON-BLOCKING.  The first albedo call after a
 * slrhip_render_begin allocates (the sums: components x 4 B per pixel; the record window, which is the feature pass's: 16 B per
 * (pixel, pass), 20 B for a scene with textures, at most 64 passes) and is not capturable; later calls allocate nothing, copy
 * nothing, do not synchronise and may be captured.  The record window is shared with the feature pass: the albedo and feature calls of
 * one context go on ONE stream (or the caller synchronises between them), and the first feature call and the first albedo call after
 * a slrhip_render_begin may each allocate — and either may MOVE the shared record window when it needs more room than the other
 * sized it for.  A graph that holds feature or albedo calls of a context that uses both must therefore be captured after BOTH
 * first calls of that slrhip_render_begin: a call captured earlier holds the window's old address.  Feature calls, albedo calls and slrhip_render calls interleave freely: none changes a bit of
 * another's result, of the counters or of the error words.  A traversal that gives up sets the FEATURE error word
 * (slrhip_features_status); slrhip_read_albedo fails on it as slrhip_read_features does.
 * Errors: SLRHIP_ERR_NO_SCENE before slrhip_render_begin; SLRHIP_ERR_INVALID_ARGUMENT for a null context, a pass range beyond 2^32, a
 * null or misaligned (4 bytes) destination or too little room; spp_count == 0 does nothing.                                       */
int slrhip_render_albedo(slrhip_ctx* ctx, uint32_t spp_begin, uint32_t spp_count, void* stream);
/* The SUMS into DEVICE memory as [height][width][components] float32, zeros outside the shard, so that shards add like the frame;
 * num_floats: room at device_dst, at least width x height x components.  *passes (HOST memory, may be NULL; written at the call): the
 * number of passes accumulated since slrhip_render_begin, the divisor of the mean.  Stream-ordered, non-blocking, allocates nothing;
 * before the first albedo call the sums are zeros and *passes is 0.                                                                */
int slrhip_resolve_albedo(slrhip_ctx* ctx, float* device_dst, size_t num_floats, uint32_t* passes, void* stream);
/* The same into HOST memory: resolves, waits for the device, and fails with SLRHIP_ERR_HIP if the feature error word is set.       */
int slrhip_read_albedo(slrhip_ctx* ctx, float* host_dst, size_t num_floats, uint32_t* passes);

/* ---- motion vectors: where was this sample's surface point on the previous frame's image? ------------------------------------------
 * What temporal reprojection (slrhip_reproject below) fetches the previous frame's history along.  Its own calls, not a channel bit of
 * slrhip_render_features: SLRHIP_FEATURE_ALL stays 63.  The call is STATELESS: the library keeps no previous frame; the caller names it,
 * because the caller uploaded it (slrhip_set_instance_transforms, slrhip_set_camera).
 *
 * The definition, per (pixel, pass) of the shard.  Everything is float32, every operation IEEE-rounded on its own (no fused
 * multiply-add), IEEE division and square root; stated once for host and device in slr_amd/csrc/pt_motion.h.
 *   Ray, hit:   the camera ray and the closest hit of slrhip_render_features for that (pixel, pass): same seed, same draws, the alpha
 *               test the render applies.  A miss (the environment sphere is a miss) adds nothing.
 *   Point now:  P = org + dist * dir, per component, one multiply and one add.
 *   mulPoint:   (M, p) -> per row r of the column-major M: ((M[r] p.x + M[4 + r] p.y) + M[8 + r] p.z) + M[12 + r] * 1.0f, rows 0 .. 3; if
 *               the fourth, w, is not 1: x, y, z each times (1.0f / w).  (Matrix4x4.h:71-81; the traversal's own.)
 *   Local:      an instanced hit: l = mulPoint(world_to_local_now, P); a loose triangle: l = P.
 *   Placements: an instanced hit: P_now = mulPoint(local_to_world_now, l), P_prev = mulPoint(local_to_world_prev, l); a loose triangle:
 *               P_now = P_prev = l.  Both points go through the same arithmetic on purpose: where nothing moved (matrices bit-equal,
 *               cameras equal) the motion is exactly 0.0f, with no special case.
 *   proj(cam, Q), the inverse of the camera sample through the lens CENTRE (depth of field is ignored):
 *               q = mulPoint(cam.world_to_local, Q); valid if q.z > 0 and q.x, q.y, q.z are finite;
 *               X = (0.5f - ((q.x / q.z) * objPlaneDistance) / opWidth) * (float)width
 *               Y = (0.5f - ((q.y / q.z) * objPlaneDistance) / opHeight) * (float)height            evaluated as written,
 *               with opHeight = 2.0f * obj_plane_distance * tanf(fov_y * 0.5f) and opWidth = opHeight * aspect from the host
 *               arithmetic of slrhip_upload_scene's camera constants (PerspectiveCamera.cpp:15-24); slrhip_motion_camera returns them.
 *   Result:     the sample is VALID if proj(cam_now, P_now) and proj(cam_prev, P_prev) are both valid;
 *               m = proj(cam_prev, P_prev) - proj(cam_now, P_now), in pixels: a pixel centre p of this frame was at p + m;
 *               z' = length(P_prev - C_prev) = sqrtf((dx dx + dy dy) + dz dz), C_prev = mulPoint(cam_prev.local_to_world, (0, 0, 0)):
 *               the distance the previous frame's DISTANCE feature would have shown for the point.
 *   Sum:        per pixel a float4 {sum m.x, sum m.y, sum z', number of valid samples} over the VALID samples: plain float32 sums in
 *               pass order, one lane per pixel, like the feature channels.  sum / w is the mean over the valid samples.
 *
 * The contract mirrors slrhip_render_albedo's.  Cleared by slrhip_render_begin; independent of the shard split, of how ascending passes
 * are cut into calls, of the tree kind and of scheduling; RGB and spectral contexts give equal buffers.  Stream-ordered and
 * NON-BLOCKING.  The first motion call after a slrhip_render_begin allocates (the sums: 16 B per pixel; the record window, which is the
 * feature pass's: 16 B per (pixel, pass), at most 64 passes) and is not capturable; later calls allocate nothing, copy nothing, do not
 * synchronise and may be captured.  The record window is shared with the feature and the albedo passes: the three kinds of call of one
 * context go on ONE stream (or the caller synchronises between them), and the first call of each kind after a slrhip_render_begin may
 * MOVE the shared record window when it needs more room than the others sized it for: capture graphs after the first calls.
 * EVERY motion call between two slrhip_render_begin calls must name the SAME previous frame (the same camera values, the same matrices):
 * the sums of a pixel would otherwise mix vectors into two different frames.  The library cannot check this and does not.
 * The previous camera is taken BY VALUE at the call; `previous_transforms` is read in order on `stream` and is free once the stream has
 * passed the call.  Motion calls interleave freely with slrhip_render, feature and albedo calls: none changes a bit of another's
 * result, of the counters or of the error words.  A traversal that gives up sets the FEATURE error word (slrhip_features_status);
 * slrhip_read_motion fails on it as slrhip_read_features does.
 * Errors: SLRHIP_ERR_INVALID_ARGUMENT for a null context or descriptor, a nonzero `reserved`, a misaligned (16 bytes)
 * previous_transforms, previous_transforms on a scene without instances, a pass range beyond 2^32, a null or misaligned (4 bytes)
 * destination or too little room; SLRHIP_ERR_NO_SCENE before slrhip_render_begin; spp_count == 0 does nothing.
 * Not covered: the environment under camera rotation (a miss has no vector); motion of loose triangles (they are taken to stand
 * still; only instances and the camera move — vertices moved by slrhip_set_vertices, of loose triangles and of meshes alike, are
 * covered by slrhip_render_motion_vertices below); depth of field (the projection goes through the lens centre).                    */
struct slrhip_instance_transform;                                    /* defined below, with slrhip_set_instance_transforms */
typedef struct slrhip_motion_desc {
    const slrhip_camera* previous_camera;                           /* HOST; NULL = the camera did not move */
    const struct slrhip_instance_transform* previous_transforms;    /* DEVICE, 16-byte aligned, ALL instances of the scene, in order;
                                                                       NULL = no instance moved (required NULL for a scene without instances) */
    uint32_t reserved[2];                                           /* 0 */
} slrhip_motion_desc;
int slrhip_render_motion(slrhip_ctx* ctx, const slrhip_motion_desc* desc, uint32_t spp_begin, uint32_t spp_count, void* stream);
/* The SUMS into DEVICE memory as [height][width][4] float32 {sum m.x, sum m.y, sum z', valid samples}, zeros outside the shard, so that
 * shards add like the frame; num_floats: room at device_dst, at least width x height x 4.  Stream-ordered, non-blocking, allocates
 * nothing; before the first motion call the sums are zeros.                                                                         */
int slrhip_resolve_motion(slrhip_ctx* ctx, float* device_dst, size_t num_floats, void* stream);
/* The same into HOST memory: resolves, waits for the device, and fails with SLRHIP_ERR_HIP if the feature error word is set.       */
int slrhip_read_motion(slrhip_ctx* ctx, float* host_dst, size_t num_floats);

/* The constants proj() takes of a camera, on the HOST (pure; no GPU is touched), from the arithmetic the upload uses: out[0 .. 15] the
 * world_to_local matrix as used, out[16 .. 18] the lens centre mulPoint(local_to_world, (0, 0, 0)), out[19] opWidth, out[20] opHeight,
 * out[21] objPlaneDistance, out[22], out[23] = 0.  So that a test can take the constants without restating tanf.                     */
int slrhip_motion_camera(const slrhip_camera* camera, float out[24]);
/* One sample through the function the kernel calls (pt_motion.h), on the HOST (pure).  now_record / prev_record: the 32 floats of a
 * slrhip_instance_transform of the instance that was hit, now and in the previous frame; now_record NULL: a loose triangle
 * (prev_record is not read); prev_record NULL: the instance did not move.  P: the hit point now.  out = {m.x, m.y, z', 1} for a valid
 * sample, {0, 0, 0, 0} for one that is not.  SLRHIP_ERR_INVALID_ARGUMENT for a null camera, P or out.                                */
int slrhip_motion_sample(const slrhip_camera* now_camera, const slrhip_camera* prev_camera, const float* now_record, const float* prev_record,
                         uint32_t width, uint32_t height, const float P[3], float out[4]);

/* ---- motion vectors of moved vertices: the caller also names the previous frame's vertices ----------------------------------------
 * slrhip_render_motion takes vertices to stand still.  A caller who deforms a mesh with slrhip_set_vertices (below) names the vertices
 * of the previous frame here, beside the previous camera and placements of `frame`.  The call adds into the SAME per-pixel sums as
 * slrhip_render_motion (read by slrhip_resolve_motion / slrhip_read_motion) and keeps that call's contract in full: stateless;
 * stream-ordered and non-blocking; the first motion call after a slrhip_render_begin allocates and may MOVE the shared record window
 * (this call's window also keeps the second barycentric: 20 B per (pixel, pass), at most 64 passes; the first call of EACH of the two
 * kinds may move it), later calls allocate nothing and may be captured; the same independence of shards, cuts, colour mode and
 * interleaved calls; ALL motion calls of one render, of either kind, name ONE previous frame.  `previous_vertices` is read in order
 * on `stream` and is free once the stream has passed the call.
 *
 * With previous_vertices == NULL the call IS slrhip_render_motion(ctx, &desc->frame, ...): the same path, the same kernel, bit for bit,
 * in any context.
 *
 * The definition of a sample when previous_vertices is given (float32, every operation IEEE-rounded on its own, no fused multiply-add;
 * stated once for host and device in slr_amd/csrc/pt_motion.h, motionSampleVertices):
 *   Hit:        the feature pass's hit record of that (pixel, pass): triangle t, instance, and Moller-Trumbore's barycentrics b1 (on
 *               the triangle's second vertex) and b2 (on its third).  A miss adds nothing.
 *   b0:         b0 = (1.0f - b1) - b2.
 *   Vertices:   (i0, i1, i2) = the context's kept index array at t; p_k = the position of vertex i_k in the kept vertex array AS IT NOW
 *               STANDS (after every slrhip_set_vertices ordered before the call); q_k = the position of vertex i_k in previous_vertices.
 *   Local:      per component l_now = (b0 * p0 + b1 * p1) + b2 * p2 and l_prev = (b0 * q0 + b1 * q1) + b2 * q2: one expression on two
 *               sets of operands, so where the two arrays are bit-equal the two points are, and with equal matrices and cameras the
 *               motion is exactly 0.0f, with no special case.  The camera ray is not rebuilt: org + dist * dir is not used here.
 *   Placements: an instanced hit: P_now = mulPoint(local_to_world_now, l_now), P_prev = mulPoint(local_to_world_prev, l_prev), the
 *               previous record being the current one when frame.previous_transforms is NULL; a loose triangle: P_now = l_now,
 *               P_prev = l_prev.  (A mesh's vertices are in its local space, as the upload stores them.)
 *   Result:     proj, validity, m, z' and the sums exactly as above.  A previous position that is not finite makes the sample INVALID:
 *               it adds nothing, and the sums stay finite.
 *
 * Errors, synchronous, with nothing changed: everything slrhip_render_motion refuses for `frame`; SLRHIP_ERR_INVALID_ARGUMENT for a
 * null descriptor, a nonzero outer `reserved` or a previous_vertices misaligned to 4 bytes; SLRHIP_ERR_UNSUPPORTED for
 * previous_vertices in a context that does not keep the vertex and index arrays — one created without SLRHIP_FLAG_DYNAMIC_GEOMETRY, a
 * scene with instances in one created without SLRHIP_FLAG_DYNAMIC_INSTANCED (the message names the missing flag), a tree built with
 * spatial splits.  The library CANNOT check how long the caller's array is: it must hold all slrhip_scene_desc::num_vertices records.
 * Not covered: vertex normals and shading of the previous frame, motion of the environment, depth of field, the C++ host mirror, the
 * libSLR adapter and bench.py.                                                                                                       */
typedef struct slrhip_motion_vertices_desc {
    slrhip_motion_desc frame;                  /* exactly as for slrhip_render_motion (reserved 0)                       */
    const slrhip_vertex* previous_vertices;    /* DEVICE, 4-byte aligned, ALL num_vertices records of the scene in order,
                                                  as the previous frame had them; only `position` is read.
                                                  NULL = no vertex moved                                                    */
    uint64_t reserved;                         /* 0 */
} slrhip_motion_vertices_desc;
int slrhip_render_motion_vertices(slrhip_ctx* ctx, const slrhip_motion_vertices_desc* desc, uint32_t spp_begin, uint32_t spp_count, void* stream);
/* One sample of that definition through the function the kernel calls (pt_motion.h), on the HOST (pure).  Cameras, records, width,
 * height and out as for slrhip_motion_sample (only local_to_world is read of a record).  now_positions / prev_positions: x, y, z of the
 * hit triangle's first, second and third vertex, now and in the previous frame; b1, b2: the hit's barycentrics.
 * SLRHIP_ERR_INVALID_ARGUMENT for a null camera, position array or out.                                                              */
int slrhip_motion_sample_vertices(const slrhip_camera* now_camera, const slrhip_camera* prev_camera, const float* now_record, const float* prev_record,
                                  uint32_t width, uint32_t height, const float now_positions[9], const float prev_positions[9], float b1, float b2,
                                  float out[4]);

/* The per-(pixel, sample) seeding contract (pure function, also used by the oracle).      */
int32_t slrhip_sample_seed(int32_t rng_seed, uint32_t pixel_x, uint32_t pixel_y, uint32_t pass);

/* ---- per-pixel noise statistics and rendering to a noise target ------------------------------------------------------------
 * How noisy is the frame, and when is it good enough?  The reference leaves that to a human looking at the BMPs it writes after
 * 1, 2, 4, ... passes (PathTracingRenderer.cpp:83-94).  With statistics on, the pass that adds a window's samples to the sensor
 * (ImageSensor::add, in pass order) also keeps, per pixel of the shard, the running moments of the samples' LUMINANCE: one
 * 16-byte record {mean, M2, n, max}, updated per sample with float32 Welford steps in pass order,
 *     n += 1;  d = Y - mean;  mean = mean + d / (float)n;  M2 = M2 + d * (Y - mean);  max = fmaxf(max, Y);
 * (IEEE division; a non-finite sample is not filtered and propagates into the mean).  Like the frame, the records depend on the
 * (pixel, pass) samples alone: not on the slot count, the shard split, the result windows, how the passes are cut into
 * slrhip_render calls (ascending) or scheduling — not even in the last bit.  A render that does not ask for statistics launches
 * the kernels it launched before and produces the same bits; with statistics on, the frame, the counters and the error word
 * are unchanged in every bit.  slrhip_render and slrhip_render_until give every pixel the same passes; per-pixel adaptive sampling
 * on top of the records is slrhip_render_adaptive, below.
 *
 * The luminance of a sample = of its result-window entry, weight x C as ImageSensor::add receives it (un-normalised: not
 * divided by the pass count, no brightness, no sensitivity, no clamp), with the constants of slrhip_tonemap_bgr8:
 *   3 components:  Y = (float)(0.222485 * r + 0.716905 * g + 0.060610 * b)     (double literals, float operands; saveImage's Y)
 *   16 components: p_q = ((w[4q] v[4q] + w[4q+1] v[4q+1]) + w[4q+2] v[4q+2]) + w[4q+3] v[4q+3] for q = 0..3 in float32, with w =
 *                  DiscretizedSpectrum::ybar (16 strata); Y = ((p_0 + p_1) + (p_2 + p_3)) / integralCMF.
 * Pure function; the kernels evaluate the same expression.  Other component counts return NaN.                              */
float slrhip_sample_luminance(int32_t components, const float* values);

/* Channels of slrhip_resolve_statistics / slrhip_read_statistics (ONE bit per call), each [height][width] float32:          */
#define SLRHIP_STATISTICS_MEAN             1u   /* mean of the pixel's sample luminances                                     */
#define SLRHIP_STATISTICS_VARIANCE         2u   /* sample variance M2 / (n - 1); 0 while n < 2                                */
#define SLRHIP_STATISTICS_VARIANCE_OF_MEAN 4u   /* M2 / ((n - 1) n), the divisor a float32 product; 0 while n < 2            */
#define SLRHIP_STATISTICS_COUNT            8u   /* n, as float                                                               */
#define SLRHIP_STATISTICS_MAX             16u   /* largest sample luminance (0 before the first sample)                      */
#define SLRHIP_STATISTICS_ALL             31u

/* Switches statistics on for the render that slrhip_render_begin just began: call it after slrhip_render_begin and before that
 * render's first slrhip_render.  Later: SLRHIP_ERR_INVALID_ARGUMENT (the render goes on, its frame untouched); before
 * slrhip_render_begin: SLRHIP_ERR_NO_SCENE.  Allocates the records (16 B per pixel of the shard) and the summary's partial sums;
 * they are kept for later renders and freed with the context.  A failed allocation (SLRHIP_ERR_HIP) leaves statistics off and the
 * render usable.  The records are cleared in stream order by the first statistics-aware call that follows (render, resolve,
 * summary), on that call's stream: keep one render's calls on one stream, or synchronise between them.  Every
 * slrhip_render_begin switches statistics off again.                                                                        */
int slrhip_statistics_begin(slrhip_ctx* ctx);

/* One channel into DEVICE memory as [height][width] float32 (num_floats: room at device_dst, at least width x height), zeros
 * outside the shard, so that the channels of shards add up to the whole frame's.  Stream-ordered, non-blocking, allocates
 * nothing.  SLRHIP_ERR_INVALID_ARGUMENT when statistics are off, when `channel` is not exactly one SLRHIP_STATISTICS_* bit, or
 * when the destination is null, misaligned (4 bytes) or too small; SLRHIP_ERR_NO_SCENE before slrhip_render_begin.            */
int slrhip_resolve_statistics(slrhip_ctx* ctx, uint32_t channel, float* device_dst, size_t num_floats, void* stream);
/* The same into HOST memory (synchronises the device).                                                                      */
int slrhip_read_statistics(slrhip_ctx* ctx, uint32_t channel, float* host_dst, size_t num_floats);

/* Totals over the pixels of the shard.  The three sums are taken in double over the float32 channel values, in a fixed order
 * (a two-stage reduction without floating-point atomics whose grid depends on the pixel count alone): two calls on the same
 * state return the same bits.  All fields ADD over shards except max_sample (take the larger).  (A struct tag, not a typedef:
 * the function below has the same name.)                                                                                     */
struct slrhip_statistics_summary {
    uint64_t pixels;                  /* pixels of the shard                                          */
    uint64_t samples;                 /* sum of COUNT: pixels x passes folded so far                  */
    double sum_mean;                  /* sum of MEAN                                                  */
    double sum_mean_sq;               /* sum of MEAN^2 (the square taken in double)                   */
    double sum_variance_of_mean;      /* sum of VARIANCE_OF_MEAN                                      */
    float max_sample;                 /* largest MAX                                                  */
    uint32_t reserved;
};                                    /* 48 bytes */
/* Fills *host_out (HOST memory) in order on `stream`; waits for that stream only, not for the device.  Allocates nothing.
 * SLRHIP_ERR_INVALID_ARGUMENT when statistics are off; SLRHIP_ERR_NO_SCENE before slrhip_render_begin.                       */
int slrhip_statistics_summary(slrhip_ctx* ctx, struct slrhip_statistics_summary* host_out, void* stream);

/* Rendering to a noise target.  metric, evaluated on the host in double from the summary:                                  */
#define SLRHIP_NOISE_RMSE     0u   /* sqrt(sum_variance_of_mean / pixels): the estimated RMS error of the per-pixel mean luminance */
#define SLRHIP_NOISE_RELATIVE 1u   /* that divided by the frame's mean luminance sum_mean / pixels; infinity when that is 0 */
typedef struct slrhip_noise_target {
    uint32_t metric;                  /* SLRHIP_NOISE_*                                                */
    float target;                     /* stop once metric <= target (0: never; INFINITY: after the first block with 2 passes) */
    uint32_t spp_step;                /* passes per block: the stop check runs after each block        */
    uint32_t spp_max;                 /* at most this many passes; the last block is cut to fit        */
} slrhip_noise_target;
/* Renders passes [spp_begin, spp_begin + *spp_done) in blocks of spp_step passes through slrhip_render (same stream ordering,
 * blocks the host).  After each block it takes the summary and stops at the first block after which every pixel holds at least 2
 * samples and metric <= target, or at spp_max passes.  Every pixel gets the same passes, so the frame is BIT-IDENTICAL to one
 * slrhip_render(ctx, spp_begin, *spp_done, stream).  *spp_done (HOST) is the number of passes rendered by this call, also when
 * it fails part-way; *last (HOST, may be NULL) the summary of the last stop check.  The records continue across calls, like
 * the frame: a second call goes on from where the first stopped (give it spp_begin + *spp_done).
 * Needs slrhip_statistics_begin (else SLRHIP_ERR_INVALID_ARGUMENT); spp_step == 0, spp_max == 0, an unknown metric, a NaN
 * target or a pass range beyond 2^32: SLRHIP_ERR_INVALID_ARGUMENT; before slrhip_render_begin: SLRHIP_ERR_NO_SCENE.
 * Per context: a multi-rank host renders fixed blocks with slrhip_render on every rank, adds the ranks' summaries (the sums add)
 * and evaluates the metric itself, so that all ranks stop at the same pass.                                                 */
int slrhip_render_until(slrhip_ctx* ctx, uint32_t spp_begin, const slrhip_noise_target* target, uint32_t* spp_done,
                        struct slrhip_statistics_summary* last, void* stream);

/* ---- adaptive sampling: retire converged pixels, render only the rest --------------------------------------------------------
 * slrhip_render_until stops the whole frame; here every pixel stops on its own.  The call renders blocks of passes — the first of
 * spp_min passes, every later one of spp_step, the last cut to fit spp_max — through the window loop of slrhip_render (same
 * ordering on `stream`, same host blocking, same device error word).  After EACH block, the last included, the check below runs on
 * the noise records of the pixels that are still active, and a pixel that passes it RETIRES: it gets no further pass from any
 * adaptive call until the next slrhip_render_begin, which makes every pixel active again.  The call ends when no pixel is active
 * or spp_max passes have been handed out.  Every still-active pixel has received the same passes, so a block is an ordinary render
 * window over a shorter, compacted pixel list (ascending order of the shard's pixel list, compacted on the device without atomics:
 * the list, too, is reproducible); the records of retired pixels stay as they are.
 *
 * The check, on a pixel's record {mean, M2, n, max}, in float32, every operation IEEE-rounded on its own (no fused multiply-add):
 *     vom = M2 / ((float)(n - 1) * (float)n)        the expression of the VARIANCE_OF_MEAN channel
 *     m   = fmaxf(mean, floor)
 *     a   = threshold * m
 *     the pixel retires if  n >= 2  &&  vom <= a * a
 * i.e. when the standard error of the pixel's mean luminance is at most `threshold` times that mean, or times `floor` for a pixel
 * darker than that.  A NaN record never retires: a NaN M2 makes vom NaN and the comparison false; a NaN mean is tested
 * explicitly (fmaxf(NaN, floor) is floor, so the rule alone would not see it).  threshold = 0 retires exactly the pixels whose
 * samples so far all had the same luminance.  threshold = INFINITY retires every pixel at the first check IF floor > 0.  With
 * floor = 0 a pixel whose mean is 0 (black so far) gives a = INFINITY * 0 = NaN and NEVER retires at an infinite threshold.
 *
 * Invariants.  The rule reads one pixel's own samples only, so the frame, the noise records and the per-pixel counts depend on
 * (seed, target) alone: not — in any bit — on the slot count, the shard split, the result-window size or scheduling.  A
 * multi-rank host needs no exchange to stay consistent.  Cutting a call in two: EVERY call begins with a block of spp_min passes,
 * so two calls reproduce one only if the first ends at a block boundary of the single call and the second is given the single
 * call's spp_step as its spp_min (and spp_max = the passes that are left); any other cut moves the checks and is another target.
 * slrhip_render and slrhip_render_until keep rendering ALL pixels of the shard, retired or not, unchanged in every bit; a
 * context that never calls slrhip_render_adaptive launches the kernels it launched before.
 * Cost: the 16 B per pixel of the records plus two pairs of list buffers of 8 B per pixel, allocated at the first adaptive call,
 * kept for later renders and freed with the context; per block one check (three small launches over the active list) and one
 * 4-byte read-back.  The slot count stays the shard's: with few active pixels most slots idle at once and the tail kernel takes
 * over early.                                                                                                                */
typedef struct slrhip_adaptive_target {
    float    threshold;   /* t >= 0: relative standard error of the pixel's mean luminance at which it retires */
    float    floor;       /* f >= 0: luminance below which the error is taken relative to f, not to the mean */
    uint32_t spp_min;     /* >= 2: passes every pixel gets before the first check */
    uint32_t spp_step;    /* >= 1: passes per block after that; a check follows every block */
    uint32_t spp_max;     /* >= spp_min: no pixel gets more passes than this from this call */
} slrhip_adaptive_target;
/* Passes [spp_begin, spp_begin + *spp_done) for the pixels that stay active longest.  *spp_done (HOST): the passes the
 * longest-lived pixel got from this call; *samples_done (HOST, may be NULL): the (pixel, pass) samples it rendered (what
 * slrhip_counters::samples rose by).  Both are written on a failure part-way through as well.  A second call continues with the
 * surviving pixels: give it spp_begin + *spp_done, as with slrhip_render_until; with no pixel active it returns SLRHIP_OK and
 * *spp_done = 0, as does a call on an empty shard.
 * Needs slrhip_statistics_begin for the current render (else SLRHIP_ERR_INVALID_ARGUMENT).  SLRHIP_ERR_INVALID_ARGUMENT also for a
 * null argument, a NaN or negative threshold or floor, spp_min < 2, spp_step == 0, spp_max < spp_min, or a pass range beyond 2^32;
 * a refused call renders nothing and leaves the frame untouched.  Before slrhip_render_begin: SLRHIP_ERR_NO_SCENE.            */
int slrhip_render_adaptive(slrhip_ctx* ctx, uint32_t spp_begin, const slrhip_adaptive_target* target, uint32_t* spp_done,
                           uint64_t* samples_done, void* stream);
/* The frame as per-pixel MEANS, for pixels with unequal counts: [height][width][components], sum[c] / (float)n (IEEE division) with
 * n of the pixel's noise record, 0 where n == 0, zeros outside the shard.  slrhip_resolve_framebuffer is unchanged: the frame
 * stays the un-normalised sum.  Needs statistics on (else SLRHIP_ERR_INVALID_ARGUMENT); pointer, alignment and size rules are those of
 * slrhip_resolve_framebuffer (DEVICE memory, stream-ordered, non-blocking) / slrhip_read_framebuffer (HOST memory, synchronises). */
int slrhip_resolve_framebuffer_mean(slrhip_ctx* ctx, float* device_dst, size_t num_floats, void* stream);
int slrhip_read_framebuffer_mean(slrhip_ctx* ctx, float* host_dst, size_t num_floats);
/* *host_count (HOST) = pixels of the shard not yet retired: all of them after slrhip_render_begin.  The count is known on the
 * host since the last check (slrhip_render_adaptive blocks), so nothing is queued on `stream`.                                */
int slrhip_adaptive_active(slrhip_ctx* ctx, uint32_t* host_count, void* stream);   /* pixels of the shard not yet retired */

/* ---- sample clamp: bound a sample's luminance, drop non-finite samples ---------------------------------------------------------
 * A firefly — one sample many orders of magnitude brighter than its pixel's mean — or a single NaN sample spoils a pixel for any
 * pass count a user can afford, and everything downstream with it (the noise records, the denoiser, the tone map).  With a clamp
 * on, the pass that adds a window's samples to the sensor first puts EVERY sample through the rule below: those of slrhip_render,
 * slrhip_render_until and slrhip_render_adaptive, whichever kernel rendered them (no kernel adds to the sensor anywhere else).
 *
 * The rule, per sample v of C components as the sensor would receive it, BEFORE the Kahan add and the Welford step; float32, every
 * operation IEEE-rounded on its own (no fused multiply-add), IEEE division:
 *     Y = the expression of slrhip_sample_luminance on v
 *     if (flags & SLRHIP_CLAMP_DROP_NONFINITE) && !(fabsf(Y) < INFINITY):            NaN or +-infinity
 *         v[k] = +0.0f for every k;  Y = +0.0f;  record.dropped += 1
 *     else if Y > limit:                                                             false for a NaN; Y == limit is not clamped
 *         f = limit / Y;  v[k] = v[k] * f for every k
 *         Y' = the same expression on the scaled v
 *         record.clamped += 1;  record.removed = record.removed + (Y - Y');  record.largest = fmaxf(record.largest, Y);  Y = Y'
 *     then the Kahan add of v into the sensor and, with statistics on, the Welford step on Y, both as without a clamp.
 * A generated NaN (infinity x 0 when an infinite sample is clamped, infinity - infinity) has no specified sign or payload: where
 * the rule yields a NaN, only THAT it is one is defined.
 *
 * Consequences.
 *   - The statistics are those of the samples as the sensor received them: the noise records of a clamped render are the Welford
 *     steps over the clamped samples' luminances.
 *   - Without DROP_NONFINITE a NaN sample is added as before (NaN > limit is false), and an infinite one is "clamped" into NaNs.
 *   - A sample of negative luminance is never touched; nor is one whose components are non-finite but whose Y is finite and
 *     <= limit (the test is on Y alone).
 *   - Directly visible emitters are clamped like everything else: the sensor receives only a sample's total.
 *   - `limit` is in the un-normalised units of slrhip_sample_luminance (not divided by the pass count).  For an image tone-mapped
 *     with `scale`, the displayed value of a sample is scale x Y.
 *   - The clamp is BIASED: it removes energy, record.removed per pixel.  It trades that bias for variance; choose the limit well
 *     above what a converged pixel of the scene shows.
 *   - The rule reads (pixel, pass) samples alone, in pass order, so the frame, the noise records and the clamp records keep every
 *     invariant of the unclamped ones: they do not depend — in any bit — on the slot count, the shard split, the result windows,
 *     how the passes are cut into calls (ascending), the tail kernel or scheduling.  A multi-rank host needs no exchange.
 *   - A render that does not call slrhip_clamp_begin launches the kernels it launched before and produces the same bits.        */
#define SLRHIP_CLAMP_DROP_NONFINITE 1u     /* slrhip_clamp_desc::flags                                                         */
typedef struct slrhip_clamp_desc {
    float    limit;        /* > 0; INFINITY: clamp nothing (with DROP_NONFINITE: "drop only")                              */
    uint32_t flags;        /* SLRHIP_CLAMP_DROP_NONFINITE or 0                                                             */
    uint32_t reserved[2];  /* 0                                                                                            */
} slrhip_clamp_desc;
/* Switches the clamp on for the render that slrhip_render_begin just began: after slrhip_render_begin and before that render's
 * first render call, the contract of slrhip_statistics_begin (later: SLRHIP_ERR_INVALID_ARGUMENT, the render goes on untouched;
 * before slrhip_render_begin: SLRHIP_ERR_NO_SCENE).  Independent of statistics: with or without them, in either order.  A second
 * call before the first render replaces the first's limit and flags.  SLRHIP_ERR_INVALID_ARGUMENT for a null argument, a NaN or
 * non-positive limit, unknown flag bits or a nonzero `reserved`; a refused call changes nothing.  Allocates one 16-byte record
 * per pixel of the shard, {uint32 clamped, uint32 dropped, float removed, float largest}, and the summary's partials; they are
 * kept for later renders and freed with the context, and a failed allocation (SLRHIP_ERR_HIP) leaves the clamp off and the render
 * usable.  The records are cleared in stream order by the first clamp-aware call that follows (render, resolve, summary), on that
 * call's stream.  Every slrhip_render_begin switches the clamp off again.                                                     */
int slrhip_clamp_begin(slrhip_ctx* ctx, const slrhip_clamp_desc* desc);

/* Channels of slrhip_resolve_clamp / slrhip_read_clamp (ONE bit per call), each [height][width] float32:                    */
#define SLRHIP_CLAMP_CLAMPED  1u   /* samples of the pixel that were scaled down, as float                                     */
#define SLRHIP_CLAMP_DROPPED  2u   /* samples of the pixel that were replaced by zero, as float                                */
#define SLRHIP_CLAMP_REMOVED  4u   /* luminance taken away from the pixel: the float32 sum, in pass order, of Y - Y'           */
#define SLRHIP_CLAMP_LARGEST  8u   /* largest luminance a clamped sample of the pixel came with (0: none was clamped)          */
#define SLRHIP_CLAMP_ALL     15u
/* One channel into DEVICE memory / HOST memory: pointer, alignment, size, zero-fill and blocking rules are those of
 * slrhip_resolve_statistics / slrhip_read_statistics, so the channels of shards add up to the whole frame's.
 * SLRHIP_ERR_INVALID_ARGUMENT when the clamp is off, when `channel` is not exactly one SLRHIP_CLAMP_* bit, or when the
 * destination is null, misaligned (4 bytes) or too small; SLRHIP_ERR_NO_SCENE before slrhip_render_begin.                     */
int slrhip_resolve_clamp(slrhip_ctx* ctx, uint32_t channel, float* device_dst, size_t num_floats, void* stream);
int slrhip_read_clamp(slrhip_ctx* ctx, uint32_t channel, float* host_dst, size_t num_floats);

/* Totals over the pixels of the shard.  clamped, dropped and removed ADD over shards, largest takes the larger.  `removed` is the
 * sum in double of the pixels' float32 REMOVED values in a FIXED order, that of slrhip_statistics_summary.  With the shard's
 * pixels p = 0 .. P-1 in the order of its pixel list, and x[p] = 0 for p >= P:
 *     block b = 0 .. ceil(P / 4096) - 1, thread t = 0 .. 255:   a[b][t] = (..((0 + x[4096 b + t]) + x[4096 b + 256 + t]) + ..) + x[4096 b + 3840 + t]
 *     per wave w = 0..3 of a block, over its 64 threads:        for off = 32, 16, 8, 4, 2, 1:  a[t] = a[t] + a[t + off]  for t < off
 *     per block:                                                 B[b] = ((a[0] + a[64]) + a[128]) + a[192]   (the waves' results)
 *     removed = (..((0 + B[0]) + B[1]) + ..)
 * so the value can be restated exactly.  Two calls on the same state return the same bits.                                    */
struct slrhip_clamp_summary {
    uint64_t clamped;                 /* sum of CLAMPED                                               */
    uint64_t dropped;                 /* sum of DROPPED                                               */
    double removed;                   /* sum of REMOVED, in the order above                           */
    float largest;                    /* largest LARGEST                                              */
    uint32_t reserved;
};                                    /* 32 bytes */
/* Fills *host_out (HOST memory) in order on `stream`; waits for that stream only, not for the device.  Allocates nothing.
 * SLRHIP_ERR_INVALID_ARGUMENT when the clamp is off; SLRHIP_ERR_NO_SCENE before slrhip_render_begin.                          */
int slrhip_clamp_summary(slrhip_ctx* ctx, struct slrhip_clamp_summary* host_out, void* stream);

/* The rule on ONE sample, on the host, with the very function the kernels call: `in` and `out` hold `components` (3 or 16) floats
 * and may be the same array; *y_in receives Y of the sample as given, *y_out that of the sample as the sensor would receive it
 * (either may be NULL).  Returns 0 (kept), 1 (clamped) or 2 (dropped); -1 for another component count or a null `in` / `out`
 * (nothing is written).  `limit` and `flags` are taken as they are, unchecked.  Pure function; no GPU is touched.               */
int slrhip_clamp_sample(int32_t components, const float* in, float limit, uint32_t flags, float* out, float* y_in, float* y_out);

/* ---- denoising: a variance-guided, edge-avoiding a-trous filter on device buffers --------------------------------------------
 * The feature buffers, the noise records and the mean frame above are the inputs of a denoiser; this is the denoiser: the 5 x 5
 * B3-spline a-trous wavelet filter with the edge-stopping weights of SVGF (normal, distance, luminance over the local standard
 * deviation), `iterations` passes with the tap distance doubling.  It is a PURE FUNCTION OF THE CALLER'S DEVICE BUFFERS: it never
 * reads the render state, needs no scene and no slrhip_render_begin; the context only names the device and owns the scratch.
 *
 * The definition.  Everything is float32, every operation IEEE-rounded on its own (no fused multiply-add), no transcendental
 * function; sqrtf and division are the correctly rounded ones.  p, q are pixels, C = components.
 *   Guides, once per call.  hit_p = coverage != NULL && coverage_p > 0.  For a hit pixel, with `normal` given:
 *     len = sqrtf((Nx*Nx + Ny*Ny) + Nz*Nz);  n_p = N / len component-wise (by division) if len > 0, else (0, 0, 0);
 *   with `distance` given: z_p = distance_p / coverage_p.
 *   Luminance.  Y(c) = the expression of slrhip_sample_luminance on the pixel's C components.
 *   Iterations.  Iteration i = 0 .. iterations - 1 has the step s = 2^i and the input (c, v), colour and variance:
 *     c_0 = color;  v_0 = variance, or all zeros if variance is NULL.
 *   Taps.  h = {1/16, 1/4, 3/8, 1/4, 1/16}, indexed by d + 2.  The taps of the centre p = (x, y) are q = (x + dx*s, y + dy*s);
 *     dy is the OUTER loop from -2 to 2, dx the INNER loop from -2 to 2, and all sums below add in that order, starting from 0.0f.
 *     A tap is skipped if it lies outside the image or if hit_q != hit_p.
 *   Centre tap (dx = dy = 0): w = h[2]*h[2], unconditionally.
 *   Other taps: w = ((h[dx+2]*h[dy+2]) * w_n) * w_z * w_l, evaluated left to right, with
 *     w_n = 1 if normal is NULL or !hit_p; else t = fmaxf(0.0f, (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z), then t = t*t repeated
 *           normal_power_log2 times, and w_n = t;
 *     w_z = 1 if distance is NULL, sigma_distance <= 0 or !hit_p; else d = (float)(s * max(|dx|, |dy|)),
 *           x = fabsf(z_p - z_q) / ((sigma_distance * d) * z_p), t = fmaxf(0.0f, 1.0f - x), w_z = t*t;
 *     w_l = 1 if variance is NULL or sigma_luminance <= 0; else x = fabsf(Y(c_p) - Y(c_q)) / (sigma_luminance * sd_p + 1e-20f),
 *           t = fmaxf(0.0f, 1.0f - x), w_l = t*t;
 *     sd_p = sqrtf(fmaxf(0.0f, vbar_p)), vbar_p = the 3 x 3 prefilter of this iteration's v at p: weights
 *           g = {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; 1/16, 1/8, 1/16} at offsets of ONE pixel for every s, in-image taps only, in row-major
 *           order: vbar = (sum g v_q) / (sum g).
 *     A tap whose weight w is 0 adds nothing to any sum (its colour is not read).
 *   Output of the iteration: c'_p[k] = (sum w * c_q[k]) / W with W = sum w;  v'_p = (sum (w*w) * v_q) / (W*W).
 *   The last iteration's c' goes to `output`, its v' to `output_variance`.
 * Consequences.  fmaxf(0, NaN) is 0, so a tap with a NaN guide, a NaN luminance or a zero or NaN denominator gets weight 0.  With
 * the luminance stop on, a non-finite pixel stays where it is: it is the centre of its own filter only, and W >= 9/64 always.  With
 * the luminance stop off a NaN or an infinity SPREADS to every pixel whose taps reach it.  Pixels that miss everything (environment,
 * background) are filtered among themselves, by luminance alone.  A pixel with v = 0 merges only with taps of exactly equal
 * luminance.  Each pixel's sums are formed by one thread in the stated order: the result does not depend on scheduling.
 *
 * The call.  All pointers are DEVICE pointers, 4-byte aligned.  The inputs are the channels exactly as the resolve calls write them
 * (SUMS for the features, means for the colour), so a multi-GPU host reduces the shards' five buffers and denoises on the root with
 * no extra pass.  Ordered on `stream`, non-blocking, copies nothing to the host.  The scratch, slrhip_denoise_scratch_bytes bytes
 * = width * height * (32 + 2 * (components == 3 ? 16 : 64)) (one 16-byte guide record and two 8-byte {Y, v} records per pixel, two
 * colour planes of float4s), is allocated by the first call and by any call that needs more, kept, and freed with the context; a call
 * that fits the scratch it finds allocates nothing.  The denoise calls of one context go on one stream, or the caller synchronises
 * between them: they share the scratch.
 * SLRHIP_ERR_INVALID_ARGUMENT, with nothing written: a null context or descriptor; a zero size or width * height >= 2^31; a null
 * or misaligned color or output, another misaligned pointer; components other than 3 or 16; iterations outside 1 .. 8;
 * normal_power_log2 > 7; a nonzero `reserved`; a NaN sigma; normal or distance without coverage; output or output_variance
 * overlapping any input or each other (byte ranges).  A failed allocation: SLRHIP_ERR_OUT_OF_MEMORY, the context stays usable.   */
typedef struct slrhip_denoise_desc {
    uint32_t width, height;       /* >= 1 each; width * height < 2^31 */
    uint32_t components;          /* 3 or 16 (the two modes; the luminance is defined for these) */
    uint32_t iterations;          /* 1 .. 8: iteration i uses step 2^i */
    const float* color;           /* [H][W][C] per-pixel MEANS (slrhip_resolve_framebuffer_mean, or sum / spp) */
    const float* variance;        /* [H][W] variance of the mean luminance (SLRHIP_STATISTICS_VARIANCE_OF_MEAN), or NULL */
    const float* normal;          /* [H][W][3] SUM of shading normals (SLRHIP_FEATURE_SHADING_NORMAL as resolved), or NULL */
    const float* distance;        /* [H][W] SUM of distances (SLRHIP_FEATURE_DISTANCE as resolved), or NULL */
    const float* coverage;        /* [H][W] SLRHIP_FEATURE_COVERAGE; required when normal or distance is given, else may be NULL */
    float* output;                /* [H][W][C] */
    float* output_variance;       /* [H][W] the filtered variance, or NULL */
    float sigma_luminance;        /* > 0: luminance stop in standard deviations (SVGF uses 4); <= 0 or variance NULL: off */
    float sigma_distance;         /* > 0: accepted relative change of distance per pixel of offset; <= 0 or distance NULL: off */
    uint32_t normal_power_log2;   /* 0 .. 7: the normal weight is max(0, n.n')^(2^k), by k squarings (SVGF: 7) */
    uint32_t reserved;            /* 0 */
} slrhip_denoise_desc;
int    slrhip_denoise(slrhip_ctx* ctx, const slrhip_denoise_desc* desc, void* stream);
size_t slrhip_denoise_scratch_bytes(uint32_t width, uint32_t height, uint32_t components);  /* pure; 0 for invalid arguments */

/* ---- image export on the device: linear floats -> 8-bit pixels ------------------------------------------------------------------
 * The last step of render -> mean -> denoise -> image without a read-back of floats: the pixel pipeline of slrhip_tonemap_bgr8 below
 * (ImageSensor::saveImage, ImageSensor.cpp:138-186) as a kernel over the caller's device buffers.  Like the denoiser it is a PURE
 * FUNCTION OF THE CALLER'S DEVICE BUFFERS: it reads nothing of the render state, needs no scene and no slrhip_render_begin; the
 * context only names the device.
 *
 * The definition, per pixel, C = components.  Every operation is float32 and IEEE-rounded on its own (no fused multiply-add),
 * except the steps marked double, whose operands are converted to double, whose operations are IEEE double operations evaluated
 * left to right, and whose result is rounded to float once.
 *   C = 3:   RGB[k] = p[k] * scale.
 *   C = 16:  X = Y = Z = 0.0f;  for b = 0 .. 15 in ascending order: v = p[b] * scale;  X += xbar[b] * v;  Y += ybar[b] * v;
 *            Z += zbar[b] * v  (the three tables and integralCMF of DiscretizedSpectrum, 16 bins);  X /= integralCMF, Y, Z likewise;
 *            double:  R = 3.2404542 * X - 1.5371385 * Y - 0.4985314 * Z;   G = -0.9692660 * X + 1.8760108 * Y + 0.0415560 * Z;
 *                     B = 0.0556434 * X - 0.2040259 * Y + 1.0572252 * Z.
 *   Clamp:   RGB[k] = RGB[k] < 0 ? 0 : RGB[k]  (a NaN stays).
 *   Tone:    double:  Y = 0.222485 * R + 0.716905 * G + 0.060610 * B;
 *            e = (float)exp((double)(-Y));   scaleY = Y != 0 ? (1.0f - e) / Y : 0.0f;   v[k] = fminf(scaleY * RGB[k], 1.0f).
 *   Gamma:   g[k] = v[k] <= 0.0031308 (compared in double) ? (float)(12.92 * v[k]) : (float)(1.055 * pow((double)v[k], 1.0 / 2.4) - 0.055),
 *            both in double.
 *   Byte:    (uint8_t)(256 * fminf(g[k], 0.999f)), the product in float, truncated.
 * exp and pow are the only library calls, and the only places where two implementations of this definition can differ in a last
 * bit (slrhip_tonemap_bgr8 calls the host's expf and pow).  Consequence: an output byte can differ from slrhip_tonemap_bgr8's only
 * where the un-truncated value 256 * fminf(g[k], 0.999f) lies within rounding distance of an integer.
 * Non-finite and negative values come out as the host function gives them (fminf returns its other operand for a NaN): a pixel with
 * a NaN in any component, or with +infinity in every component, is 255 in every channel; a channel that is +infinity next to finite
 * ones is 255 and the finite ones are 0 (C = 3); a negative RGB channel is 0; an all-zero pixel is 0.
 *
 * Formats.  Both run the same arithmetic.
 *   SLRHIP_IMAGE_BGR8_BMP  bottom-up rows (image row i is output row height - 1 - i) of 3 * width + width % 4 bytes, B G R per pixel,
 *                          the padding bytes 0: byte for byte what slrhip_tonemap_bgr8 fills and slrhip_save_bmp takes.
 *   SLRHIP_IMAGE_RGBA8     top-down rows of 4 * width bytes, R G B 255: a display surface, a uint8 tensor [H][W][4].
 *
 * The call.  Ordered on `stream`, non-blocking; it allocates nothing, copies nothing and does not synchronise, so it can be captured
 * into a graph from the first call on.  It writes exactly slrhip_tonemap_bytes(width, height, format) bytes, padding included, and
 * nothing beyond them.  Any `scale` is accepted, as slrhip_tonemap_bgr8 accepts it.
 * SLRHIP_ERR_INVALID_ARGUMENT, with nothing written: a null context, descriptor, color or output; a misaligned pointer (4 bytes); a
 * zero size or width * height >= 2^31; components other than 3 or 16; an unknown format; a nonzero `reserved`; output_bytes less
 * than slrhip_tonemap_bytes; output overlapping color (byte ranges).                                                              */
#define SLRHIP_IMAGE_BGR8_BMP 0u
#define SLRHIP_IMAGE_RGBA8    1u
typedef struct slrhip_tonemap_desc {
    uint32_t width, height;       /* >= 1 each; width * height < 2^31 */
    uint32_t components;          /* 3 or 16 */
    uint32_t format;              /* SLRHIP_IMAGE_* */
    const float* color;           /* DEVICE [H][W][C]; 4-byte aligned */
    uint8_t* output;              /* DEVICE; 4-byte aligned */
    size_t output_bytes;          /* room at output; at least slrhip_tonemap_bytes(width, height, format) */
    float scale;                  /* as slrhip_tonemap_bgr8's: brightness / samples x sensitivity for a frame of sums */
    uint32_t reserved;            /* 0 */
} slrhip_tonemap_desc;
int    slrhip_tonemap(slrhip_ctx* ctx, const slrhip_tonemap_desc* desc, void* stream);
size_t slrhip_tonemap_bytes(uint32_t width, uint32_t height, uint32_t format);   /* pure; 0 for invalid arguments */

/* ---- albedo demodulation: divide a frame by the albedo, multiply it back -------------------------------------------------------------
 * The denoiser's luminance stop cannot tell a texture edge from noise.  The cure: divide the frame by the first-hit albedo
 * (slrhip_resolve_albedo), filter the smooth irradiance (slrhip_denoise), multiply back.  Like the denoiser and the image export this is a
 * PURE FUNCTION OF THE CALLER'S DEVICE BUFFERS: it reads nothing of the render state, needs no scene and no slrhip_render_begin; the
 * context only names the device.
 *
 * The definition, per pixel, C = components.  Everything is float32, every operation IEEE-rounded on its own (no fused multiply-add).
 *   a[k] = fmaxf(albedo[k] / (float)albedo_passes, floor)        (fmaxf returns its other operand for a NaN: a NaN albedo becomes floor)
 *   ya   = Y(a), the expression of slrhip_sample_luminance on the C values a[k]
 *   SLRHIP_MODULATE_DIVIDE:    output[k] = color[k] / a[k];   output_variance = variance / (ya * ya)
 *   SLRHIP_MODULATE_MULTIPLY:  output[k] = color[k] * a[k];   output_variance = variance * (ya * ya)
 * `variance` is the variance of a luminance (SLRHIP_STATISTICS_VARIANCE_OF_MEAN, slrhip_denoise's output_variance): it is scaled by
 * the square of the albedo's luminance, which is exact for a grey albedo.
 *
 * The call.  All pointers are DEVICE pointers, 4-byte aligned.  Ordered on `stream`, non-blocking; it allocates nothing, copies nothing
 * and does not synchronise, so it can be captured into a graph from the first call on.  `output` may be exactly `color`, and
 * `output_variance` exactly `variance` (in place); any other overlap of an output with a buffer of the call is refused.
 * SLRHIP_ERR_INVALID_ARGUMENT, with nothing written: a null context or descriptor; a zero size or width * height >= 2^31; components
 * other than 3 or 16; an unknown op; albedo_passes == 0; a floor that is not finite or <= 0; a nonzero `reserved`; a null color,
 * albedo or output; a misaligned pointer; output_variance without variance; an output that overlaps another buffer (byte ranges) other
 * than being exactly equal to its own input.                                                                                       */
#define SLRHIP_MODULATE_DIVIDE   0u
#define SLRHIP_MODULATE_MULTIPLY 1u
typedef struct slrhip_modulate_desc {
    uint32_t width, height;       /* >= 1 each; width * height < 2^31 */
    uint32_t components;          /* 3 or 16 */
    uint32_t op;                  /* SLRHIP_MODULATE_* */
    const float* color;           /* [H][W][C] */
    const float* variance;        /* [H][W] variance of the mean luminance, or NULL */
    const float* albedo;          /* [H][W][C] SUMS as slrhip_resolve_albedo writes them */
    float* output;                /* [H][W][C]; may be exactly `color` */
    float* output_variance;       /* [H][W] or NULL; may be exactly `variance` */
    uint32_t albedo_passes;       /* >= 1: the divisor of the albedo sums (slrhip_resolve_albedo's *passes) */
    float floor;                  /* > 0, finite: the smallest albedo a pixel is divided by */
    uint32_t reserved;            /* 0 */
} slrhip_modulate_desc;
int slrhip_modulate(slrhip_ctx* ctx, const slrhip_modulate_desc* desc, void* stream);

/* ---- temporal reprojection: blend the current frame into the previous frame's history --------------------------------------------------
 * slrhip_denoise is the spatial half of SVGF; this is the temporal half.  The previous frame's accumulated colour is fetched along the
 * motion vectors (slrhip_resolve_motion), tested against the current frame's guides, and blended with the current frame with a weight
 * that falls with the length of the history.  Like the denoiser it is a PURE FUNCTION OF THE CALLER'S DEVICE BUFFERS: it reads nothing
 * of the render state, needs no scene and no slrhip_render_begin; the context only names the device.
 *
 * The definition, per pixel p = (x, y), C = components.  Everything is float32, every operation IEEE-rounded on its own (no fused
 * multiply-add), IEEE division and square root, floorf exact.
 *   Rejected:  p is rejected if coverage_p <= 0 or n = motion_p.w <= 0 (no sample of the pixel has a vector; the environment is out of scope).
 *   Position:  m = (motion_p.x / n, motion_p.y / n);  z_e = motion_p.z / n, the distance expected in the previous frame;
 *              fx = (float)x + m.x;  x0 = floorf(fx);  tx = fx - x0;  y likewise.  The pixel centre is x + 0.5 and the bilinear footprint
 *              of a position u starts at floorf(u - 0.5): the + 0.5 and the - 0.5 cancel.
 *   Taps:      q = (x0 + (float)i, y0 + (float)j), the sums in float32; j is the OUTER loop and i the INNER loop over {0, 1}, and every sum
 *              below adds in that order, starting from 0.0f.  b = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty).  A tap with b == 0 adds
 *              nothing and is not read.
 *   Validity:  a tap q is valid if ALL of these hold:
 *                it lies inside the image (0 <= q.x < width, 0 <= q.y < height; false for a NaN);
 *                prev_coverage_q > 0;  prev_length_q > 0;
 *                with ids: ids_p[1] == prev_ids_q[1] and ids_p[2] == prev_ids_q[2] (instance and material; triangle indices differ
 *                  between neighbours by design);
 *                with sigma_distance > 0: fabsf(prev_distance_q / prev_coverage_q - z_e) <= sigma_distance * z_e;
 *                with normals: (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >= min_normal_dot, n_p from normal_p and n_q from prev_normal_q as
 *                  slrhip_denoise normalises: len = sqrtf((Nx Nx + Ny Ny) + Nz Nz); N / len component-wise (by division) if len > 0,
 *                  else (0, 0, 0);
 *                Y(prev_color_q), the expression of slrhip_sample_luminance on the tap's C components, is finite (fabsf(Y) <= FLT_MAX):
 *                  a NaN or an infinity does not live on in the history.
 *   History:   B = sum b over the valid taps.  If B <= 0 the pixel is rejected.  Otherwise hist[k] = (sum b * prev_color_q[k]) / B,
 *              len = (sum b * prev_length_q) / B, vhist = (sum b * prev_variance_q) / B.
 *   Blend:     N = fminf(len + 1.0f, max_history);  a = fmaxf(1.0f / N, min_alpha);
 *              output[k] = (1.0f - a) * hist[k] + a * color[k];  output_length = N;
 *              output_variance = (a * a) * variance_p + ((1.0f - a) * (1.0f - a)) * vhist.
 *   Rejected:  output[k] = color[k];  output_length = 1;  output_variance = variance_p.
 * Each pixel's sums are formed by one thread in the stated order: the result does not depend on scheduling.  The history length is a
 * float plane so that it is fetched like the colour; a fresh sequence starts from prev_length = 0 everywhere.
 *
 * The call.  All pointers are DEVICE pointers, 4-byte aligned.  The current frame's inputs are the channels exactly as the resolve calls
 * write them (SUMS for motion, coverage, distance, normal; means for the colour); the previous frame's are what the caller KEPT of the
 * previous frame: its `output` and `output_length` of this call (or of what followed it), its coverage, distance, ids, normal.  Ordered on
 * `stream`, non-blocking; it allocates nothing, copies nothing and does not synchronise, so it can be captured into a graph from the
 * first call on.  The gather reads neighbours of the previous frame, so there is no in-place mode.
 * SLRHIP_ERR_INVALID_ARGUMENT, with nothing written: a null context or descriptor; a zero size or width * height >= 2^31; components
 * other than 3 or 16; a null color, motion, coverage, prev_color, prev_length, prev_distance, prev_coverage, output or output_length;
 * a misaligned pointer (4 bytes); prev_variance without variance or variance without prev_variance, likewise ids / prev_ids and
 * normal / prev_normal; output_variance without variance; a NaN max_history, min_alpha, sigma_distance or min_normal_dot;
 * max_history < 1; min_alpha outside [0, 1]; a nonzero `reserved`; any output overlapping any input or another output (byte ranges).
 * Not covered: reprojecting the environment under camera rotation (a pixel without a hit is rejected and starts again); motion of loose
 * triangles (slrhip_render_motion takes them to stand still); moment-based temporal variance (the variance is blended, not estimated
 * from the history's moments); bench.py, the C++ host mirror and the libSLR adapter (the motion pass and this call are reached through
 * this header and the Python binding only).                                                                                       */
typedef struct slrhip_reproject_desc {
    uint32_t width, height;       /* >= 1 each; width * height < 2^31 */
    uint32_t components;          /* 3 or 16 */
    /* the current frame */
    const float* color;           /* [H][W][C] per-pixel MEANS */
    const float* variance;        /* [H][W] variance of the mean luminance, or NULL */
    const float* motion;          /* [H][W][4] as slrhip_resolve_motion writes it */
    const float* coverage;        /* [H][W] SLRHIP_FEATURE_COVERAGE */
    const uint32_t* ids;          /* [H][W][3] SLRHIP_FEATURE_IDS, or NULL */
    const float* normal;          /* [H][W][3] SUM of shading normals, or NULL */
    /* the previous frame */
    const float* prev_color;      /* [H][W][C] the accumulated history */
    const float* prev_variance;   /* [H][W], or NULL (required if and only if variance is given) */
    const float* prev_length;     /* [H][W] history length, as float; 0 = no history */
    const float* prev_distance;   /* [H][W] SUM of distances */
    const float* prev_coverage;   /* [H][W] */
    const uint32_t* prev_ids;     /* [H][W][3]; required if and only if ids is given */
    const float* prev_normal;     /* [H][W][3]; required if and only if normal is given */
    /* outputs */
    float* output;                /* [H][W][C] */
    float* output_variance;       /* [H][W], or NULL; needs variance */
    float* output_length;         /* [H][W] */
    float max_history;            /* >= 1: the history length is capped here (a = 1 / N never falls below 1 / max_history) */
    float min_alpha;              /* 0 .. 1: the least weight of the current frame */
    float sigma_distance;         /* > 0: accepted relative difference of a tap's distance from z_e; <= 0: the test is off */
    float min_normal_dot;         /* a tap needs n_p . n_q >= this; used only with normals */
    uint32_t reserved[2];         /* 0 */
} slrhip_reproject_desc;
int slrhip_reproject(slrhip_ctx* ctx, const slrhip_reproject_desc* desc, void* stream);

/* ---- the environment light from device memory ----------------------------------------------------------------------------------------
 * Replaces or adds the environment sphere of the UPLOADED scene from texels that are already on the device, and leaves everything else
 * of the scene as it is: no descriptor check, no tree build, no table copied again.  The importance map (slrhip_envmap::importance) and
 * the sampling tables are built where the texels are.
 *
 * The contract.  From the call on the context renders exactly what a fresh slrhip_upload_scene of the same description renders with
 *   env = {width, height, texels, scale, width / 4, height / 4, slrhip_env_importance(texels)}
 * where `texels` are the texels as STORED (below): the frame, the counters and every later call match in every bit.  The definitions are
 * the reference's and are stated once, for host and device, in slr_amd/csrc/pt_envmap.h; all float32, every operation IEEE-rounded on its
 * own, except where double is stated:
 *   importance : a map cell is a 4x4 block of texels.  Per component, Image2D::areaAverage (Core/Image.cpp:19-120): a compensated sum
 *                (s = 0, comp = 0; per texel: val = 1.0f * texel; ci = val - comp; t = s + ci; comp = (t - s) - ci; s = t) over the 16
 *                texels in the order of (x, y) offsets (0,0) (3,0) (0,3) (3,3) (1,0) (1,3) (2,0) (2,3) (0,1) (3,1) (0,2) (3,2) (1,1)
 *                (2,1) (1,2) (2,2), then (float)(binary16)(s / 16.0f), round to nearest even, subnormals kept.  RGB mode
 *                (image_textures.cpp:81-108,131): Y = (0.222485f * a0 + 0.716905f * a1) + 0.060610f * a2 on the three averages.
 *                Spectral mode, averages (u, v, s): x = (float)(0.0491440520940413 u - 0.02361291916573777 v + 0.13292069743203658),
 *                y = (float)(0.022853819546830627 u + 0.05077639329371236 v - 0.006895157122499944) in double; X = x s, Y = y s,
 *                Z = (s - X) - Y; XYZ_to_sRGB (Spectrum.h:59-64) in double rounded to float; the same luminance.
 *   tables     : row[x] = (float)(sinRow[y] * (double)importance[y][x]) with the DOUBLE sinRow[y] = sin(M_PI * (y + 0.5f) / map_height),
 *                evaluated on the host and copied (at most 64 KiB); RegularConstantContinuous1D (Core/distributions.cpp:127-147) over
 *                each row and then over the rows' integrals: a sequential float32 Kahan sum of PDF[i] / n in index order, then PDF[i]
 *                and CDF[i + 1] divided by the total.  This is what slrhip_upload_scene does with the importance it is given.
 *   STORED     : the library COPIES the texels into its own array; the caller's buffer is free once the stream has passed the call.
 *                SLRHIP_ENV_STORE_HALF rounds every component as given to binary16 first; then, in a SPECTRAL context,
 *                SLRHIP_ENV_TEXELS_RGB converts every texel (r, g, b) -> (u, v, s) as slrhip_env_texels_to_uvs does.
 *
 * Ordering.  The work is ordered on `stream`.  slrhip_render blocks until its passes are done, so no render is in flight when the call is
 * made; feature, albedo and query calls never read the environment.  The accumulation is not touched: samples rendered after the call
 * see the new light, and a caller who wants a clean frame calls slrhip_render_begin.
 *
 * Graphs and allocation.  The call is NOT capturable in a graph: it copies sinRow from the host and may allocate.  It allocates only
 * when the map is larger than what the context holds, and it allocates the new arrays BEFORE it lets go of the old ones: a failed
 * allocation returns SLRHIP_ERR_OUT_OF_MEMORY and leaves the previous environment rendering as before.  The importance map stays on the
 * device (width / 4 x height / 4 floats) for slrhip_debug_environment.
 *
 * Errors.  SLRHIP_ERR_INVALID_ARGUMENT, with nothing changed: a null context or descriptor; a width or height that is not a multiple
 * of 4 in 4 .. 32768; a null or misaligned (16 bytes) `texels`; unknown flag bits; a nonzero `reserved`; a NaN, infinite or negative
 * `scale`.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.  SLRHIP_ERR_UNSUPPORTED in a SPECTRAL context whose scene was uploaded
 * without slrhip_scene_desc::upsampling (a scene without environment or image textures may name the tables for this purpose).       */
#define SLRHIP_ENV_TEXELS_RGB 1u   /* the texels are linear (r,g,b) radiance; a SPECTRAL context converts them per texel to (u,v,s)
                                    * (slrhip_env_texels_to_uvs); an RGB context ignores the bit                                  */
#define SLRHIP_ENV_STORE_HALF 2u   /* round every component of the texels as given to binary16 first, as the reference's RGBA16F
                                    * image would hold them (beyond 65504: infinity, as there)                                    */
typedef struct slrhip_environment_desc {
    uint32_t width, height;        /* multiples of 4, 4 .. 32768; the importance map is width/4 x height/4 */
    const float* texels;           /* DEVICE, [height][width][3], 16-byte aligned; without TEXELS_RGB: what slrhip_envmap::texels holds for the mode */
    float scale;                   /* slrhip_envmap::scale */
    uint32_t flags;                /* SLRHIP_ENV_* */
    uint32_t reserved[2];          /* 0 */
} slrhip_environment_desc;
int slrhip_set_environment(slrhip_ctx* ctx, const slrhip_environment_desc* desc, void* stream);

/* The same preprocessing on the HOST (pure; no device is touched), with the functions the kernels call.
 * importance[(height/4)][(width/4)] = what slrhip_envmap::importance must hold for `texels` ([height][width][3]; mode RGB: (r,g,b),
 * mode SPECTRAL: (u,v,s)).  width, height: multiples of 4, 4 .. 32768.  num_floats: room at importance.                      */
int slrhip_env_importance(int32_t mode, const float* texels, uint32_t width, uint32_t height, float* importance, size_t num_floats);
/* (r,g,b) -> (u,v,s) as the spectral build stores an RGB image (Upsampling::sRGB_to_uvs, Illuminant, BasicTypes/Spectrum.h:148-171;
 * x = y = (float)(1.0 / 3.0) for a black texel), binary16-rounded; rgb and uvs may be the same array.
 * Both return SLRHIP_ERR_INVALID_ARGUMENT, with nothing written, for a null pointer, a size that is not a multiple of 4 or is out of
 * range, another mode, or too little room.                                                                                          */
int slrhip_env_texels_to_uvs(const float* rgb, size_t num_texels, float* uvs);

/* ---- moving instances and the camera without a scene upload ----------------------------------------------------------------------------
 * A second frame of the same scene with something moved: new StaticTransforms for TransformedSurfaceObjects that exist
 * (Core/SurfaceObject.cpp:303-392, Transform.h:38-87) and a new PerspectiveCamera (Cameras/PerspectiveCamera.cpp:15-24), with no
 * descriptor check, no copy of the geometry and no tree build.
 *
 * slrhip_set_instance_transforms gives the instances [first_instance, first_instance + count) of the UPLOADED scene the matrices of
 * `device_src`: DEVICE memory, 16-byte aligned, `count` records.  Both matrices are the caller's, column-major, as in slrhip_instance
 * (the reference inverts in float, so the inverse is a scene input).  Meshes, triangle ranges and the number of instances stay.
 *
 * The contract.  From the call on, the context renders, answers ray queries and fills feature buffers exactly as a fresh context does
 * that uploaded the scene with the new matrices: every bit of the frame, of the hits and of the counters.  The top-level tree keeps
 * its SHAPE and gets new child boxes (a refit on the device, bottom-up); hits do not depend on the tree's shape because the tie rule
 * among equal distances is a rule on (instance, triangle) pairs.  Speed does depend on it: after large motion the tree fits the scene
 * badly and rays visit more nodes (DESIGN.md has the measured factor); a caller for whom that matters calls
 * slrhip_rebuild_top_level (below), or uploads the scene again.
 *
 * A record is checked on the device as slrhip_upload_scene checks an instance: every entry finite, bottom rows 0 0 0 1.  A record
 * that fails leaves ITS instance exactly as it was (matrices and box), the others of the call move, and SLRHIP_INSTANCE_BAD_TRANSFORM
 * is set in a status word that slrhip_instances_status reads and clears (it waits for `stream`).
 *
 * Ordering.  The call allocates nothing, copies nothing from the host and does not synchronise; its launches are ordered on `stream`.
 * A render, query or feature pass enqueued after it on the same stream sees the new placement; the caller's buffer is free once the
 * stream has passed the call.  slrhip_render blocks until its passes are done, so no render is in flight when the call is made.
 * NOTHING accumulated is reset: the frame, the feature buffers, the albedo and the statistics since slrhip_render_begin stay, and
 * samples rendered after the call see the new placement.  Starting the new frame is the caller's slrhip_render_begin.
 *
 * Errors, synchronous, with nothing changed.  SLRHIP_ERR_INVALID_ARGUMENT: a null context or pointer, count == 0, a misaligned
 * pointer (16 bytes), a range beyond slrhip_scene_desc::num_instances.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.
 * SLRHIP_ERR_UNSUPPORTED for a scene without instances.  Not covered: adding or removing instances, instances that emit, moving
 * loose triangles (flat scenes: slrhip_set_vertices).  Repairing the top level after large motion: slrhip_rebuild_top_level.      */
#define SLRHIP_INSTANCE_BAD_TRANSFORM 1u   /* a record of a call had a non-finite entry or a bottom row other than 0 0 0 1; its instance did not move */
typedef struct slrhip_instance_transform {
    float local_to_world[16];
    float world_to_local[16];
} slrhip_instance_transform;               /* 128 B, column-major */
int slrhip_set_instance_transforms(slrhip_ctx* ctx, const slrhip_instance_transform* device_src, uint32_t first_instance, uint32_t count,
                                   void* stream);
/* The SLRHIP_INSTANCE_* bits of the calls since the last read, then cleared; waits for `stream`.  0 before any scene.              */
int slrhip_instances_status(slrhip_ctx* ctx, uint32_t* bits, void* stream);

/* The world box the top-level tree holds for an instance: the box of the eight corners of the mesh's local box [mesh_lo, mesh_hi]
 * taken through local_to_world (StaticTransform x BoundingBox3D, Transform.h:54-65), padded per axis by
 * 1e-5f * max(1, |lo|, |hi|).  On the HOST (pure), with the function the upload and the kernel call.  lo, hi: 3 floats each.        */
int slrhip_instance_world_box(const float mesh_lo[3], const float mesh_hi[3], const float local_to_world[16], float out_lo[3],
                              float out_hi[3]);

/* Replaces the camera of the UPLOADED scene: the same host arithmetic as slrhip_upload_scene's camera constants, written into the
 * context and nothing else; no device call is made.  Launches enqueued after the call see the new camera (slrhip_render,
 * slrhip_camera_rays, the feature and albedo passes); nothing accumulated is reset — starting the new frame is the caller's
 * slrhip_render_begin.  The image size is slrhip_render_begin's, so `aspect` should agree with it as it does at upload.
 * SLRHIP_ERR_INVALID_ARGUMENT for a null argument, SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.                                  */
int slrhip_set_camera(slrhip_ctx* ctx, const slrhip_camera* camera);

/* ---- repairing the top-level tree after instances have moved ---------------------------------------------------------------------------
 * slrhip_set_instance_transforms keeps the top-level tree's shape; after large motion the shape no longer fits the scene.
 * slrhip_rebuild_top_level keeps the shape too, and moves the LEAVES: the top level's primitives are sorted by the Morton code of
 * their box centres and seated in that order into the leaf slots of the tree as it stands, taken depth-first; then the refit of
 * slrhip_set_instance_transforms runs.  It is the CALLER'S decision: on a tree that has lost its fit the call repairs most of the
 * damage, on a tree that still fits it makes the tree somewhat WORSE than the upload's (INTEGRATION.md has the figures), and on a
 * tiny top level that mixes large packets of loose triangles with small instances it does not help.  slrhip_top_level_cost is the
 * read-out to decide with.
 *
 * Primitives.  A top-level primitive is a leaf child of the top-level tree: an instance leaf (count 0, index = the instance) or a
 * packet of loose triangles (count >= 1).  Their canonical order is ascending child word: the instances first, by index.  An
 * instance's box is its current world box (what slrhip_set_instance_transforms maintains); a packet's box is the box the upload
 * gave its slot (loose triangles of an instanced scene never move).
 *
 * Scene box.  Per axis the minimum of the primitives' lo and the maximum of their hi — equal to the union of the root's valid child
 * boxes, because uploads and refits keep unions exact.
 *
 * Key (slrhip_top_level_key; one definition for host and device, slr_amd/csrc/pt_toplevel.h).  float32 throughout, every operation
 * rounded on its own, IEEE division.  Per axis a:  c = (lo[a] + hi[a]) * 0.5f;  e = scene_hi[a] - scene_lo[a];
 * x = e > 0 ? (c - scene_lo[a]) / e : 0;  q = x >= 0 ? (uint32_t)fminf(floorf(x * 2097152.0f), 2097151.0f) : 0 (a NaN gives 0).
 * The key is the 63-bit interleave of the three axes: bit 3 i + 2 is bit i of q.x, bit 3 i + 1 bit i of q.y, bit 3 i bit i of q.z.
 *
 * Order.  The primitives are sorted stably by ascending key: equal keys (coincident placements) keep the canonical order.
 *
 * Slots.  The leaf slots of the top-level tree depth-first from node 0: child slots 0 .. 3 in order, an inner child's whole subtree
 * before the next slot.  Inner child words never change, so the slot table is fixed per upload.
 *
 * Seating.  Slot i receives primitive order[i]: its child word and its six planes.  Then every inner child box of the top level is
 * refitted bottom-up, by the rule and the launches of slrhip_set_instance_transforms.
 *
 * What stays: the number of top-level nodes, the level table, slrhip_counters::bvh_nodes and bvh_depth, every inner child word and
 * pad word, every node of the mesh trees, the instance records, the instance and mesh boxes, the triangle records and every
 * pointer the kernels hold.  Only leaf child words and child planes of the top-level nodes are written.  The result is a pure
 * function of the primitives' boxes: a second call with nothing moved in between changes no bit.  slrhip_set_instance_transforms
 * keeps working after the call, and its refit then runs over the new arrangement.
 *
 * Behaviour.  Hits do not depend on the tree's shape.  From the call on the context renders, answers slrhip_intersect_rays /
 * slrhip_test_visibility and fills feature buffers exactly as before the call, and as a fresh context does that uploaded the
 * current placements: every bit of the frame, of the hits and of the counters.  Only speed changes.  Nothing accumulated is reset.
 *
 * Ordering.  The FIRST call after a slrhip_upload_scene reads the top level back once, builds the slot table, the canonical
 * references and the packets' boxes on the host and allocates what the calls need (those tables, keys, order, the sort's
 * temporary storage): it synchronises and cannot be captured.  Every LATER call allocates nothing, copies nothing from the host
 * and does not synchronise; its launches are ordered on `stream` (two to a handful: at most SLRHIP_TOP_SEAT_GROUP primitives are
 * sorted and seated by one launch of one workgroup, more by a key launch, a device radix sort and a seat launch; the refit's
 * launches follow).  slrhip_upload_scene drops the state.
 *
 * Errors, synchronous, with nothing changed.  SLRHIP_ERR_INVALID_ARGUMENT: a null context.  SLRHIP_ERR_NO_SCENE before
 * slrhip_upload_scene.  SLRHIP_ERR_UNSUPPORTED ("the scene has no instances") for a flat scene.  Not covered: another node count
 * (a rebuild of the SHAPE), adding or removing instances, the mesh trees.                                                        */
#define SLRHIP_TOP_SEAT_GROUP 4096u
int slrhip_rebuild_top_level(slrhip_ctx* ctx, void* stream);

/* The expected number of top-level nodes a random line through the root box visits, the surface-area measure of how well the top
 * level fits: 1 + (sum of the surface areas of all inner-child boxes) / (area of the root box).  Computed in double on the HOST
 * from a read-back of the top-level nodes: the sum runs in node order, then child order; a box's area is 2 (dx dy + dy dz + dz dx)
 * of max(hi - lo, 0) taken in double; the root box is the union of the root's valid children, and a root of zero area gives 1.
 * Waits for `stream`; allocates nothing on the device.  A caller compares the value before and after a move or a rebuild, or
 * against the upload's.  The refusals of slrhip_rebuild_top_level, and SLRHIP_ERR_INVALID_ARGUMENT for a null pointer.          */
int slrhip_top_level_cost(slrhip_ctx* ctx, double* host_cost, void* stream);

/* The key of the box [lo, hi] in the scene box [scene_lo, scene_hi], on the HOST (pure), with the function the kernels call.
 * SLRHIP_ERR_INVALID_ARGUMENT for a null pointer.                                                                                */
int slrhip_top_level_key(const float lo[3], const float hi[3], const float scene_lo[3], const float scene_hi[3], uint64_t* key);

/* ---- host-side construction of spectral-mode spectra ------------------------------------------------------------------ */
/* SpectrumType / ColorSpace of the reference (BasicTypes/Spectrum.h:17-35), as the scene language's Spectrum(...) passes them. */
enum { SLRHIP_SPECTRUMTYPE_REFLECTANCE = 0, SLRHIP_SPECTRUMTYPE_ILLUMINANT = 1, SLRHIP_SPECTRUMTYPE_IOR = 2 };
enum { SLRHIP_COLORSPACE_SRGB = 0, SLRHIP_COLORSPACE_SRGB_NONLINEAR = 1, SLRHIP_COLORSPACE_XYY = 2, SLRHIP_COLORSPACE_XYZ = 3 };
#define SLRHIP_UPSAMPLING_SAMPLES 95u    /* samples per data-point spectrum, 360-830 nm (Spectrum.h:197) */
/* Replaces: the UpsampledContinuousSpectrum(spType, space, e0, e1, e2) constructor (BasicTypes/SpectrumTypes.h:180-237), which
 * `Spectrum(r, g, b)` of the scene language calls (libSLRSceneGraph/API.cpp:286-441, :1139-1147): writes (u, v, scale).        */
int slrhip_upsample(int32_t spectrum_type, int32_t color_space, float e0, float e1, float e2, float uvs[3]);
/* Replaces: the (u, v)-only half of UpsampledContinuousSpectrum::evaluate (SpectrumTypes.h:241-312).  Writes the number of data
 * points (0, 3 or 4 -> slrhip_spectrum::reserved) and the 4 + 4 * SLRHIP_UPSAMPLING_SAMPLES floats of the UPSAMPLED payload. */
int slrhip_resolve_upsampled(const slrhip_upsampling_tables* tables, float u, float v, uint32_t* num_points, float* payload);

/* Replaces: Spectrum::create(spType, minLambda, maxLambda, values, n) / (spType, lambdas, values, n) of the reference's RGB build
 * (libSLRSceneGraph/API.cpp:1149-1278,1326-1369): integrates the sampled spectrum against the CIE 2-degree colour-matching
 * functions (trapezoids over the union of both sample grids, Kahan sums), normalises by integralCMF, converts XYZ -> linear sRGB
 * (type ILLUMINANT) or sRGB_E (REFLECTANCE, IOR) and clamps negative components: the `rgb` of a slrhip_spectrum of kind REGULAR
 * (lambdas == NULL; min / max wavelength given) or IRREGULAR (lambdas given), i.e. what RGB mode renders named spectra such as
 * Spectrum("ID": "D65") or the refractive-index tables with.                                                              */
int slrhip_spectrum_to_rgb(int32_t spectrum_type, const float* lambdas, float lambda_min, float lambda_max, const float* values,
                           uint32_t num_samples, float rgb[3]);

/* Host-side helpers on the float framebuffer.
 * slrhip_tonemap_bgr8: ImageSensor::saveImage (ImageSensor.cpp:138-186) pixel pipeline:
 * scale*sensitivity -> (spectral: XYZ->sRGB) -> 1-exp(-Y) tone map -> sRGB gamma -> 8-bit BGR,
 * bottom-up rows as the BMP writer stores them.                                            */
int slrhip_tonemap_bgr8(const float* framebuffer, int32_t width, int32_t height, int32_t components,
                        float scale, uint8_t* dst_bgr, size_t dst_bytes);
int slrhip_save_bmp(const char* path, const uint8_t* bgr_bottom_up, int32_t width, int32_t height);

/* ---- moving vertices without a scene upload ----------------------------------------------------------------------------------------
 * The next frame of a deforming mesh: what the reference does by building a new TriangleMesh and a new aggregate over it
 * (Surface/TriangleMesh.cpp, Core/SurfaceObject.cpp:226-250), with no descriptor check, no host tree build and no copy of any record.
 * Together with slrhip_set_camera, slrhip_set_instance_transforms and slrhip_set_environment it completes what a second frame of
 * the same scene can change without slrhip_upload_scene.
 *
 * A context created with SLRHIP_FLAG_DYNAMIC_GEOMETRY keeps, from slrhip_upload_scene on and all on the device: the scene's vertex
 * array (44 B per vertex), its triangle index array (16 B per triangle), a scratch of one box per LeafTri record (32 B each: one per
 * triangle) and, on the host, the first node of every tree level.  A 10 M-triangle grid of 5 M vertices costs 220 + 160 + 320 MB.
 *
 * slrhip_set_vertices replaces the vertices [first_vertex, first_vertex + count) of the kept array with the records at
 * `device_src`: DEVICE memory, 4-byte aligned, `count` whole slrhip_vertex records — position, normal, tangent and texcoord all take
 * effect.  Then everything that depends on vertices is rebuilt in place from the kept array, on the device: the leaf triangles
 * (v0, e1, e2), the shading records, the light records (both copies), the texture coordinates of textured scenes and of the alpha
 * records, every child box of the tree bottom-up, and the quantized nodes where they are in use.  The arithmetic is the upload's own,
 * operation for operation (one definition: slr_amd/csrc/pt_triangle.h), the NaN normal of a degenerate triangle included.  Indices,
 * materials, the light list and its distribution (every light's importance is the constant 1) stay.
 *
 * The contract.  From the call on, the context renders, answers ray queries (slrhip_intersect_rays, slrhip_test_visibility,
 * slrhip_trace_rays) and fills feature and albedo buffers exactly as a fresh context does that uploaded the scene with the kept
 * vertex array as it now stands: every bit of the frame, of the hits and of the samples / extension_rays / shadow_rays counters.
 * The tree keeps its SHAPE — child words, node order, packet order, depth; bvh_nodes, bvh_depth and build_seconds keep the upload's
 * values — and gets EXACT boxes: a packet's box is the min / max over the vertex positions of its triangles, an inner child's the
 * min / max union of the valid child boxes of the node it names, with no padding.  Hits do not depend on the tree's shape because
 * the tie rule among equal distances is a rule on (instance, triangle) pairs.  Speed does depend on it: after large deformation the
 * tree fits the scene badly and rays visit more nodes; a caller for whom that matters uploads the scene again.  Measured (DESIGN.md
 * 7.23): every vertex of the 10 M-triangle grid displaced by up to half a cell costs 1.14 - 1.16 x the nodes per ray of the tree as
 * uploaded, which is 0.95 - 0.97 x what a fresh build of the displaced scene costs — at that amplitude a rebuild buys nothing.
 *
 * A record is checked on the device: all eleven floats finite.  A record that fails leaves ITS vertex exactly as it was, the others
 * of the call move, and SLRHIP_GEOMETRY_BAD_VERTEX is set in a status word that slrhip_geometry_status reads and clears (it waits
 * for `stream`).
 *
 * Ordering, as for slrhip_set_instance_transforms.  The call allocates nothing, copies nothing from the host and does not
 * synchronise; its launches are ordered on `stream`.  No scene array is reallocated or moved, so a captured render graph stays
 * valid.  NOTHING accumulated is reset; starting the new frame is the caller's slrhip_render_begin.
 *
 * Errors, synchronous, with nothing changed.  SLRHIP_ERR_INVALID_ARGUMENT: a null context or pointer, count == 0, a misaligned
 * pointer (4 bytes), a range beyond slrhip_scene_desc::num_vertices.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.
 * SLRHIP_ERR_UNSUPPORTED: a context created without SLRHIP_FLAG_DYNAMIC_GEOMETRY, a scene with instances in a context created
 * without SLRHIP_FLAG_DYNAMIC_INSTANCED, a tree built with spatial splits (its leaf boxes are clipped and its references duplicated).
 *
 * Scenes with instances.  A context created with SLRHIP_FLAG_DYNAMIC_GEOMETRY | SLRHIP_FLAG_DYNAMIC_INSTANCED keeps the same arrays
 * for a scene with instances (the leaf records of the top level's loose packets and of every mesh share one array), and on top of
 * them the mesh trees' merged level list (4 B per mesh node: level d of EVERY mesh tree is one run, so the refit's launches are
 * bounded by the deepest mesh, not by meshes x depth) and each mesh's root.  The call then runs, in order on `stream`: the vertex
 * store and the record kernels as for a flat scene (a mesh's triangles stay in its local space, exactly as the upload stores them);
 * the refit of ALL mesh trees, deepest merged level first; one launch that gives every mesh its box (the exact union of the valid
 * child boxes of its root) and every instance its world box (the upload's bounds() arithmetic on that box and the instance's CURRENT
 * local_to_world, with that function's own pad and no other); the top-level refit, where an instance child takes its world box and a
 * loose packet the union of its triangles' boxes; and, where slrhip_rebuild_top_level has built its tables, a refresh of the
 * packet boxes it seats with.  The contract is the one above, read as: a fresh context that uploaded the scene with the kept
 * vertex array AND the current placements — frames, slrhip_intersect_rays with instance ids, slrhip_test_visibility, feature,
 * albedo and motion buffers, and the three counters, bit for bit.  Both tree levels keep their shape.  All meshes are refitted on
 * every call, whatever the range.  slrhip_set_instance_transforms afterwards places against the new mesh boxes, and
 * slrhip_rebuild_top_level afterwards seats with the new packet boxes.
 *
 * Not covered: spatial-split trees; adding or removing vertices, triangles or instances; changing indices or materials; a change
 * of SHAPE of either tree level (slrhip_rebuild_top_level re-seats the top level's leaves, nothing rebuilds a mesh tree: the caller
 * uploads again when a tree has degraded); instances that emit; the C++ host mirror and the libSLR adapter.  Motion vectors of moved vertices: slrhip_render_motion
 * takes vertices to stand still; slrhip_render_motion_vertices takes the previous frame's vertex array and covers them.            */
#define SLRHIP_GEOMETRY_BAD_VERTEX 1u      /* a record of a call had a non-finite float; its vertex did not move */
int slrhip_set_vertices(slrhip_ctx* ctx, const slrhip_vertex* device_src, uint32_t first_vertex, uint32_t count, void* stream);
/* The SLRHIP_GEOMETRY_* bits of the calls since the last read, then cleared; waits for `stream`.  0 before any scene.              */
int slrhip_geometry_status(slrhip_ctx* ctx, uint32_t* bits, void* stream);

/* ---- changing materials, spectra and lights without a scene upload ---------------------------------------------------------------
 * The last part of a scene description that a second frame could only change through slrhip_upload_scene: a wall's colour, a lobe's
 * roughness, a lamp's spectrum or intensity, a lamp switched on or off, a checker texture's spectra and mapping, a MULTI record's
 * factors, a material's type.  slrhip_set_materials takes the WHOLE tables again — materials, spectra, spectrum data, textures, in the
 * types and with the meaning of the slrhip_scene_desc fields of the same names, all HOST memory — and replaces the scene's.  The tree,
 * the kept geometry (SLRHIP_FLAG_DYNAMIC_GEOMETRY), slrhip_rebuild_top_level's tables, the environment, the camera, the image
 * textures' texels and everything accumulated since slrhip_render_begin (sensor, statistics, clamp, feature, albedo and motion
 * state) stay; samples rendered after the call see the new tables.
 *
 * The contract, as for slrhip_set_vertices: from the call on the context is indistinguishable, in every bit of every frame, query,
 * feature and albedo buffer and counter, from a context freshly uploaded with the scene description whose four tables are the call's.
 *
 * The light list.  Triangles whose material has an emittance are the scene's lights, in triangle order.  While the set of emitting
 * materials (among those that triangles name) stays as it is, the call does no per-triangle work and runs on every context.  When
 * it changes, the list is rebuilt ON THE DEVICE from the kept index and vertex arrays — a ballot / scan / scatter over the triangles,
 * no atomics, the order taken from the triangle index — which needs a context that keeps its geometry (SLRHIP_FLAG_DYNAMIC_GEOMETRY,
 * and a scene slrhip_set_vertices covers).  The light distribution is uniform (every light's importance is 1), so its tables have a
 * closed form, PMF[i] = 1 / n and CDF[i] = i / n, which is bit for bit the upload's compensated sum for n <= 2^24.
 *
 * Ordering.  The call first waits for the device (albedo, feature and query calls may still read the old tables); it may allocate and
 * it copies from the host, so it can NOT be captured in a graph — like slrhip_set_environment, unlike slrhip_set_vertices.  Its launches
 * run on `stream`.  The library caches no graph across calls, so none outlives the tables.
 *
 * Errors, decided on the host, synchronous, with nothing changed.  SLRHIP_ERR_INVALID_ARGUMENT: a null context or descriptor, non-zero
 * `reserved`, a null material or spectrum table, num_materials or num_textures other than the uploaded scene's (triangles name
 * materials by index, and texture coordinates exist only if the scene had textures), and everything slrhip_upload_scene refuses these
 * tables for, with its code and message.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.  SLRHIP_ERR_UNSUPPORTED: a texture that
 * changes its kind, an IMAGE_SPECTRUM texture that changes width, height or first texel, a material whose alpha-map assignment
 * changes (the leaf records carry it), an emitting material on an instanced triangle, no emitting triangle and no environment, more
 * than 2^24 lights, a change of the emitting set in a context that does not keep its geometry.  A HIP failure after these checks
 * leaves the context without a scene, as a failed upload does.                                                                    */
typedef struct slrhip_materials_desc {
    const slrhip_material* materials;
    uint32_t num_materials;               /* as uploaded */
    const slrhip_spectrum* spectra;
    uint32_t num_spectra;
    const float* spectrum_data;
    uint32_t num_spectrum_data;
    const slrhip_texture* textures;
    uint32_t num_textures;                /* as uploaded */
    uint32_t reserved[2];                 /* 0 */
} slrhip_materials_desc;
int slrhip_set_materials(slrhip_ctx* ctx, const slrhip_materials_desc* desc, void* stream);

/* New texels for ONE IMAGE_SPECTRUM texture of the uploaded scene, in place: the next frame of an animated image.  `texture` is its index
 * in the texture table; width, height and first texel stay as uploaded.  `device_src`: DEVICE memory, 4-byte aligned, [height][width][3]
 * floats in the stored form of the context's mode — (r, g, b) in RGB mode, (u, v, s) in spectral mode.  Nothing is converted: the
 * image textures' spectral form is a reflectance upsampling (not slrhip_env_texels_to_uvs) and stays with the caller, as on upload.
 * SLRHIP_TEXELS_STORE_HALF rounds every float to binary16 first.  One launch, one lane per texel, ordered on `stream`; the call allocates
 * nothing, copies nothing from the host and does not synchronise, so it can be captured in a graph.  Nothing accumulated is reset.
 * SLRHIP_ERR_INVALID_ARGUMENT: a null context or pointer, a misaligned pointer, unknown flag bits, a texture index out of range or of a
 * texture that is no image.  SLRHIP_ERR_NO_SCENE before slrhip_upload_scene.                                                        */
#define SLRHIP_TEXELS_STORE_HALF 1u
int slrhip_set_texture_texels(slrhip_ctx* ctx, uint32_t texture, const float* device_src, uint32_t flags, void* stream);

const char* slrhip_last_error_string(void);
int slrhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SLRHIP_H */
