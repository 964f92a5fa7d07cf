/*
 * slr_oracle.cpp — CPU ORACLE: a scalar restatement of the reference's unidirectional
 * path tracer (goofoo/SLR, libSLR).  TEST INFRASTRUCTURE ONLY: the product never
 * includes, links or calls this file (see oracle/slr_oracle.h).
 *
 * Parity status: PINNED.  oracle/ref_build builds the reference's own sources (in place,
 * unmodified) into oracle/_ref/ and tests/test_oracle_vs_reference.py checks this file
 * against it bit for bit (whole frames with per-(pixel,sample) seeding, single samples,
 * closest-hit batches, RNG known answers, and the reference's own serial render()).
 * The golden vectors under tests/golden/ were produced by that build
 * (tests/golden/make_golden.py) and pin this file where /root/reference is absent.
 *
 * Every function cites the reference file:line it follows (paths relative to
 * /root/reference/libSLR).  Arithmetic is reproduced operation by operation, including
 * the float/double mixing the reference gets from M_PI and unsuffixed literals, and
 * "x / s" implemented as "x * (1.0f / s)" (BasicTypes/Vector3.h:31, RGBTypes.h:67).
 * Build with -ffp-contract=off and without -ffast-math (oracle/Makefile).
 *
 * Deliberate differences (documented in DESIGN.md):
 *   - accelerator: own binary BVH; the reference result does not depend on the tree
 *      except among hits at exactly equal distance, where the reference
 *     keeps the last one tested (TriangleMesh.cpp:158).  Here: larger triangle index wins
 *     (with instances: the larger (instance, triangle) pair, loose triangles = instance -1).
 *   - one xorshift128 stream per (pixel, sample), seeded by slrhip_sample_seed
 *     (the reference has one stream per worker thread, PathTracingRenderer.cpp:33-38).
 */
#include "slr_oracle.h"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

// ------------------------------------------------------------------------------------------
// BasicTypes/Vector3.h:17-147, Point3.h, Normal3.h (float instantiations)
// ------------------------------------------------------------------------------------------
struct V3 {
    float x, y, z;
    V3() : x(0), y(0), z(0) {}
    V3(float xx, float yy, float zz) : x(xx), y(yy), z(zz) {}
    float operator[](int i) const { return (&x)[i]; }
    float& operator[](int i) { return (&x)[i]; }
};
inline V3 operator+(V3 a, V3 b) { return V3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline V3 operator-(V3 a, V3 b) { return V3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline V3 operator-(V3 a) { return V3(-a.x, -a.y, -a.z); }
inline V3 operator*(V3 a, float s) { return V3(a.x * s, a.y * s, a.z * s); }
inline V3 operator*(float s, V3 a) { return V3(s * a.x, s * a.y, s * a.z); }
// Vector3.h:31: operator/(s) is a reciprocal multiply
inline V3 operator/(V3 a, float s) { float r = 1.0f / s; return V3(a.x * r, a.y * r, a.z * r); }
inline float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }            // Vector3.h:108-110
inline float absDot(V3 a, V3 b) { return std::fabs(a.x * b.x + a.y * b.y + a.z * b.z); } // Vector3.h:120-122
inline V3 cross(V3 a, V3 b) {                                                          // Vector3.h:113-117
    return V3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
inline float length(V3 a) { return std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }     // Vector3.h:55
inline float sqLength(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
inline V3 normalize(V3 a) { float l = length(a); return a / l; }                       // Vector3.h:102-105

// Core/geometry.h:225-235
struct Frame {
    V3 x, y, z;
    V3 toLocal(V3 v) const { return V3(dot(x, v), dot(y, v), dot(z, v)); }
    V3 fromLocal(V3 v) const {
        return V3(dot(V3(x.x, y.x, z.x), v), dot(V3(x.y, y.y, z.y), v), dot(V3(x.z, y.z, z.z), v));
    }
};

// ------------------------------------------------------------------------------------------
// Spectrum value types.  N = 3: RGBTemplate<float> (BasicTypes/RGBTypes.h:51-143).
// ------------------------------------------------------------------------------------------
template <int N>
struct Spec {
    float c[N];
    Spec() { for (int i = 0; i < N; ++i) c[i] = 0.0f; }
    explicit Spec(float v) { for (int i = 0; i < N; ++i) c[i] = v; }
    float operator[](int i) const { return c[i]; }
    float& operator[](int i) { return c[i]; }
    bool isZero() const { for (int i = 0; i < N; ++i) if (c[i] != 0.0f) return false; return true; }
};
template <int N> inline Spec<N> operator+(Spec<N> a, Spec<N> b) { Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = a.c[i] + b.c[i]; return r; }
template <int N> inline Spec<N> operator-(Spec<N> a, Spec<N> b) { Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = a.c[i] - b.c[i]; return r; }
template <int N> inline Spec<N> operator*(Spec<N> a, Spec<N> b) { Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = a.c[i] * b.c[i]; return r; }
template <int N> inline Spec<N> operator/(Spec<N> a, Spec<N> b) { Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = a.c[i] / b.c[i]; return r; }
template <int N> inline Spec<N> operator*(Spec<N> a, float s) { Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = a.c[i] * s; return r; }
template <int N> inline Spec<N> operator*(float s, Spec<N> a) { Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = s * a.c[i]; return r; }
// RGBTypes.h:67 / SpectrumTypes.h:393-399: reciprocal multiply
template <int N> inline Spec<N> operator/(Spec<N> a, float s) { float rc = 1.0f / s; Spec<N> r; for (int i = 0; i < N; ++i) r.c[i] = a.c[i] * rc; return r; }
template <int N> inline Spec<N> operator+(Spec<N> a, float s) { return a + Spec<N>(s); } // implicit ctor from scalar
template <int N> inline Spec<N> operator-(Spec<N> a, float s) { return a - Spec<N>(s); }

// importance(): 0.9-primary weighting.  RGBTypes.h:103-108 (sum = r + g + b, marginal = (1 - primary) / 2) and
// SpectrumTypes.h:512-526 (running sum from 0, marginal = (1 - primary) / (N - 1)) are the same float
// operations for N = 3, so one template serves both.
template <int N>
inline float importance(const Spec<N>& s, uint16_t selectedLambda) {
    float sum = 0;
    for (int i = 0; i < N; ++i) sum += s.c[i];
    const float primary = 0.9f;
    const float marginal = (1 - primary) / (N - 1);
    return sum * marginal + s.c[selectedLambda] * (primary - marginal);
}

// luminance(): RGBTypes.h:94-100 (double coefficients, float result) / SpectrumTypes.h:504-509 (mean of the samples)
template <int N>
inline float luminance(const Spec<N>& s) {
    if (N == 3) return (float)(0.222485 * s.c[0] + 0.716905 * s.c[1] + 0.060610 * s.c[2]);
    float sum = 0;
    for (int i = 0; i < N; ++i) sum += s.c[i];
    return sum / N;
}

// WavelengthSamples: RGBSamplesTemplate (RGBTypes.h:19-48) / WavelengthSamplesTemplate (SpectrumTypes.h:17-65)
template <int N>
struct Wls {
    float lambdas[N];
    uint16_t selectedLambda;
    uint16_t flags;              // bit 0 = LambdaIsSelected
};
static const float kWavelengthLowBound = 360.0f, kWavelengthHighBound = 830.0f;   // BasicTypes/Spectrum.h:115-116

// BasicTypes/CompensatedSum.h:15-32
template <typename T>
struct Kahan {
    T result, comp;
    Kahan() : result(), comp() {}
    void add(const T& value) {
        T cInput = value - comp;
        T sumTemp = result + cInput;
        comp = (sumTemp - result) - cInput;
        result = sumTemp;
    }
};

// ------------------------------------------------------------------------------------------
// RNGs/XORShiftRNG.cpp:21-36, Core/RandomNumberGenerator.cpp:12-15
// ------------------------------------------------------------------------------------------
struct XorShift {
    uint32_t s[4];
    uint64_t* drawCounter;
    explicit XorShift(int32_t seed, uint64_t* counter = nullptr) : drawCounter(counter) {
        for (int i = 0; i < 4; ++i) {
            // `seed` is SIGNED: the shift is arithmetic; the product is computed in unsigned.
            uint32_t v = 1812433253U * ((uint32_t)seed ^ (uint32_t)(seed >> 30)) + (uint32_t)i;
            s[i] = v;
            seed = (int32_t)v;
        }
        for (int i = 0; i < 50; ++i) getUInt();
    }
    uint32_t getUInt() {
        uint32_t t = s[0] ^ (s[0] << 11);
        s[0] = s[1]; s[1] = s[2]; s[2] = s[3];
        return s[3] = (s[3] ^ (s[3] >> 19)) ^ (t ^ (t >> 8));
    }
    float getFloat0cTo1o() {
        if (drawCounter) ++*drawCounter;
        uint32_t fractionBits = (getUInt() >> 9) | 0x3f800000;
        float f;
        std::memcpy(&f, &fractionBits, 4);
        return f - 1.0f;
    }
};

// ------------------------------------------------------------------------------------------
// Core/distributions.cpp:37-70 (float instantiation).  `theta *= M_PI_4` is a double
// multiply rounded to float; `cos(theta)` is the double ::cos (unqualified call in namespace
// SLR resolves to the C function), `r * cos(theta)` is a double product rounded to float.
// ------------------------------------------------------------------------------------------
inline void concentricSampleDisk(float u0, float u1, float* dx, float* dy) {
    float r, theta;
    float sx = 2 * u0 - 1;
    float sy = 2 * u1 - 1;
    if (sx == 0 && sy == 0) { *dx = 0; *dy = 0; return; }
    if (sx >= -sy) {
        if (sx > sy) { r = sx; theta = sy / sx; }
        else { r = sy; theta = 2 - sx / sy; }
    }
    else {
        if (sx > sy) { r = -sy; theta = 6 + sx / sy; }
        else { r = -sx; theta = 4 + sy / sx; }
    }
    theta = (float)((double)theta * M_PI_4);
    *dx = (float)((double)r * ::cos((double)theta));
    *dy = (float)((double)r * ::sin((double)theta));
}
// Core/distributions.h:26-33
inline V3 cosineSampleHemisphere(float u0, float u1) {
    float x, y;
    concentricSampleDisk(u0, u1, &x, &y);
    return V3(x, y, std::sqrt(std::fmax(0.0f, 1.0f - x * x - y * y)));
}
// Core/distributions.h:59-64
inline void uniformSampleTriangle(float u0, float u1, float* b0, float* b1) {
    float su1 = std::sqrt(u0);
    *b0 = 1.0f - su1;
    *b1 = u1 * su1;
}

inline uint32_t prevPowerOf2(uint32_t x) {   // defines.h:136-143
    x |= x >> 1; x |= x >> 2; x |= x >> 4; x |= x >> 8; x |= x >> 16;
    return x - (x >> 1);
}

// Core/distributions.cpp:76-119  RegularConstantDiscrete1D
struct Discrete1D {
    std::vector<float> PMF, CDF;
    float integral = 0.0f;
    void build(const std::vector<float>& values) {
        size_t n = values.size();
        PMF = values;
        CDF.assign(n + 1, 0.0f);
        Kahan<float> sum;
        for (size_t i = 0; i < n; ++i) { sum.add(PMF[i]); CDF[i + 1] = sum.result; }
        integral = sum.result;
        for (size_t i = 0; i < n; ++i) { PMF[i] /= integral; CDF[i + 1] /= integral; }
    }
    uint32_t sample(float u, float* prob) const {
        uint32_t n = (uint32_t)PMF.size();
        int idx = (int)n;
        for (int d = (int)prevPowerOf2(n); d > 0; d >>= 1)
            if (idx - d > 0 && CDF[idx - d] >= u) idx -= d;
        --idx;
        *prob = PMF[idx];
        return (uint32_t)idx;
    }
};

// Core/distributions.cpp:127-184  RegularConstantContinuous1D (constructed from a pick function)
struct Continuous1D {
    std::vector<float> PDF, CDF;
    float integral = 0.0f;
    uint32_t numValues = 0;
    void build(const std::vector<float>& values) {
        numValues = (uint32_t)values.size();
        PDF = values;
        CDF.assign(numValues + 1, 0.0f);
        Kahan<float> sum;
        for (uint32_t i = 0; i < numValues; ++i) { sum.add(PDF[i] / numValues); CDF[i + 1] = sum.result; }
        integral = sum.result;
        for (uint32_t i = 0; i < numValues; ++i) { PDF[i] /= sum.result; CDF[i + 1] /= sum.result; }
    }
    float sample(float u, float* pdf) const {
        int idx = (int)numValues;
        for (int d = (int)prevPowerOf2(numValues); d > 0; d >>= 1)
            if (idx - d > 0 && CDF[idx - d] >= u) idx -= d;
        --idx;
        *pdf = PDF[idx];
        float t = (u - CDF[idx]) / (CDF[idx + 1] - CDF[idx]);
        return (idx + t) / numValues;
    }
    // :181-184 index with no clamp and assert smp < 1.  theta / pi and phi / 2pi DO round up to 1.0f — a direction out of a
    // bump-mapped frame (three unit vectors, not orthogonal: SurfaceObject.cpp:123-134) is not a unit vector, its y below -1 is
    // clamped and acos gives (float)pi — and the reference then reads one float past its table: no answer to restate.  The
    // last cell, as the device does (envAreaPDF, pt_env_sphere.h).
    float evaluatePDF(float smp) const { return PDF[std::min((uint32_t)(int32_t)(smp * numValues), numValues - 1)]; }
};
// Core/distributions.cpp:186-224  RegularConstantContinuous2D
struct Continuous2D {
    std::vector<Continuous1D> rows;
    Continuous1D top;
    void build(uint32_t numD1, uint32_t numD2, const std::vector<float>& values /* [numD2][numD1] */) {
        rows.resize(numD2);
        std::vector<float> integrals(numD2);
        for (uint32_t i = 0; i < numD2; ++i) {
            rows[i].build(std::vector<float>(values.begin() + (size_t)i * numD1, values.begin() + (size_t)(i + 1) * numD1));
            integrals[i] = rows[i].integral;
        }
        top.build(integrals);
    }
    void sample(float u0, float u1, float* d0, float* d1, float* pdf) const {
        float topPDF;
        *d1 = top.sample(u1, &topPDF);
        uint32_t num = (uint32_t)rows.size();
        uint32_t idx1D = std::min(uint32_t(num * *d1), num - 1);
        *d0 = rows[idx1D].sample(u0, pdf);
        *pdf *= topPDF;
    }
    float evaluatePDF(float d0, float d1) const {
        uint32_t num = (uint32_t)rows.size();
        uint32_t idx1D = std::min(uint32_t(num * d1), num - 1);
        return top.evaluatePDF(d1) * rows[idx1D].evaluatePDF(d0);
    }
};

// ------------------------------------------------------------------------------------------
// Scene data
// ------------------------------------------------------------------------------------------
struct Tri {
    uint32_t v[3];
    uint32_t material;
    int32_t lightIndex;   // index in the aggregate's light list, -1 if not emitting
};

struct Ray {
    V3 org, dir;
    float distMin, distMax;
};

struct Isect {             // Core/geometry.h:206-221 (fields the path uses)
    float dist;
    V3 p;
    V3 gNormal;
    float u, v;
    float texU, texV;      // Intersection::texCoord (TriangleMesh.cpp:160-161,174)
    uint32_t tri;
    int32_t inst;          // TransformedSurfaceObject the hit went through (index into the scene's instances), -1 = none
    bool atInfinity;
    Isect() : dist(INFINITY), u(0), v(0), texU(0), texV(0), tri(0xFFFFFFFFu), inst(-1), atInfinity(false) {}
};

struct SurfPt {            // Core/geometry.h:239-258
    V3 p;
    bool atInfinity;
    V3 gNormal;
    float u, v;
    Frame frame;
    uint32_t tri;          // obj; kEnvObject = the environment sphere
    float texU, texV;      // texCoord: the environment texture and the checkerboard textures read it
};
static const uint32_t kEnvObject = 0xFFFFFFFEu;

struct BVHNode {
    float bmin[3], bmax[3];
    uint32_t left;         // inner: left child (right = left + 1); leaf: first triangle slot
    uint32_t count;        // 0 = inner
};

struct Camera {            // Cameras/PerspectiveCamera.h:17-29 + its StaticTransform
    float mat[16], matInv[16];    // column-major
    float aspect, fovY, lensRadius, imgPlaneDistance, objPlaneDistance;
    float opWidth, opHeight, imgPlaneArea;
    float sensitivity;
};

} // namespace

struct slr_oracle_scene {
    int mode;
    std::vector<slrhip_vertex> vertices;
    std::vector<Tri> tris;
    std::vector<slrhip_material> materials;
    std::vector<slrhip_spectrum> spectra;
    std::vector<float> spectrumData;
    std::vector<slrhip_texture> textures;
    std::vector<float> textureTexels;          // texels of the IMAGE_SPECTRUM textures, 3 floats each
    Camera camera;
    std::vector<uint32_t> lightTris;   // SurfaceObjectAggregate::m_lightList (SurfaceObject.cpp:232-249)
    Discrete1D lightDist;              // m_lightDist1D
    std::vector<BVHNode> nodes;        // top level: the loose triangles and the instances (primitive id >= tris.size())
    std::vector<uint32_t> triOrder;
    // instancing (TransformedSurfaceObject, SurfaceObject.cpp:303-392): per instance its mesh; per mesh its own tree
    std::vector<slrhip_instance> instances;
    struct Mesh { uint32_t first, count; std::vector<BVHNode> nodes; std::vector<uint32_t> order; float bmin[3], bmax[3]; };
    std::vector<Mesh> meshes;
    std::vector<uint32_t> meshOfInstance;
    bool hasEnv;
    // InfiniteSphereSurfaceObject (SurfaceObject.cpp:137-141): texture, scale, importance distribution
    uint32_t envWidth = 0, envHeight = 0;
    std::vector<float> envTexels;
    // Meng-15 upsampling tables for spectra whose (u, v) is only known at run time (environment texels in spectral mode)
    uint32_t gridWidth = 0, gridHeight = 0;
    std::vector<uint8_t> gridCells;          // 8 bytes per cell: inside, num_points, idx[6]
    std::vector<float> pointUV, pointSpectrum;
    float envScale = 1.0f;
    Continuous2D envDist;
};

namespace {

typedef slr_oracle_scene Scene;

inline V3 vpos(const Scene& s, uint32_t vi) { const float* p = s.vertices[vi].position; return V3(p[0], p[1], p[2]); }
inline V3 vnrm(const Scene& s, uint32_t vi) { const float* p = s.vertices[vi].normal; return V3(p[0], p[1], p[2]); }
inline V3 vtan(const Scene& s, uint32_t vi) { const float* p = s.vertices[vi].tangent; return V3(p[0], p[1], p[2]); }

// Matrix4x4 x Point3D / Vector3D (Matrix4x4.h:71-81) and StaticTransform x Normal3D (Transform.h:47-52); column-major m
inline V3 mulPoint(const float* m, V3 p) {
    float x = m[0] * p.x + m[4] * p.y + m[8] * p.z + m[12] * 1.0f;
    float y = m[1] * p.x + m[5] * p.y + m[9] * p.z + m[13] * 1.0f;
    float z = m[2] * p.x + m[6] * p.y + m[10] * p.z + m[14] * 1.0f;
    float w = m[3] * p.x + m[7] * p.y + m[11] * p.z + m[15] * 1.0f;
    if (w != 1.0f) { float r = 1.0f / w; x *= r; y *= r; z *= r; }
    return V3(x, y, z);
}
inline V3 mulVector(const float* m, V3 v) {   // Matrix4x4.h:71-73
    return V3(m[0] * v.x + m[4] * v.y + m[8] * v.z, m[1] * v.x + m[5] * v.y + m[9] * v.z, m[2] * v.x + m[6] * v.y + m[10] * v.z);
}
inline V3 mulNormal(const float* mi, V3 n) {  // Transform.h:47-52 (rows of the inverse)
    return V3(mi[0] * n.x + mi[1] * n.y + mi[2] * n.z, mi[4] * n.x + mi[5] * n.y + mi[6] * n.z, mi[8] * n.x + mi[9] * n.y + mi[10] * n.z);
}

// ------------------------------------------------------------------------------------------
// Accelerator (oracle's own): binary BVH, median split on the widest centroid axis.
// ------------------------------------------------------------------------------------------
// `order` starts as the list of primitive ids; bmin / bmax / cen are indexed by primitive id
void buildBVHOver(std::vector<BVHNode>& nodes, std::vector<uint32_t>& order, const std::vector<float>& bmin, const std::vector<float>& bmax,
                  const std::vector<float>& cen) {
    const uint32_t n = (uint32_t)order.size();
    nodes.clear();
    nodes.reserve(2 * (size_t)n + 1);
    struct Job { uint32_t node, begin, end; };
    std::vector<Job> stack;
    nodes.push_back(BVHNode());
    stack.push_back({0, 0, n});
    while (!stack.empty()) {
        Job j = stack.back(); stack.pop_back();
        BVHNode nd;
        float cmin[3] = {INFINITY, INFINITY, INFINITY}, cmax[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int a = 0; a < 3; ++a) { nd.bmin[a] = INFINITY; nd.bmax[a] = -INFINITY; }
        for (uint32_t k = j.begin; k < j.end; ++k) {
            uint32_t t = order[k];
            for (int a = 0; a < 3; ++a) {
                nd.bmin[a] = std::fmin(nd.bmin[a], bmin[3 * (size_t)t + a]);
                nd.bmax[a] = std::fmax(nd.bmax[a], bmax[3 * (size_t)t + a]);
                cmin[a] = std::fmin(cmin[a], cen[3 * (size_t)t + a]);
                cmax[a] = std::fmax(cmax[a], cen[3 * (size_t)t + a]);
            }
        }
        uint32_t cnt = j.end - j.begin;
        int axis = 0;
        float ext = cmax[0] - cmin[0];
        for (int a = 1; a < 3; ++a) if (cmax[a] - cmin[a] > ext) { ext = cmax[a] - cmin[a]; axis = a; }
        if (cnt <= 4 || !(ext > 0.0f)) {
            nd.left = j.begin; nd.count = cnt;
            nodes[j.node] = nd;
            continue;
        }
        uint32_t mid = j.begin + cnt / 2;
        std::nth_element(order.begin() + j.begin, order.begin() + mid, order.begin() + j.end,
                         [&](uint32_t a, uint32_t b) {
                             float ca = cen[3 * (size_t)a + axis], cb = cen[3 * (size_t)b + axis];
                             return ca < cb || (ca == cb && a < b);
                         });
        nd.left = (uint32_t)nodes.size(); nd.count = 0;
        nodes[j.node] = nd;
        nodes.push_back(BVHNode()); nodes.push_back(BVHNode());
        stack.push_back({nd.left, j.begin, mid});
        stack.push_back({nd.left + 1, mid, j.end});
    }
}

void buildBVH(Scene& s) {
    const uint32_t n = (uint32_t)s.tris.size(), ni = (uint32_t)s.instances.size();
    std::vector<float> cen(3 * (size_t)(n + ni)), bmin(3 * (size_t)(n + ni)), bmax(3 * (size_t)(n + ni));
    std::vector<char> instanced(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        for (int a = 0; a < 3; ++a) {
            float p0 = vpos(s, s.tris[i].v[0])[a], p1 = vpos(s, s.tris[i].v[1])[a], p2 = vpos(s, s.tris[i].v[2])[a];
            float lo = std::fmin(p0, std::fmin(p1, p2)), hi = std::fmax(p0, std::fmax(p1, p2));
            bmin[3 * (size_t)i + a] = lo; bmax[3 * (size_t)i + a] = hi; cen[3 * (size_t)i + a] = 0.5f * (lo + hi);
        }
    }
    // one tree per distinct mesh (triangle range), in the mesh's local space
    s.meshes.clear();
    s.meshOfInstance.assign(ni, 0);
    for (uint32_t k = 0; k < ni; ++k) {
        const slrhip_instance& in = s.instances[k];
        uint32_t m = 0;
        for (; m < s.meshes.size(); ++m) if (s.meshes[m].first == in.first_triangle && s.meshes[m].count == in.num_triangles) break;
        if (m == s.meshes.size()) {
            Scene::Mesh mesh;
            mesh.first = in.first_triangle; mesh.count = in.num_triangles;
            mesh.order.resize(mesh.count);
            for (int a = 0; a < 3; ++a) { mesh.bmin[a] = INFINITY; mesh.bmax[a] = -INFINITY; }
            for (uint32_t t = 0; t < mesh.count; ++t) {
                mesh.order[t] = mesh.first + t;
                instanced[mesh.first + t] = 1;
                for (int a = 0; a < 3; ++a) {
                    mesh.bmin[a] = std::fmin(mesh.bmin[a], bmin[3 * (size_t)(mesh.first + t) + a]);
                    mesh.bmax[a] = std::fmax(mesh.bmax[a], bmax[3 * (size_t)(mesh.first + t) + a]);
                }
            }
            buildBVHOver(mesh.nodes, mesh.order, bmin, bmax, cen);
            s.meshes.push_back(std::move(mesh));
        }
        s.meshOfInstance[k] = m;
        // the instance's world box: the eight corners of the mesh box through the transform (StaticTransform x BoundingBox3D, Transform.h:54-65)
        const Scene::Mesh& mesh = s.meshes[m];
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int c = 0; c < 8; ++c) {
            V3 p = mulPoint(in.local_to_world, V3((c & 4) ? mesh.bmax[0] : mesh.bmin[0], (c & 2) ? mesh.bmax[1] : mesh.bmin[1], (c & 1) ? mesh.bmax[2] : mesh.bmin[2]));
            for (int a = 0; a < 3; ++a) { lo[a] = std::fmin(lo[a], p[a]); hi[a] = std::fmax(hi[a], p[a]); }
        }
        for (int a = 0; a < 3; ++a) {
            // a hair of slack: the local-space traversal rounds differently from a world-space box test
            const float pad = 1e-5f * std::fmax(1.0f, std::fmax(std::fabs(lo[a]), std::fabs(hi[a])));
            bmin[3 * (size_t)(n + k) + a] = lo[a] - pad; bmax[3 * (size_t)(n + k) + a] = hi[a] + pad; cen[3 * (size_t)(n + k) + a] = 0.5f * (lo[a] + hi[a]);
        }
    }
    // top level: loose triangles + instances
    s.triOrder.clear();
    for (uint32_t i = 0; i < n; ++i) if (!instanced[i]) s.triOrder.push_back(i);
    for (uint32_t k = 0; k < ni; ++k) s.triOrder.push_back(n + k);
    buildBVHOver(s.nodes, s.triOrder, bmin, bmax, cen);
}

// Core/geometry.h:112-126 BoundingBox3D::intersect (slab test)
inline bool boxHit(const BVHNode& nd, const Ray& r, V3 invDir) {
    float dist0 = r.distMin, dist1 = r.distMax;
    for (int i = 0; i < 3; ++i) {
        float tNear = (nd.bmin[i] - r.org[i]) * invDir[i];
        float tFar = (nd.bmax[i] - r.org[i]) * invDir[i];
        if (tNear > tFar) std::swap(tNear, tFar);
        dist0 = tNear > dist0 ? tNear : dist0;
        dist1 = tFar < dist1 ? tFar : dist1;
        if (dist0 > dist1) return false;
    }
    return true;
}

// Surface/TriangleMesh.cpp:131-178  Triangle::intersect (Moller-Trumbore, no culling).
// Returns true and fills *isect when the hit is accepted under the closest-hit rule;
// ties at equal distance: larger triangle index wins (see file header).
// ---- procedural textures: Textures/checker_board_textures.{h,cpp} through a Texture2DMapping (Core/textures.h:16-42) ---------
inline void textureMap(const slrhip_texture& t, float u, float v, float* x, float* y) {
    *x = (u + t.offset[0]) * t.scale[0];           // OffsetAndScale2DMapping::map :37-41 (offset 0, scale 1 = Texture2DMapping::map)
    *y = (v + t.offset[1]) * t.scale[1];
}
inline int checkerIndex(const slrhip_texture& t, float u, float v) {
    float x, y;
    textureMap(t, u, v, &x, &y);
    int idx = ((int)(x * 2) + (int)(y * 2)) % 2;   // checker_board_textures.h:23,49
    return idx < 0 ? -idx : idx;                   // (the reference indexes its two-element array with -1 there: undefined)
}
// CheckerBoardNormal3DTexture::evaluate, checker_board_textures.cpp:16-43
inline V3 checkerNormal(const slrhip_texture& t, float u, float v) {
    float x, y;
    textureMap(t, u, v, &x, &y);
    const float stepWidth = t.value[0];
    const bool reverse = t.value[1] != 0.0f;
    float halfWidth = stepWidth * 0.5f;
    float uComp = 0.0f;
    float absWrapU = std::fmod(std::fabs(x), 1.0f);
    if (absWrapU < halfWidth * 0.5f || absWrapU > 1.0f - halfWidth * 0.5f) uComp = 1.0f;
    else if (absWrapU > 0.5f - halfWidth * 0.5f && absWrapU < 0.5f + halfWidth * 0.5f) uComp = -1.0f;
    float vComp = 0.0f;
    float absWrapV = std::fmod(std::fabs(y), 1.0f);
    if (absWrapV < halfWidth * 0.5f || absWrapV > 1.0f - halfWidth * 0.5f) vComp = 1.0f;
    else if (absWrapV > 0.5f - halfWidth * 0.5f && absWrapV < 0.5f + halfWidth * 0.5f) vComp = -1.0f;
    if (absWrapV > 0.5f) uComp *= -1;
    if (absWrapU > 0.5f) vComp *= -1;
    if (reverse) { uComp *= -1; vComp *= -1; }
    return normalize(V3(uComp, vComp, 1.0f));
}
inline const slrhip_texture* normalMapOf(const Scene& s, const slrhip_material& m) {
    const uint32_t t = m.reserved & 0xFFFFu;
    return t ? &s.textures[t - 1] : nullptr;
}
inline const slrhip_texture* alphaMapOf(const Scene& s, const slrhip_material& m) {
    const uint32_t t = m.reserved >> 16;
    return t ? &s.textures[t - 1] : nullptr;
}

inline bool triIntersect(const Scene& s, uint32_t ti, const Ray& ray, Isect* isect, int32_t inst = -1) {
    const Tri& tri = s.tris[ti];
    V3 p0 = vpos(s, tri.v[0]), p1 = vpos(s, tri.v[1]), p2 = vpos(s, tri.v[2]);
    V3 edge01 = p1 - p0;
    V3 edge02 = p2 - p0;
    V3 p = cross(ray.dir, edge02);
    float det = dot(edge01, p);
    if (det == 0.0f) return false;
    float invDet = 1.0f / det;
    V3 d = ray.org - p0;
    float b1 = dot(d, p) * invDet;
    if (b1 < 0.0f || b1 > 1.0f) return false;
    V3 q = cross(d, edge01);
    float b2 = dot(ray.dir, q) * invDet;
    if (b2 < 0.0f || b1 + b2 > 1.0f) return false;
    float tt = dot(edge02, q) * invDet;
    if (tt < ray.distMin || tt > ray.distMax) return false;
    // tie rule (file header): at equal distance the later object wins — larger (instance, triangle) pair
    if (tt == ray.distMax && isect->tri != 0xFFFFFFFFu && (inst < isect->inst || (inst == isect->inst && ti < isect->tri))) return false;
    float b0 = 1.0f - b1 - b2;
    // TexCoord2D texCoord = b0 * v0.texCoord + b1 * v1.texCoord + b2 * v2.texCoord  (:160-161), from the ORIGINAL barycentrics
    const float* tc0 = s.vertices[tri.v[0]].texcoord;
    const float* tc1 = s.vertices[tri.v[1]].texcoord;
    const float* tc2 = s.vertices[tri.v[2]].texcoord;
    const float texU = (b0 * tc0[0] + b1 * tc1[0]) + b2 * tc2[0];
    const float texV = (b0 * tc0[1] + b1 * tc1[1]) + b2 * tc2[1];
    // "If zero, intersection doesn't occur" (:162-167)
    if (const slrhip_texture* alpha = alphaMapOf(s, s.materials[tri.material]))
        if (alpha->value[checkerIndex(*alpha, texU, texV)] == 0.0f) return false;
    isect->texU = texU;
    isect->texV = texV;
    isect->dist = tt;
    isect->p = ray.org + ray.dir * tt;
    isect->gNormal = normalize(cross(edge01, edge02));
    isect->u = b0;
    isect->v = b1;
    isect->tri = ti;
    isect->inst = inst;
    isect->atInfinity = false;
    return true;
}

// SurfaceObjectAggregate::intersect -> Accelerator::intersect (Core/SurfaceObject.cpp:267-269).
// On every accepted hit ray.distMax = isect->dist (SBVH.h:417-442 / QBVH.h:334-336).
// TransformedSurfaceObject::intersect (SurfaceObject.cpp:307-317): localRay = invert(TF) * ray — origin as a point, direction as a
// vector, distMin / distMax unchanged (Transform.h:53) — the mesh's aggregate intersects it, ray.distMax = localRay.distMax.
bool instanceIntersect(const Scene& s, uint32_t k, Ray& ray, Isect* isect, slr_oracle_counters* ctr) {
    const slrhip_instance& in = s.instances[k];
    const Scene::Mesh& mesh = s.meshes[s.meshOfInstance[k]];
    Ray local;
    local.org = mulPoint(in.world_to_local, ray.org);
    local.dir = mulVector(in.world_to_local, ray.dir);
    local.distMin = ray.distMin; local.distMax = ray.distMax;
    V3 invDir(1.0f / local.dir.x, 1.0f / local.dir.y, 1.0f / local.dir.z);
    uint32_t stack[128];
    int sp = 0;
    stack[sp++] = 0;
    bool any = false;
    while (sp > 0) {
        const BVHNode& nd = mesh.nodes[stack[--sp]];
        if (ctr) ++ctr->nodes_visited;
        if (!boxHit(nd, local, invDir)) continue;
        if (nd.count) {
            for (uint32_t t = 0; t < nd.count; ++t) {
                if (ctr) ++ctr->tris_tested;
                if (triIntersect(s, mesh.order[nd.left + t], local, isect, (int32_t)k)) { local.distMax = isect->dist; any = true; }
            }
        }
        else {
            stack[sp++] = nd.left;
            stack[sp++] = nd.left + 1;
        }
    }
    if (any) ray.distMax = local.distMax;
    return any;
}

bool aggregateIntersect(const Scene& s, Ray& ray, Isect* isect, slr_oracle_counters* ctr) {
    V3 invDir(1.0f / ray.dir.x, 1.0f / ray.dir.y, 1.0f / ray.dir.z);   // Vector3.h:60 reciprocal()
    const uint32_t numTris = (uint32_t)s.tris.size();
    uint32_t stack[128];
    int sp = 0;
    stack[sp++] = 0;
    bool any = false;
    while (sp > 0) {
        const BVHNode& nd = s.nodes[stack[--sp]];
        if (ctr) ++ctr->nodes_visited;
        if (!boxHit(nd, ray, invDir)) continue;
        if (nd.count) {
            for (uint32_t k = 0; k < nd.count; ++k) {
                const uint32_t prim = s.triOrder[nd.left + k];
                if (prim >= numTris) { if (instanceIntersect(s, prim - numTris, ray, isect, ctr)) any = true; continue; }
                if (ctr) ++ctr->tris_tested;
                if (triIntersect(s, prim, ray, isect)) { ray.distMax = isect->dist; any = true; }
            }
        }
        else {
            stack[sp++] = nd.left;
            stack[sp++] = nd.left + 1;
        }
    }
    return any;
}

// Core/SurfaceObject.cpp:408-416  Scene::intersect; Surface/InfiniteSphere.cpp:34-46  InfiniteSphere::intersect
bool sceneIntersect(const Scene& s, Ray& ray, Isect* isect, slr_oracle_counters* ctr) {
    if (ctr) ++ctr->extension_rays;
    if (aggregateIntersect(s, ray, isect, ctr)) return true;
    if (s.hasEnv) {
        if (!std::isinf(ray.distMax)) return false;
        // Vector3::toPolarYUp, BasicTypes/Vector3.h:72-75
        float theta = std::acos(std::min(1.0f, std::max(-1.0f, ray.dir.y)));
        float phi = std::fmod((float)(std::atan2(-ray.dir.x, ray.dir.z) + 2 * M_PI), (float)(2 * M_PI));
        isect->dist = INFINITY;
        isect->p = ray.dir;
        isect->gNormal = -ray.dir;
        isect->u = phi;
        isect->v = theta;
        isect->tri = kEnvObject;
        isect->atInfinity = true;
        return true;
    }
    return false;
}

// ImageSpectrumTexture::evaluate (Textures/image_textures.cpp:13-20,57-63): nearest texel, wrap by fmod
Spec<3> envTexture(const Scene& s, float tcU, float tcV) {
    float u = std::fmod(tcU, 1.0f);
    float v = std::fmod(tcV, 1.0f);
    u += u < 0 ? 1.0f : 0.0f;
    v += v < 0 ? 1.0f : 0.0f;
    uint32_t px = std::min((uint32_t)(s.envWidth * u), s.envWidth - 1);
    uint32_t py = std::min((uint32_t)(s.envHeight * v), s.envHeight - 1);
    const float* t = &s.envTexels[((size_t)py * s.envWidth + px) * 3];
    Spec<3> r; r.c[0] = t[0]; r.c[1] = t[1]; r.c[2] = t[2];
    return r;
}
// IBLEmission::emittance, SurfaceMaterials/IBLEmission.cpp:15-17: M_PI * tex * scale
Spec<3> envEmittance(const Scene& s, float tcU, float tcV) { return ((float)M_PI * envTexture(s, tcU, tcV)) * s.envScale; }
// UpsampledContinuousSpectrumTemplate::evaluate with the grid look-up done here (SpectrumTypes.h:239-339): the run-time twin of
// what slr_amd/spectra.py:resolve_upsampled does ahead of time for constant spectra.
inline Spec<16> evaluateUpsampled(const Scene& sc, float u, float v, float scale, const Wls<16>& wls) {
    const uint32_t GridWidth = sc.gridWidth, GridHeight = sc.gridHeight, NumWavelengthSamples = 95;
    if (u < 0.0f || u >= GridWidth || v < 0.0f || v >= GridHeight) return Spec<16>(0.0f);
    const int32_t ui = (int32_t)u, vi = (int32_t)v;
    const uint8_t* cell = &sc.gridCells[(size_t)(ui + (int32_t)GridWidth * vi) * 8];
    const uint8_t* indices = cell + 2;
    const uint8_t numPoints = cell[1];
    uint8_t usedIndices[4] = {255, 255, 255, 255};
    float weights[4] = {0, 0, 0, 0};
    const float* uv = sc.pointUV.data();
    if (cell[0]) {
        float s = u - ui, t = v - vi;
        weights[0] = (1 - s) * (1 - t);
        weights[1] = s * (1 - t);
        weights[2] = (1 - s) * t;
        weights[3] = s * t;
        for (int k = 0; k < 4; ++k) usedIndices[k] = indices[k];
    }
    else {
        const float ex = u - uv[2 * indices[0]], ey = v - uv[2 * indices[0] + 1];
        float e0x = uv[2 * indices[1]] - uv[2 * indices[0]], e0y = uv[2 * indices[1] + 1] - uv[2 * indices[0] + 1];
        float uu = e0x * ey - ex * e0y;
        for (int i = 1; i < numPoints; ++i) {
            uint32_t idx = indices[i % (numPoints - 1) + 1];
            float e1x = uv[2 * idx] - uv[2 * indices[0]], e1y = uv[2 * idx + 1] - uv[2 * indices[0] + 1];
            float vv = ex * e1y - e1x * ey;
            const float area = e0x * e1y - e1x * e0y;
            const float bu = uu / area, bv = vv / area;
            float bw = 1.0f - bu - bv;
            if (bu < -1e-6 || bv < -1e-6 || bw < -1e-6) {
                uu = -vv;
                e0x = e1x;
                e0y = e1y;
                continue;
            }
            weights[0] = bu; weights[1] = bv; weights[2] = bw;
            usedIndices[0] = (uint8_t)idx; usedIndices[1] = indices[i]; usedIndices[2] = indices[0];
            break;
        }
    }
    Spec<16> ret(0.0f);
    if (usedIndices[0] == 255) return ret;          // the reference asserts here (no triangle of the fan contains the point)
    for (int i = 0; i < 16; ++i) {
        float p = (wls.lambdas[i] - 360.0f) / (830.0f - 360.0f);
        float sBinF = p * (NumWavelengthSamples - 1);
        uint32_t sBin = (uint32_t)sBinF;
        uint32_t sBinNext = (sBin + 1 < NumWavelengthSamples) ? (sBin + 1) : (NumWavelengthSamples - 1);
        float t = sBinF - sBin;
        for (int j = 0; j < 4; ++j) {
            if (usedIndices[j] == 255) continue;
            const float* spectrum = &sc.pointSpectrum[(size_t)usedIndices[j] * NumWavelengthSamples];
            ret[i] += weights[j] * (spectrum[sBin] * (1 - t) + spectrum[sBinNext] * t);
        }
    }
    return ret * scale;
}
// spectral build: the texel is (u, v, s) (image_textures.cpp:23-32)
inline Spec<16> envEmittance16(const Scene& s, float tcU, float tcV, const Wls<16>& wls) {
    float u = std::fmod(tcU, 1.0f), v = std::fmod(tcV, 1.0f);
    u += u < 0 ? 1.0f : 0.0f;
    v += v < 0 ? 1.0f : 0.0f;
    uint32_t px = std::min((uint32_t)(s.envWidth * u), s.envWidth - 1);
    uint32_t py = std::min((uint32_t)(s.envHeight * v), s.envHeight - 1);
    const float* t = &s.envTexels[((size_t)py * s.envWidth + px) * 3];
    const float kEqualEnergyReflectance = 0.009355121400914532f;        // Upsampling::EqualEnergyReflectance, Spectrum.h
    Spec<16> tex = evaluateUpsampled(s, t[0], t[1], t[2] / kEqualEnergyReflectance, wls);
    return ((float)M_PI * tex) * s.envScale;                            // IBLEmission::emittance
}
template <int N> Spec<N> envEmittanceT(const Scene& s, float u, float v, const Wls<N>& wls);
template <> Spec<3> envEmittanceT<3>(const Scene& s, float u, float v, const Wls<3>&) { return envEmittance(s, u, v); }
template <> Spec<16> envEmittanceT<16>(const Scene& s, float u, float v, const Wls<16>& wls) { return envEmittance16(s, u, v, wls); }

// Surface/TriangleMesh.cpp:180-215  Triangle::getSurfacePoint (+ SingleSurfaceObject :60-63).
// texCoord0Dir is not restated: no lobe on this path reads it.
void getSurfacePoint(const Scene& s, const Isect& isect, SurfPt* sp) {
    if (isect.tri == kEnvObject) {
        // InfiniteSphere::getSurfacePoint, Surface/InfiniteSphere.cpp:48-59; texCoord from intersect :43
        sp->p = isect.p;
        sp->atInfinity = true;
        sp->gNormal = isect.gNormal;
        sp->u = isect.u;
        sp->v = isect.v;
        sp->texU = (float)(isect.u / (2 * M_PI));
        sp->texV = (float)(isect.v / M_PI);
        V3 tc0(-std::cos(sp->u), 0.0f, -std::sin(sp->u));
        sp->frame.x = tc0;
        sp->frame.z = sp->gNormal;
        sp->frame.y = cross(sp->frame.z, sp->frame.x);
        sp->tri = kEnvObject;
        return;
    }
    sp->p = isect.p;
    sp->atInfinity = false;
    sp->gNormal = isect.gNormal;
    sp->u = isect.u;
    sp->v = isect.v;
    const Tri& tri = s.tris[isect.tri];
    float b0 = isect.u, b1 = isect.v;
    float b2 = 1.0f - b0 - b1;
    sp->frame.z = normalize(b0 * vnrm(s, tri.v[0]) + b1 * vnrm(s, tri.v[1]) + b2 * vnrm(s, tri.v[2]));
    sp->frame.x = normalize(b0 * vtan(s, tri.v[0]) + b1 * vtan(s, tri.v[1]) + b2 * vtan(s, tri.v[2]));
    float dotNT = dot(sp->frame.z, sp->frame.x);
    if (std::fabs(dotNT) >= 0.01f)
        sp->frame.x = normalize(sp->frame.x - dotNT * sp->frame.z);
    sp->frame.y = cross(sp->frame.z, sp->frame.x);
    sp->tri = isect.tri;
    sp->texU = isect.texU;
    sp->texV = isect.texV;
    // BumpSingleSurfaceObject::getSurfacePoint, Core/SurfaceObject.cpp:123-134
    if (const slrhip_texture* nm = normalMapOf(s, s.materials[tri.material])) {
        V3 nLocal = checkerNormal(*nm, sp->texU, sp->texV);
        V3 tLocal = V3(1, 0, 0) - dot(nLocal, V3(1, 0, 0)) * nLocal;
        V3 bLocal = V3(0, 1, 0) - dot(nLocal, V3(0, 1, 0)) * nLocal;
        V3 t = normalize(sp->frame.fromLocal(tLocal));
        V3 b = normalize(sp->frame.fromLocal(bLocal));
        V3 n = normalize(sp->frame.fromLocal(nLocal));
        sp->frame.x = t;
        sp->frame.y = b;
        sp->frame.z = n;
    }
    if (isect.inst >= 0) {
        // TransformedSurfaceObject::getSurfacePoint (SurfaceObject.cpp:329-336): *surfPt = sampledTF * *surfPt, geometry.cpp:63-78
        const slrhip_instance& in = s.instances[isect.inst];
        sp->p = mulPoint(in.local_to_world, sp->p);
        sp->gNormal = normalize(mulNormal(in.world_to_local, sp->gNormal));
        sp->frame.x = normalize(mulVector(in.local_to_world, sp->frame.x));
        sp->frame.y = normalize(mulVector(in.local_to_world, sp->frame.y));
        sp->frame.z = normalize(mulVector(in.local_to_world, sp->frame.z));
    }
}

// Surface/TriangleMesh.cpp:217-222  Triangle::area
inline float triArea(const Scene& s, uint32_t ti) {
    const Tri& tri = s.tris[ti];
    V3 p0 = vpos(s, tri.v[0]), p1 = vpos(s, tri.v[1]), p2 = vpos(s, tri.v[2]);
    return 0.5f * length(cross(p1 - p0, p2 - p0));
}

// Surface/TriangleMesh.cpp:224-255  Triangle::sample
void triSample(const Scene& s, uint32_t ti, float u0, float u1, SurfPt* sp, float* areaPDF) {
    float b0, b1, b2;
    uniformSampleTriangle(u0, u1, &b0, &b1);
    b2 = 1.0f - b0 - b1;
    const Tri& tri = s.tris[ti];
    V3 p0 = vpos(s, tri.v[0]), p1 = vpos(s, tri.v[1]), p2 = vpos(s, tri.v[2]);
    sp->p = b0 * p0 + b1 * p1 + b2 * p2;
    sp->atInfinity = false;
    sp->gNormal = normalize(cross(p1 - p0, p2 - p0));    // Vector3::normalize(): same reciprocal multiply
    sp->u = b0;
    sp->v = b1;
    sp->frame.z = normalize(b0 * vnrm(s, tri.v[0]) + b1 * vnrm(s, tri.v[1]) + b2 * vnrm(s, tri.v[2]));
    sp->frame.x = normalize(b0 * vtan(s, tri.v[0]) + b1 * vtan(s, tri.v[1]) + b2 * vtan(s, tri.v[2]));
    sp->frame.y = cross(sp->frame.z, sp->frame.x);
    sp->tri = ti;
    *areaPDF = 1.0f / triArea(s, ti);
}

// Core/SurfaceObject.cpp:418-430  Scene::testVisibility (finite light point)
bool testVisibility(const Scene& s, const SurfPt& shdP, const SurfPt& lightP, slr_oracle_counters* ctr) {
    if (ctr) ++ctr->shadow_rays;
    Ray ray;
    if (lightP.atInfinity) {
        ray.org = shdP.p; ray.dir = normalize(lightP.p); ray.distMin = 0.0001f; ray.distMax = FLT_MAX;
    }
    else {
        float dist = length(shdP.p - lightP.p);                          // distance(lightP.p, shdP.p) Point3.h:99-101
        ray.org = shdP.p;
        ray.dir = (lightP.p - shdP.p) / dist;
        ray.distMin = 0.0001f;
        ray.distMax = dist * (1 - 0.0001f);
    }
    Isect isect;
    return !aggregateIntersect(s, ray, &isect, ctr);
}

// ------------------------------------------------------------------------------------------
// Spectra / materials (RGB mode: InputSpectrum = RGBTemplate, evaluate() returns itself,
// RGBTypes.h:124-126; ConstantSpectrumTexture constant_textures.h:16-31)
// ------------------------------------------------------------------------------------------
template <int N> struct EvalSpectrum;

template <> struct EvalSpectrum<3> {
    static Spec<3> eval(const Scene& s, int32_t idx, const Wls<3>&) {
        Spec<3> r;
        const slrhip_spectrum& sp = s.spectra[idx];
        r.c[0] = sp.rgb[0]; r.c[1] = sp.rgb[1]; r.c[2] = sp.rgb[2];
        return r;
    }
};

// Spectral mode: ConstantSpectrumTexture::evaluate -> ContinuousSpectrum::evaluate(wls)
template <> struct EvalSpectrum<16> {
    static Spec<16> eval(const Scene& s, int32_t idx, const Wls<16>& wls) {
        const int N = 16;
        const slrhip_spectrum& sp = s.spectra[idx];
        const float* data = s.spectrumData.data() + sp.data_offset;
        Spec<16> ret(0.0f);
        switch (sp.kind) {
        case SLRHIP_SPECTRUM_REGULAR: {
            // RegularContinuousSpectrumTemplate::evaluate, SpectrumTypes.h:90-109
            const float minLambda = sp.lambda_min, maxLambda = sp.lambda_max;
            const uint32_t numSamples = sp.num_samples;
            const float* values = data;
            for (int i = 0; i < N; ++i) {
                float binF = (wls.lambdas[i] - minLambda) / (maxLambda - minLambda) * (numSamples - 1);
                if (binF <= 0.0f) { ret[i] = values[0]; continue; }
                else if (binF >= numSamples - 1) { ret[i] = values[numSamples - 1]; continue; }
                int32_t bin = int32_t(binF);
                float t = binF - bin;
                ret[i] = (1 - t) * values[bin] + t * values[bin + 1];
            }
            return ret;
        }
        case SLRHIP_SPECTRUM_IRREGULAR: {
            // IrregularContinuousSpectrumTemplate::evaluate, SpectrumTypes.h:139-160
            const uint32_t numSamples = sp.num_samples;
            const float* lambdas = data;
            const float* values = data + numSamples;
            uint32_t searchBase = 0;
            for (int i = 0; i < N; ++i) {
                int32_t lowIdx = std::max((int32_t)std::distance(lambdas, std::lower_bound(lambdas + searchBase, lambdas + numSamples, wls.lambdas[i])) - 1, 0);
                searchBase = lowIdx;
                if (lowIdx >= (int32_t)numSamples - 1) { ret[i] = values[numSamples - 1]; continue; }
                float t = (wls.lambdas[i] - lambdas[lowIdx]) / (lambdas[lowIdx + 1] - lambdas[lowIdx]);
                if (t <= 0.0f) { ret[i] = values[0]; continue; }
                ret[i] = (1 - t) * values[lowIdx] + t * values[lowIdx + 1];
            }
            return ret;
        }
        case SLRHIP_SPECTRUM_UPSAMPLED: {
            // UpsampledContinuousSpectrumTemplate::evaluate, SpectrumTypes.h:239-339.  The cell lookup and the
            // barycentric weights (:241-312) depend only on (u, v): resolved by the scene builder into
            // `weights` + the 3 or 4 data-point spectra (slr_amd/spectra.py); the wavelength loop is here.
            const uint32_t numPoints = sp.reserved;             // 0: outside the grid -> Zero (:241-242)
            if (numPoints == 0) return Spec<16>(0.0f);
            const uint32_t NumWavelengthSamples = sp.num_samples;    // 95
            const float* weights = data;
            const float* spectra = data + 4;
            for (int i = 0; i < N; ++i) {
                float lambda = wls.lambdas[i];
                float p = (lambda - 360.0f) / (830.0f - 360.0f);
                float sBinF = p * (NumWavelengthSamples - 1);
                uint32_t sBin = (uint32_t)sBinF;
                uint32_t sBinNext = (sBin + 1 < NumWavelengthSamples) ? (sBin + 1) : (NumWavelengthSamples - 1);
                float t = sBinF - sBin;
                for (uint32_t j = 0; j < numPoints; ++j)       // samples are stored [bin][point] (include/slrhip.h)
                    ret[i] += weights[j] * (spectra[4 * sBin + j] * (1 - t) + spectra[4 * sBinNext + j] * t);
            }
            return ret * sp.scale;
        }
        default:
            return Spec<16>(0.0f);
        }
    }
};

enum : uint32_t {   // Core/directional_distribution_functions.h:18-51
    DT_LowFreq = 1 << 0, DT_HighFreq = 1 << 1, DT_Delta0D = 1 << 2, DT_Delta1D = 1 << 3,
    DT_NonDelta = DT_LowFreq | DT_HighFreq, DT_Delta = DT_Delta0D | DT_Delta1D, DT_AllFreq = DT_NonDelta | DT_Delta,
    DT_Reflection = 1 << 4, DT_Transmission = 1 << 5, DT_WholeSphere = DT_Reflection | DT_Transmission,
    DT_All = DT_AllFreq | DT_WholeSphere, DT_Dispersive = 1 << 6
};
inline bool dtMatches(uint32_t type, uint32_t t) { uint32_t res = type & t; return (res & DT_WholeSphere) && (res & DT_AllFreq); } // :83
inline bool dtIsDelta(uint32_t v) { return (v & DT_Delta) && !(v & DT_NonDelta); }        // :86
inline bool dtIsDispersive(uint32_t v) { return (v & DT_Dispersive) != 0; }


// std::max / std::min as the reference uses them: (a < b) ? b : a and (b < a) ? b : a
inline float stdmax(float a, float b) { return (a < b) ? b : a; }
inline float stdmin(float a, float b) { return (b < a) ? b : a; }

template <int N>
struct BSDFQuery {   // DDF.h:118-126
    V3 dir_sn, gNormal_sn;
    int16_t wlHint;
    uint32_t flags;
};
struct BSDFResult {  // DDF.h:140-146
    V3 dir_sn;
    float dirPDF;
    uint32_t dirType;
};

// Per-hit BSDF (SurfacePoint::createBSDF geometry.cpp:56-58 -> material->getBSDF)
template <int N>
struct BSDF {
    uint32_t kind;      // SLRHIP_MATERIAL_*
    uint32_t type;      // DirectionType of the lobe
    Spec<N> a, b, c;    // matte: a = R;  metal: a = coeffR, b = eta, c = k;  glass: a = coeff, b = etaExt, c = etaInt
    float param;        // matte: sigma (< 0: Lambert);  microfacet: alpha_g;  Ward: anisoX;  Ashikhmin: nu
    float param2;       // Ward: anisoY;  Ashikhmin: nv
    float onA, onB;     // Oren-Nayar m_A, m_B (OrenNayerBRDF.h:28-30)
};

// OrenNayerBRDF::sampleInternal / evaluateInternal share this term (OrenNayerBRDF.cpp:19-27,46-53).
// "sin" terms are 1 - z^2 without the square root, as in the reference.
template <int N>
inline Spec<N> orenNayar(const BSDF<N>& f, V3 dirI, V3 dirO, bool guardNonFinite) {
    float sinThetaI = 1.0f - dirI.z * dirI.z;
    float sinThetaO = 1.0f - dirO.z * dirO.z;
    float absTanThetaI = sinThetaI / std::abs(dirI.z);
    float absTanThetaO = sinThetaO / std::abs(dirO.z);
    float sinAlpha = stdmax(sinThetaI, sinThetaO);
    float tanBeta = stdmin(absTanThetaI, absTanThetaO);
    float cos_dAzimuth = (dirI.x * dirO.x + dirI.y * dirO.y) / (sinThetaI * sinThetaO);
    if (guardNonFinite && !std::isfinite(cos_dAzimuth)) cos_dAzimuth = 0.0f;
    return f.a * (float)((double)(f.onA + f.onB * stdmax(0.0f, cos_dAzimuth) * sinAlpha * tanBeta) / M_PI);
}

// Core/directional_distribution_functions.cpp:68-78  FresnelConductor::evaluate
template <int N>
Spec<N> fresnelConductor(const Spec<N>& eta, const Spec<N>& k, float cosEnter) {
    cosEnter = std::fabs(cosEnter);
    float cosEnter2 = cosEnter * cosEnter;
    Spec<N> _2EtaCosEnter = 2.0f * eta * cosEnter;
    Spec<N> tmp_f = eta * eta + k * k;
    Spec<N> tmp = tmp_f * cosEnter2;
    Spec<N> Rparl2 = (tmp - _2EtaCosEnter + 1) / (tmp + _2EtaCosEnter + 1);
    Spec<N> Rperp2 = (tmp_f - _2EtaCosEnter + cosEnter2) / (tmp_f + _2EtaCosEnter + cosEnter2);
    return (Rparl2 + Rperp2) / 2.0f;
}
// DDF.cpp:155-159
inline float fresnelEvalF(float etaEnter, float etaExit, float cosEnter, float cosExit) {
    float Rparl = ((etaExit * cosEnter) - (etaEnter * cosExit)) / ((etaExit * cosEnter) + (etaEnter * cosExit));
    float Rperp = ((etaEnter * cosEnter) - (etaExit * cosExit)) / ((etaEnter * cosEnter) + (etaExit * cosExit));
    return (Rparl * Rparl + Rperp * Rperp) / 2.0f;
}
// DDF.cpp:90-111  FresnelDielectric::evaluate(cosEnter)
template <int N>
Spec<N> fresnelDielectric(const Spec<N>& etaExt, const Spec<N>& etaInt, float cosEnter) {
    cosEnter = std::min(1.0f, std::max(-1.0f, cosEnter));     // std::clamp defines.h:118-121
    bool entering = cosEnter > 0.0f;
    const Spec<N>& eEnter = entering ? etaExt : etaInt;
    const Spec<N>& eExit = entering ? etaInt : etaExt;
    Spec<N> sinExit = eEnter / eExit * std::sqrt(std::fmax(0.0f, 1.0f - cosEnter * cosEnter));
    Spec<N> ret;
    cosEnter = std::fabs(cosEnter);
    for (int i = 0; i < N; ++i) {
        if (sinExit[i] >= 1.0f) ret[i] = 1.0f;
        else {
            float cosExit = std::sqrt(std::fmax(0.0f, 1.0f - sinExit[i] * sinExit[i]));
            ret[i] = fresnelEvalF(eEnter[i], eExit[i], cosEnter, cosExit);
        }
    }
    return ret;
}



// ------------------------------------------------------------------------------------------
// GGX, Core/directional_distribution_functions.cpp:162-268.  std::pow(float, int) is the double
// pow; unqualified cos/sin/tan inside namespace SLR are the double C functions; std::acos,
// std::atan2, std::tan, std::cos, std::sin on floats are the float overloads.
// ------------------------------------------------------------------------------------------
struct GGX {
    float alpha_g;
    // :176-183
    float evaluate(V3 m) const {
        if (m.z <= 0) return 0.0f;
        float theta_m = std::acos(m.z);
        float cosTheta_m = m.z;
        float tanTheta_m = std::tan(theta_m);
        return (float)((double)(alpha_g * alpha_g) /
                       (M_PI * std::pow((double)cosTheta_m, 4.0) * std::pow((double)(alpha_g * alpha_g + tanTheta_m * tanTheta_m), 2.0)));
    }
    // :264-268
    float evaluateSmithG1(V3 v, V3 m) const {
        float chi = (dot(v, m) / v.z) > 0 ? 1 : 0;
        float theta_v = std::acos(std::min(1.0f, std::max(-1.0f, v.z)));
        return (float)((double)(chi * 2) / (1 + std::sqrt(1 + std::pow((double)(alpha_g * std::tan(theta_v)), 2.0))));
    }
    // :260-262
    float evaluatePDF(V3 v, V3 m) const { return evaluateSmithG1(v, m) * absDot(v, m) * evaluate(m) / std::abs(v.z); }
    // :191-258  Heitz-14 visible-normal sampling
    float sample(V3 v, float u0, float u1, V3* m, float* normalPDF) const {
        float alpha_gx = alpha_g, alpha_gy = alpha_g;
        V3 sv = normalize(V3(alpha_gx * v.x, alpha_gy * v.y, v.z));
        float theta_sv = std::acos(sv.z);
        float phi_sv = std::atan2(sv.y, sv.x);
        if (sv.z > 0.99999f) { theta_sv = 0.0f; phi_sv = 0.0f; }
        float slope_x, slope_y;
        if (theta_sv < 0.0001) {
            const float r = std::sqrt(u0 / (1 - u0));
            const float phi = (float)(2 * M_PI * u1);
            slope_x = (float)(r * ::cos((double)phi));
            slope_y = (float)(r * ::sin((double)phi));
        }
        else {
            const float tan_theta_i = (float)::tan((double)theta_sv);
            const float a = 1 / tan_theta_i;
            const float G1 = (float)(2 / (1 + std::sqrt(1.0 + 1.0 / (a * a))));
            const float A = (float)(2.0 * u0 / G1 - 1.0);
            const float tmp = (float)(1.0 / (A * A - 1.0));
            const float B = tan_theta_i;
            const float D = std::sqrt(B * B * tmp * tmp - (A * A - B * B) * tmp);
            const float slope_x_1 = B * tmp - D;
            const float slope_x_2 = B * tmp + D;
            slope_x = (A < 0 || slope_x_2 > 1.0 / tan_theta_i) ? slope_x_1 : slope_x_2;
            if (u0 == 0) slope_x = 0;
            float S;
            if (u1 > 0.5) { S = 1.0; u1 = (float)(2.0 * (u1 - 0.5)); }
            else { S = -1.0; u1 = (float)(2.0 * (0.5 - u1)); }
            const float z = (float)((u1 * (u1 * (u1 * 0.27385 - 0.73369) + 0.46341)) / (u1 * (u1 * (u1 * 0.093073 + 0.309420) - 1.000000) + 0.597999));
            slope_y = (float)(S * z * std::sqrt(1.0 + slope_x * slope_x));
        }
        float tmp = std::cos(phi_sv) * slope_x - std::sin(phi_sv) * slope_y;
        slope_y = std::sin(phi_sv) * slope_x + std::cos(phi_sv) * slope_y;
        slope_x = tmp;
        slope_x *= alpha_gx;
        slope_y *= alpha_gy;
        *m = normalize(V3(-slope_x, -slope_y, 1));
        float D = evaluate(*m);
        *normalPDF = evaluateSmithG1(v, *m) * absDot(v, *m) * D / std::abs(v.z);
        return D;
    }
};

// DDF.cpp:80-88 / :113-129  per-wavelength Fresnel
template <int N>
inline float fresnelDielectric1(const Spec<N>& etaExt, const Spec<N>& etaInt, float cosEnter, int wlIdx) {
    cosEnter = std::min(1.0f, std::max(-1.0f, cosEnter));
    bool entering = cosEnter > 0.0f;
    const float eEnter = entering ? etaExt[wlIdx] : etaInt[wlIdx];
    const float eExit = entering ? etaInt[wlIdx] : etaExt[wlIdx];
    float sinExit = eEnter / eExit * std::sqrt(std::fmax(0.0f, 1.0f - cosEnter * cosEnter));
    cosEnter = std::fabs(cosEnter);
    if (sinExit >= 1.0f) return 1.0f;
    float cosExit = std::sqrt(std::fmax(0.0f, 1.0f - sinExit * sinExit));
    return fresnelEvalF(eEnter, eExit, cosEnter, cosExit);
}

// ---- ModifiedWardDurBRDF (BSDFs/ModifiedWardDurBRDF.cpp:11-87): a = R, param = anisoX, param2 = anisoY ------------------------
template <int N>
inline float wardTerms(const BSDF<N>& f, V3 halfv, V3 dirL, float* dotHI, float* dotHN) {
    float hx_ax = halfv.x / f.param;
    float hy_ay = halfv.y / f.param2;
    *dotHN = std::fabs(halfv.z);
    *dotHI = dot(halfv, dirL);
    return std::exp(-(hx_ax * hx_ax + hy_ay * hy_ay) / (*dotHN * *dotHN));      // the numerator
}
// ---- AshikhminShirleyBRDF (BSDFs/AshikhminShirleyBRDF.cpp:12-170): a = Rs, b = Rd, param = nu, param2 = nv ----------------------
// std::pow(float, int) promotes to double (C++11), so the Schlick / Fresnel-like terms are evaluated in double
template <int N>
inline void ashikhminWeights(const BSDF<N>& f, int16_t wlHint, float absCos, float* specularWeight, float* diffuseWeight) {
    float iRs = importance(f.a, wlHint);
    float iRd = importance(f.b, wlHint);
    *specularWeight = (float)(iRs + (1 - iRs) * std::pow(1.0f - absCos, 5));
    float transmissionTerm = (float)(1 - std::pow(1 - absCos * 0.5f, 5));
    *diffuseWeight = 28 * iRd / 23 * (1 - iRs) * transmissionTerm * transmissionTerm;
}
// commonTerm = specular direction PDF (:41-43,:116-118,:138-140)
template <int N>
inline float ashikhminCommon(const BSDF<N>& f, V3 halfv, float dotHV) {
    float exp = (f.param * halfv.x * halfv.x + f.param2 * halfv.y * halfv.y) / (1 - halfv.z * halfv.z);
    return (float)(std::sqrt((f.param + 1) * (f.param2 + 1)) / (8 * M_PI * dotHV) * std::pow(std::fabs(halfv.z), exp));
}
template <int N>
inline Spec<N> ashikhminFs(const BSDF<N>& f, float commonTerm, float dotHV, float zQuery, float zDir) {
    Spec<N> F = f.a + (Spec<N>(1.0f) - f.a) * (float)std::pow(1.0f - dotHV, 5);
    Spec<N> specular_fs = commonTerm / std::fmax(std::fabs(zQuery), std::fabs(zDir)) * F;
    Spec<N> diffuse_fs = (28 * f.b / (float)(23 * M_PI) * (Spec<N>(1.0f) - f.a) *
                          (float)(1.0f - std::pow(1.0f - std::fabs(zQuery) / 2, 5)) *
                          (float)(1.0f - std::pow(1.0f - std::fabs(zDir) / 2, 5)));
    return specular_fs + diffuse_fs;
}

// sampleInternal of each lobe.  Returns fs_sn; result->dirPDF == 0 signals failure.
template <int N>
Spec<N> bsdfSampleInternal(const BSDF<N>& f, const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result) {
    switch (f.kind) {
    case SLRHIP_MATERIAL_MATTE: {
        if (f.param >= 0.0f) {
            // BSDFs/OrenNayerBRDF.cpp:12-34
            bool frontSide = dot(q.dir_sn, q.gNormal_sn) > 0;
            result->dir_sn = cosineSampleHemisphere(uDir[0], uDir[1]);
            result->dirPDF = (float)((double)result->dir_sn.z / M_PI);
            result->dirType = f.type;
            result->dir_sn.z *= frontSide ? 1 : -1;
            return orenNayar(f, result->dir_sn, q.dir_sn, true);
        }
        // BSDFs/basic_BSDFs.cpp:12-26  LambertianBRDF::sampleInternal
        result->dir_sn = cosineSampleHemisphere(uDir[0], uDir[1]);
        result->dirPDF = (float)((double)result->dir_sn.z / M_PI);
        result->dirType = f.type;
        result->dir_sn.z *= dot(q.dir_sn, q.gNormal_sn) > 0 ? 1 : -1;
        return f.a / (float)M_PI;
    }
    case SLRHIP_MATERIAL_WARD: {
        // ModifiedWardDurBRDF.cpp:11-40
        float quad = (float)(2 * M_PI * uDir[1]);
        float phi_h = std::atan2(f.param2 * std::sin(quad), f.param * std::cos(quad));
        float cosphi_ax = std::cos(phi_h) / f.param;
        float sinphi_ay = std::sin(phi_h) / f.param2;
        float theta_h = std::atan(std::sqrt(-std::log(1 - uDir[0]) / (cosphi_ax * cosphi_ax + sinphi_ay * sinphi_ay)));
        V3 halfv(std::sin(theta_h) * std::cos(phi_h), std::sin(theta_h) * std::sin(phi_h), std::cos(theta_h));
        halfv.z *= q.dir_sn.z > 0 ? 1 : -1;
        result->dir_sn = 2 * dot(q.dir_sn, halfv) * halfv - q.dir_sn;
        if (result->dir_sn.z * q.dir_sn.z <= 0) { result->dirPDF = 0.0f; return Spec<N>(); }
        float dotHI, dotHN;
        float numerator = wardTerms(f, halfv, result->dir_sn, &dotHI, &dotHN);
        float commonDenom = (float)(4 * M_PI * f.param * f.param2 * dotHI * dotHN * dotHN * dotHN);
        result->dirPDF = numerator / commonDenom;
        result->dirType = f.type;
        return f.a * (numerator / (commonDenom * dotHI * dotHN));
    }
    case SLRHIP_MATERIAL_ASHIKHMIN: {
        // AshikhminShirleyBRDF.cpp:12-92
        float specularWeight, diffuseWeight;
        ashikhminWeights(f, q.wlHint, std::fabs(q.dir_sn.z), &specularWeight, &diffuseWeight);
        float sumWeights = specularWeight + diffuseWeight;
        float specularDirPDF, diffuseDirPDF;
        Spec<N> fs;
        if (uComponent * sumWeights < specularWeight) {
            result->dirType = DT_Reflection | DT_HighFreq;
            float quad = (float)(2 * M_PI * uDir[1]);
            float phi_h = std::atan2(std::sqrt(f.param + 1) * std::sin(quad), std::sqrt(f.param2 + 1) * std::cos(quad));
            float cosphi = std::cos(phi_h);
            float sinphi = std::sin(phi_h);
            float theta_h = std::acos(std::pow(1 - uDir[0], 1.0f / (f.param * cosphi * cosphi + f.param2 * sinphi * sinphi + 1)));
            if (q.dir_sn.z < 0) theta_h = (float)(M_PI - theta_h);
            V3 halfv(std::sin(theta_h) * std::cos(phi_h), std::sin(theta_h) * std::sin(phi_h), std::cos(theta_h));
            result->dir_sn = 2 * dot(q.dir_sn, halfv) * halfv - q.dir_sn;
            if (result->dir_sn.z * q.dir_sn.z <= 0) { result->dirPDF = 0.0f; return Spec<N>(); }
            float dotHV = dot(halfv, q.dir_sn);
            specularDirPDF = ashikhminCommon(f, halfv, dotHV);
            diffuseDirPDF = (float)(std::fabs(result->dir_sn.z) / M_PI);
            fs = ashikhminFs(f, specularDirPDF, dotHV, q.dir_sn.z, result->dir_sn.z);
        }
        else {
            result->dirType = DT_Reflection | DT_LowFreq;
            result->dir_sn = cosineSampleHemisphere(uDir[0], uDir[1]);
            diffuseDirPDF = (float)(result->dir_sn.z / M_PI);
            result->dir_sn.z *= dot(q.dir_sn, q.gNormal_sn) > 0 ? 1 : -1;
            V3 halfv = normalize(q.dir_sn + result->dir_sn);
            float dotHV = dot(halfv, q.dir_sn);
            specularDirPDF = ashikhminCommon(f, halfv, dotHV);
            fs = ashikhminFs(f, specularDirPDF, dotHV, q.dir_sn.z, result->dir_sn.z);
        }
        result->dirPDF = (specularDirPDF * specularWeight + diffuseDirPDF * diffuseWeight) / sumWeights;
        return fs;
    }
    case SLRHIP_MATERIAL_METAL: {
        // basic_BSDFs.cpp:61-71  SpecularBRDF::sampleInternal
        result->dir_sn = V3(-q.dir_sn.x, -q.dir_sn.y, q.dir_sn.z);
        result->dirPDF = 1.0f;
        result->dirType = f.type;
        return f.a * fresnelConductor(f.b, f.c, q.dir_sn.z) / std::fabs(q.dir_sn.z);
    }
    case SLRHIP_MATERIAL_GLASS: {
        // basic_BSDFs.cpp:95-149  SpecularBSDF::sampleInternal (query.flags == All, adjoint == false)
        Spec<N> F = fresnelDielectric(f.b, f.c, q.dir_sn.z);
        float reflectProb = importance(F, (uint16_t)q.wlHint);
        if (uComponent < reflectProb) {
            if (q.dir_sn.z == 0.0f) { result->dirPDF = 0.0f; return Spec<N>(); }
            result->dir_sn = V3(-q.dir_sn.x, -q.dir_sn.y, q.dir_sn.z);
            result->dirPDF = reflectProb;
            result->dirType = DT_Reflection | DT_Delta0D;
            return f.a * F / std::fabs(q.dir_sn.z);
        }
        else {
            bool entering = q.dir_sn.z > 0.0f;
            float eEnter = entering ? f.b[q.wlHint] : f.c[q.wlHint];
            float eExit = entering ? f.c[q.wlHint] : f.b[q.wlHint];
            float sinEnter2 = 1.0f - q.dir_sn.z * q.dir_sn.z;
            float rrEta = eEnter / eExit;
            float sinExit2 = rrEta * rrEta * sinEnter2;
            if (sinExit2 >= 1.0f) { result->dirPDF = 0.0f; return Spec<N>(); }
            float cosExit = std::sqrt(std::fmax(0.0f, 1.0f - sinExit2));
            if (entering) cosExit = -cosExit;
            result->dir_sn = V3(rrEta * -q.dir_sn.x, rrEta * -q.dir_sn.y, cosExit);
            result->dirPDF = 1.0f - reflectProb;
            result->dirType = DT_Transmission | DT_Delta0D | (dtIsDispersive(f.type) ? (uint32_t)DT_Dispersive : 0u);
            Spec<N> ret;
            ret[q.wlHint] = f.a[q.wlHint] * (1.0f - F[q.wlHint]);
            ret[q.wlHint] *= (eEnter * eEnter) / (eExit * eExit);
            return ret / std::fabs(cosExit);
        }
    }
    case SLRHIP_MATERIAL_MICROFACET_METAL: {
        // BSDFs/MicrofacetBSDF.cpp:11-45  MicrofacetBRDF::sampleInternal
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        V3 m; float mPDF;
        float D = D_.sample((float)sign * q.dir_sn, uDir[0], uDir[1], &m, &mPDF);
        float dotHV = dot(q.dir_sn, m);
        if (dotHV * sign <= 0) { result->dirPDF = 0.0f; return Spec<N>(); }
        result->dir_sn = 2 * dotHV * m - q.dir_sn;
        if (result->dir_sn.z * q.dir_sn.z <= 0) { result->dirPDF = 0.0f; return Spec<N>(); }
        float commonPDFTerm = 1.0f / (4 * dotHV * sign);
        result->dirPDF = commonPDFTerm * mPDF;
        result->dirType = f.type;
        Spec<N> F = fresnelConductor(f.b, f.c, dotHV);
        float G = D_.evaluateSmithG1(q.dir_sn, m) * D_.evaluateSmithG1(result->dir_sn, m);
        return F * D * G / (4 * q.dir_sn.z * result->dir_sn.z);
    }
    case SLRHIP_MATERIAL_MICROFACET_GLASS: {
        // MicrofacetBSDF.cpp:113-196  MicrofacetBSDF::sampleInternal (flags = All, adjoint = false)
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        const Spec<N>& eEnter = entering ? f.b : f.c;
        const Spec<N>& eExit = entering ? f.c : f.b;
        V3 m; float mPDF;
        float D = D_.sample((float)sign * q.dir_sn, uDir[0], uDir[1], &m, &mPDF);
        float dotHV = dot(q.dir_sn, m);
        if (dotHV * sign <= 0 || std::isnan(D)) { result->dirPDF = 0.0f; return Spec<N>(); }
        Spec<N> F = fresnelDielectric(f.b, f.c, dotHV);
        float reflectProb = importance(F, (uint16_t)q.wlHint);
        if (uComponent < reflectProb) {
            result->dir_sn = 2 * dotHV * m - q.dir_sn;
            if (result->dir_sn.z * q.dir_sn.z <= 0) { result->dirPDF = 0.0f; return Spec<N>(); }
            float commonPDFTerm = reflectProb / (4 * dotHV * sign);
            result->dirPDF = commonPDFTerm * mPDF;
            result->dirType = DT_Reflection | DT_HighFreq;
            float G = D_.evaluateSmithG1(q.dir_sn, m) * D_.evaluateSmithG1(result->dir_sn, m);
            return F * D * G / (4 * q.dir_sn.z * result->dir_sn.z);
        }
        else {
            float recRelIOR = eEnter[q.wlHint] / eExit[q.wlHint];
            float innerRoot = 1 + recRelIOR * recRelIOR * (dotHV * dotHV - 1);
            if (innerRoot < 0) { result->dirPDF = 0.0f; return Spec<N>(); }
            result->dir_sn = (recRelIOR * dotHV - sign * std::sqrt(innerRoot)) * m - recRelIOR * q.dir_sn;
            if (result->dir_sn.z * q.dir_sn.z >= 0) { result->dirPDF = 0.0f; return Spec<N>(); }
            float dotHL = dot(result->dir_sn, m);
            float commonPDFTerm = (float)((double)(1 - reflectProb) / std::pow((double)(eEnter[q.wlHint] * dotHV + eExit[q.wlHint] * dotHL), 2.0));
            result->dirPDF = commonPDFTerm * mPDF * eExit[q.wlHint] * eExit[q.wlHint] * std::fabs(dotHL);
            result->dirType = DT_Transmission | DT_HighFreq;
            Spec<N> ret;
            for (int wlIdx = 0; wlIdx < N; ++wlIdx) {
                V3 m_wl = normalize(-(eEnter[wlIdx] * q.dir_sn + eExit[wlIdx] * result->dir_sn));
                float dotHV_wl = dot(q.dir_sn, m_wl);
                float dotHL_wl = dot(result->dir_sn, m_wl);
                float F_wl = fresnelDielectric1(f.b, f.c, dotHV_wl, wlIdx);
                float G_wl = D_.evaluateSmithG1(q.dir_sn, m_wl) * D_.evaluateSmithG1(result->dir_sn, m_wl);
                float D_wl = D_.evaluate(m_wl);
                ret[wlIdx] = (float)((double)(std::fabs(dotHV_wl * dotHL_wl) * (1 - F_wl) * G_wl * D_wl) /
                                     std::pow((double)(eEnter[wlIdx] * dotHV_wl + eExit[wlIdx] * dotHL_wl), 2.0));
            }
            ret = ret / std::fabs(q.dir_sn.z * result->dir_sn.z);
            ret = ret * (eEnter * eEnter);
            return ret;
        }
    }
    default:
        result->dirPDF = 0.0f;
        return Spec<N>();
    }
}

// DDF.h:231-246  BSDF::sample (query.flags = All, adjoint = false)
template <int N>
Spec<N> bsdfSample(const BSDF<N>& f, const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result) {
    if (!dtMatches(f.type, q.flags)) { result->dirPDF = 0.0f; result->dirType = 0; return Spec<N>(); }
    result->dirPDF = 0.0f;
    Spec<N> fs_sn = bsdfSampleInternal(f, q, uComponent, uDir, result);
    if (result->dirPDF == 0.0f)   // reference multiplies by a correction of an unset direction; the caller breaks on dirPDF == 0
        return Spec<N>();
    float snCorrection = std::fabs(result->dir_sn.z / dot(result->dir_sn, q.gNormal_sn));
    return fs_sn * snCorrection;
}

// evaluateInternal of each lobe; `flags` = the query's flags after the caller's side test.
template <int N>
Spec<N> bsdfEvaluateInternal(const BSDF<N>& f, const BSDFQuery<N>& q, uint32_t flags, V3 dir) {
    Spec<N> fs_sn;
    switch (f.kind) {
    case SLRHIP_MATERIAL_MATTE:
        // basic_BSDFs.cpp:28-39  LambertianBRDF::evaluateInternal / OrenNayerBRDF.cpp:36-56
        if (q.dir_sn.z * dir.z <= 0.0f) fs_sn = Spec<N>();
        else if (f.param >= 0.0f) fs_sn = orenNayar(f, dir, q.dir_sn, false);
        else fs_sn = f.a / (float)M_PI;
        break;
    case SLRHIP_MATERIAL_WARD: {
        // ModifiedWardDurBRDF.cpp:42-59
        if (dir.z * q.dir_sn.z <= 0) { fs_sn = Spec<N>(); break; }
        V3 halfv = normalize(q.dir_sn + dir);
        float dotHI, dotHN;
        float numerator = wardTerms(f, halfv, dir, &dotHI, &dotHN);
        float denominator = (float)(4 * M_PI * f.param * f.param2 * dotHI * dotHI * dotHN * dotHN * dotHN * dotHN);
        fs_sn = f.a * numerator / denominator;
        break;
    }
    case SLRHIP_MATERIAL_ASHIKHMIN: {
        // AshikhminShirleyBRDF.cpp:94-113
        if (dir.z * q.dir_sn.z <= 0) { fs_sn = Spec<N>(); break; }
        V3 halfv = normalize(q.dir_sn + dir);
        float dotHV = dot(halfv, q.dir_sn);
        fs_sn = ashikhminFs(f, ashikhminCommon(f, halfv, dotHV), dotHV, q.dir_sn.z, dir.z);
        break;
    }
    case SLRHIP_MATERIAL_MICROFACET_METAL: {
        // MicrofacetBSDF.cpp:47-71  MicrofacetBRDF::evaluateInternal
        if (dir.z * q.dir_sn.z <= 0) { fs_sn = Spec<N>(); break; }
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        V3 m = (float)sign * normalize(q.dir_sn + dir);
        float dotHV = dot(q.dir_sn, m);
        float D = D_.evaluate(m);
        Spec<N> F = fresnelConductor(f.b, f.c, dotHV);
        float G = D_.evaluateSmithG1(q.dir_sn, m) * D_.evaluateSmithG1(dir, m);
        fs_sn = F * D * G / (4 * q.dir_sn.z * dir.z);
        break;
    }
    case SLRHIP_MATERIAL_MICROFACET_GLASS: {
        // MicrofacetBSDF.cpp:198-247  MicrofacetBSDF::evaluateInternal (mQuery.flags after the side test)
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        float dotNVdotNL = dir.z * q.dir_sn.z;
        if (dotNVdotNL > 0 && dtMatches(flags, DT_Reflection | DT_AllFreq)) {
            V3 m = (float)sign * normalize(q.dir_sn + dir);
            float dotHV = dot(q.dir_sn, m);
            float D = D_.evaluate(m);
            Spec<N> F = fresnelDielectric(f.b, f.c, dotHV);
            float G = D_.evaluateSmithG1(q.dir_sn, m) * D_.evaluateSmithG1(dir, m);
            fs_sn = F * D * G / (4 * dotNVdotNL);
        }
        else if (dotNVdotNL < 0 && dtMatches(flags, DT_Transmission | DT_AllFreq)) {
            const Spec<N>& eEnter = entering ? f.b : f.c;
            const Spec<N>& eExit = entering ? f.c : f.b;
            Spec<N> ret;
            for (int wlIdx = 0; wlIdx < N; ++wlIdx) {
                V3 m_wl = normalize(-(eEnter[wlIdx] * q.dir_sn + eExit[wlIdx] * dir));
                float dotHV_wl = dot(q.dir_sn, m_wl);
                float dotHL_wl = dot(dir, m_wl);
                float F_wl = fresnelDielectric1(f.b, f.c, dotHV_wl, wlIdx);
                float G_wl = D_.evaluateSmithG1(q.dir_sn, m_wl) * D_.evaluateSmithG1(dir, m_wl);
                float D_wl = D_.evaluate(m_wl);
                ret[wlIdx] = (float)((double)(std::fabs(dotHV_wl * dotHL_wl) * (1 - F_wl) * G_wl * D_wl) /
                                     std::pow((double)(eEnter[wlIdx] * dotHV_wl + eExit[wlIdx] * dotHL_wl), 2.0));
            }
            ret = ret / std::fabs(dotNVdotNL);
            ret = ret * (eEnter * eEnter);
            fs_sn = ret;
        }
        else fs_sn = Spec<N>();
        break;
    }
    default:   // SpecularBRDF / SpecularBSDF::evaluateInternal return Zero (basic_BSDFs.cpp:73-77,151-155)
        fs_sn = Spec<N>();
        break;
    }
    return fs_sn;
}

inline uint32_t sideTest(V3 ng, V3 d0, V3 d1) {      // DDF.h:209-212
    bool reflect = dot(ng, d0) * dot(ng, d1) > 0;
    return DT_AllFreq | (reflect ? DT_Reflection : DT_Transmission);
}

// DDF.h:247-267  BSDF::evaluate
template <int N>
Spec<N> bsdfEvaluate(const BSDF<N>& f, const BSDFQuery<N>& q, V3 dir) {
    uint32_t flags = q.flags & sideTest(q.gNormal_sn, q.dir_sn, dir);
    if (!dtMatches(f.type, flags)) return Spec<N>();
    Spec<N> fs_sn = bsdfEvaluateInternal(f, q, flags, dir);
    float snCorrection = std::fabs(dir.z / dot(dir, q.gNormal_sn));
    return fs_sn * snCorrection;
}

// evaluatePDFInternal of each lobe
template <int N>
float bsdfEvaluatePDFInternal(const BSDF<N>& f, const BSDFQuery<N>& q, V3 dir) {
    switch (f.kind) {
    case SLRHIP_MATERIAL_MATTE:
        // basic_BSDFs.cpp:41-50, OrenNayerBRDF.cpp:58-66 (identical)
        if (q.dir_sn.z * dir.z <= 0.0f) return 0.0f;
        return (float)((double)std::abs(dir.z) / M_PI);
    case SLRHIP_MATERIAL_WARD: {
        // ModifiedWardDurBRDF.cpp:61-77
        if (dir.z * q.dir_sn.z <= 0) return 0.0f;
        V3 halfv = normalize(q.dir_sn + dir);
        float dotHI, dotHN;
        float numerator = wardTerms(f, halfv, dir, &dotHI, &dotHN);
        float denominator = (float)(4 * M_PI * f.param * f.param2 * dotHI * dotHN * dotHN * dotHN);
        return numerator / denominator;
    }
    case SLRHIP_MATERIAL_ASHIKHMIN: {
        // AshikhminShirleyBRDF.cpp:115-153
        if (dir.z * q.dir_sn.z <= 0) return 0.0f;
        V3 halfv = normalize(q.dir_sn + dir);
        float dotHV = dot(halfv, q.dir_sn);
        float specularDirPDF = ashikhminCommon(f, halfv, dotHV);
        float diffuseDirPDF = (float)(std::fabs(dir.z) / M_PI);
        float specularWeight, diffuseWeight;
        ashikhminWeights(f, q.wlHint, std::fabs(q.dir_sn.z), &specularWeight, &diffuseWeight);
        float sumWeights = specularWeight + diffuseWeight;
        return (specularDirPDF * specularWeight + diffuseDirPDF * diffuseWeight) / sumWeights;
    }
    case SLRHIP_MATERIAL_MICROFACET_METAL: {
        // MicrofacetBSDF.cpp:73-100
        if (dir.z * q.dir_sn.z <= 0) return 0.0f;
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        V3 m = (float)sign * normalize(q.dir_sn + dir);
        float dotHV = dot(q.dir_sn, m);
        if (dotHV * sign <= 0) return 0.0f;
        float mPDF = D_.evaluatePDF((float)sign * q.dir_sn, m);
        float commonPDFTerm = 1.0f / (4 * dotHV * sign);
        return commonPDFTerm * mPDF;
    }
    case SLRHIP_MATERIAL_MICROFACET_GLASS: {
        // MicrofacetBSDF.cpp:249-303 (query.flags = All)
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        float dotNVdotNL = dir.z * q.dir_sn.z;
        if (dotNVdotNL == 0) return 0.0f;
        const Spec<N>& eEnter = entering ? f.b : f.c;
        const Spec<N>& eExit = entering ? f.c : f.b;
        V3 m;
        if (dotNVdotNL > 0) m = (float)sign * normalize(q.dir_sn + dir);
        else m = normalize(-(eEnter[q.wlHint] * q.dir_sn + eExit[q.wlHint] * dir));
        float dotHV = dot(q.dir_sn, m);
        if (dotHV * sign <= 0) return 0.0f;
        float mPDF = D_.evaluatePDF((float)sign * q.dir_sn, m);
        Spec<N> F = fresnelDielectric(f.b, f.c, dotHV);
        float reflectProb = importance(F, (uint16_t)q.wlHint);
        if (dotNVdotNL > 0) {
            float commonPDFTerm = reflectProb / (4 * dotHV * sign);
            return commonPDFTerm * mPDF;
        }
        else {
            float dotHL = dot(dir, m);
            float commonPDFTerm = (float)((double)(1 - reflectProb) / std::pow((double)(eEnter[q.wlHint] * dotHV + eExit[q.wlHint] * dotHL), 2.0));
            return commonPDFTerm * mPDF * eExit[q.wlHint] * eExit[q.wlHint] * std::fabs(dotHL);
        }
    }
    default:
        return 0.0f;
    }
}

// DDF.h:268-279  BSDF::evaluatePDF
template <int N>
float bsdfEvaluatePDF(const BSDF<N>& f, const BSDFQuery<N>& q, V3 dir) {
    if (!dtMatches(f.type, q.flags)) return 0;
    return bsdfEvaluatePDFInternal(f, q, dir);
}

// weightInternal of each lobe, and BSDF::weight (DDF.h:280-289; non-adjoint: no correction)
template <int N>
float bsdfWeight(const BSDF<N>& f, const BSDFQuery<N>& q) {
    if (!dtMatches(f.type, q.flags)) return 0;
    switch (f.kind) {
    case SLRHIP_MATERIAL_MATTE:
        // LambertianBRDF basic_BSDFs.cpp:51-53: importance;  OrenNayerBRDF.cpp:67-69: luminance
        return f.param >= 0.0f ? luminance(f.a) : importance(f.a, (uint16_t)q.wlHint);
    case SLRHIP_MATERIAL_METAL:      // basic_BSDFs.cpp:85-87
        return importance(f.a, (uint16_t)q.wlHint) * importance(fresnelConductor(f.b, f.c, q.dir_sn.z), (uint16_t)q.wlHint);
    case SLRHIP_MATERIAL_GLASS:      // basic_BSDFs.cpp:163-165
        return importance(f.a, (uint16_t)q.wlHint);
    case SLRHIP_MATERIAL_MICROFACET_METAL:
    case SLRHIP_MATERIAL_MICROFACET_GLASS: {    // MicrofacetBSDF.cpp:102-106, 307-311
        GGX D_ = {f.param};
        bool entering = q.dir_sn.z >= 0.0f;
        int32_t sign = entering ? 1 : -1;
        return D_.evaluateSmithG1(q.dir_sn * (float)sign, V3(0, 0, 1));
    }
    case SLRHIP_MATERIAL_WARD:       // ModifiedWardDurBRDF.cpp:80-82
        return importance(f.a, (uint16_t)q.wlHint);
    case SLRHIP_MATERIAL_ASHIKHMIN: {           // AshikhminShirleyBRDF.cpp:156-165
        float specularWeight, diffuseWeight;
        ashikhminWeights(f, q.wlHint, std::fabs(q.dir_sn.z), &specularWeight, &diffuseWeight);
        return specularWeight + diffuseWeight;
    }
    default:
        return 0.0f;
    }
}

// ------------------------------------------------------------------------------------------
// MultiBSDF over (optionally inverted) lobes and over other MultiBSDFs: BSDFs/MultiBSDF.cpp, InverseBSDF basic_BSDFs.cpp:172-203.
// SummedSurfaceMaterial / MixedSurfaceMaterial always add exactly two components (SummedSurfaceMaterial.cpp:13-20,
// MixedSurfaceMaterial.cpp:14-22), so a material expression is a BINARY TREE of BSDFs whose inner nodes are MultiBSDFs.
// ------------------------------------------------------------------------------------------
template <int N>
struct AnyBSDF {
    static const int kMaxNodes = 15;
    struct Node {
        bool multi;           // MultiBSDF of children child[0], child[1]; else a lobe
        bool inverse;         // lobe only: InverseBSDF(lobe)
        int child[2];
        uint32_t type;        // m_type: the lobe's (flipped under InverseBSDF, basic_BSDFs.h:71), or the union of the components' (MultiBSDF.cpp:16)
        BSDF<N> lobe;
    };
    Node nodes[kMaxNodes];    // nodes[0] is the BSDF createBSDF returns
    int numNodes;
    uint32_t type;            // = nodes[0].type
};
inline uint32_t dtFlip(uint32_t t) { return t ^ DT_WholeSphere; }        // DDF.h:79

// The component's BSDF interface as MultiBSDF sees it (m_type, weight(), the three *Internal calls).
template <int N>
struct Component {
    const BSDF<N>& base;
    bool inverse;
    uint32_t type() const { return inverse ? dtFlip(base.type) : base.type; }                     // basic_BSDFs.h:71
    bool matches(uint32_t flags) const { return dtMatches(type(), flags); }
    float weight(const BSDFQuery<N>& q) const {                                                   // DDF.h:280-289
        if (!matches(q.flags)) return 0;
        if (!inverse) return bsdfWeight(base, q);       // matches() was checked with the same type
        BSDFQuery<N> mq = q;                            // InverseBSDF::weightInternal :199-203
        mq.flags = dtFlip(mq.flags);
        return bsdfWeight(base, mq);
    }
    Spec<N> sampleInternal(const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result) const {
        if (!inverse) return bsdfSampleInternal(base, q, uComponent, uDir, result);
        BSDFQuery<N> mq = q;                            // InverseBSDF::sampleInternal :172-181 (calls the public sample())
        mq.flags = dtFlip(mq.flags);
        Spec<N> ret = bsdfSample(base, mq, uComponent, uDir, result);
        result->dirType = dtFlip(result->dirType);
        result->dir_sn.z *= -1;
        return ret;
    }
    Spec<N> evaluateInternal(const BSDFQuery<N>& q, uint32_t flags, V3 dir) const {
        if (!inverse) return bsdfEvaluateInternal(base, q, flags, dir);
        BSDFQuery<N> mq = q;                            // InverseBSDF::evaluateInternal :183-189 (public evaluate())
        mq.flags = dtFlip(flags);
        V3 mDir = dir;
        mDir.z *= -1;
        return bsdfEvaluate(base, mq, mDir);
    }
    float evaluatePDFInternal(const BSDFQuery<N>& q, V3 dir) const {
        if (!inverse) return bsdfEvaluatePDFInternal(base, q, dir);
        V3 mDir = dir;                                  // InverseBSDF::evaluatePDFInternal :191-197: `mQuery.flags.flip();`
        mDir.z *= -1;                                   // discards its result, so the flags go through unflipped
        return bsdfEvaluatePDF(base, q, mDir);
    }
};

// Core/distributions.cpp:14-29 (compensated sums; for two items they equal the plain float sums)
inline uint32_t sampleDiscrete(const float* importances, float* sumImportances, float* base, uint32_t n, float u) {
    Kahan<float> sum;
    for (uint32_t i = 0; i < n; ++i) sum.add(importances[i]);
    *sumImportances = sum.result;
    float su = u * sum.result;
    Kahan<float> cum;
    for (uint32_t i = 0; i < n; ++i) {
        *base = cum.result;
        cum.add(importances[i]);
        if (su < cum.result) return i;
    }
    return 0;
}

// The virtual calls MultiBSDF makes on a component — BSDF::weight (DDF.h:280-289) and the three *Internal functions — for
// either kind of node.
template <int N> float nodeWeight(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q);
template <int N> Spec<N> nodeSampleInternal(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result);
template <int N> Spec<N> nodeEvaluateInternal(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q, uint32_t flags, V3 dir);
template <int N> float nodeEvaluatePDFInternal(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q, V3 dir);
template <int N> inline bool nodeMatches(const AnyBSDF<N>& f, int i, uint32_t flags) { return dtMatches(f.nodes[i].type, flags); }

// MultiBSDF::sampleInternalNoRev  MultiBSDF.cpp:20-59
template <int N>
Spec<N> multiSampleInternal(const AnyBSDF<N>& f, int node, const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result) {
    const int* c = f.nodes[node].child;
    float weights[2];
    for (int i = 0; i < 2; ++i) weights[i] = nodeWeight(f, c[i], q);
    float sumWeights, base;
    uint32_t idx = sampleDiscrete(weights, &sumWeights, &base, 2u, uComponent);
    if (sumWeights == 0.0f) { result->dirPDF = 0.0f; return Spec<N>(); }
    uComponent = (uComponent * sumWeights - base) / weights[idx];
    result->dirPDF = 0.0f;
    Spec<N> value = nodeSampleInternal(f, c[idx], q, uComponent, uDir, result);
    result->dirPDF *= weights[idx];
    if (result->dirPDF == 0.0f) return Spec<N>();
    if (!dtIsDelta(result->dirType)) {
        for (int i = 0; i < 2; ++i)
            if (i != (int)idx && nodeMatches(f, c[i], q.flags))
                result->dirPDF += nodeEvaluatePDFInternal(f, c[i], q, result->dir_sn) * weights[i];
        uint32_t mflags = q.flags & sideTest(q.gNormal_sn, q.dir_sn, result->dir_sn);
        value = Spec<N>();
        for (int i = 0; i < 2; ++i) {
            if (!nodeMatches(f, c[i], mflags)) continue;
            value = value + nodeEvaluateInternal(f, c[i], q, mflags, result->dir_sn);
        }
    }
    result->dirPDF /= sumWeights;
    return value;
}
// MultiBSDF::evaluateInternal :125-149, evaluatePDFInternalNoRev :151-169, weightInternal :207-212
template <int N>
Spec<N> multiEvaluateInternal(const AnyBSDF<N>& f, int node, const BSDFQuery<N>& q, uint32_t flags, V3 dir) {
    const int* c = f.nodes[node].child;
    Spec<N> ret;
    for (int i = 0; i < 2; ++i) {
        if (!nodeMatches(f, c[i], flags)) continue;
        ret = ret + nodeEvaluateInternal(f, c[i], q, flags, dir);
    }
    return ret;
}
template <int N>
float multiEvaluatePDFInternal(const AnyBSDF<N>& f, int node, const BSDFQuery<N>& q, V3 dir) {
    const int* c = f.nodes[node].child;
    Kahan<float> sumWeights;
    float weights[2];
    for (int i = 0; i < 2; ++i) { weights[i] = nodeWeight(f, c[i], q); sumWeights.add(weights[i]); }
    if (sumWeights.result == 0.0f) return 0.0f;
    float retPDF = 0.0f;
    for (int i = 0; i < 2; ++i)
        if (weights[i] > 0) retPDF += nodeEvaluatePDFInternal(f, c[i], q, dir) * weights[i];
    retPDF /= sumWeights.result;
    return retPDF;
}
template <int N>
float nodeWeight(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q) {
    const typename AnyBSDF<N>::Node& n = f.nodes[i];
    if (!n.multi) return Component<N>{n.lobe, n.inverse}.weight(q);
    if (!dtMatches(n.type, q.flags)) return 0;              // BSDF::weight
    Kahan<float> sumWeights;                                // MultiBSDF::weightInternal
    for (int k = 0; k < 2; ++k) sumWeights.add(nodeWeight(f, n.child[k], q));
    return sumWeights.result * 1.0f;                        // non-adjoint: snCorrection 1
}
template <int N>
Spec<N> nodeSampleInternal(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result) {
    const typename AnyBSDF<N>::Node& n = f.nodes[i];
    if (!n.multi) return Component<N>{n.lobe, n.inverse}.sampleInternal(q, uComponent, uDir, result);
    return multiSampleInternal(f, i, q, uComponent, uDir, result);
}
template <int N>
Spec<N> nodeEvaluateInternal(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q, uint32_t flags, V3 dir) {
    const typename AnyBSDF<N>::Node& n = f.nodes[i];
    if (!n.multi) return Component<N>{n.lobe, n.inverse}.evaluateInternal(q, flags, dir);
    return multiEvaluateInternal(f, i, q, flags, dir);
}
template <int N>
float nodeEvaluatePDFInternal(const AnyBSDF<N>& f, int i, const BSDFQuery<N>& q, V3 dir) {
    const typename AnyBSDF<N>::Node& n = f.nodes[i];
    if (!n.multi) return Component<N>{n.lobe, n.inverse}.evaluatePDFInternal(q, dir);
    return multiEvaluatePDFInternal(f, i, q, dir);
}

// The public BSDF interface (DDF.h:231-279) on either kind
template <int N>
Spec<N> bsdfSample(const AnyBSDF<N>& f, const BSDFQuery<N>& q, float uComponent, const float uDir[2], BSDFResult* result) {
    if (!f.nodes[0].multi) return bsdfSample(f.nodes[0].lobe, q, uComponent, uDir, result);
    if (!dtMatches(f.type, q.flags)) { result->dirPDF = 0.0f; result->dirType = 0; return Spec<N>(); }
    Spec<N> fs_sn = multiSampleInternal(f, 0, q, uComponent, uDir, result);
    if (result->dirPDF == 0.0f) return Spec<N>();
    float snCorrection = std::fabs(result->dir_sn.z / dot(result->dir_sn, q.gNormal_sn));
    return fs_sn * snCorrection;
}
template <int N>
Spec<N> bsdfEvaluate(const AnyBSDF<N>& f, const BSDFQuery<N>& q, V3 dir) {
    if (!f.nodes[0].multi) return bsdfEvaluate(f.nodes[0].lobe, q, dir);
    uint32_t flags = q.flags & sideTest(q.gNormal_sn, q.dir_sn, dir);
    if (!dtMatches(f.type, flags)) return Spec<N>();
    Spec<N> fs_sn = multiEvaluateInternal(f, 0, q, flags, dir);
    float snCorrection = std::fabs(dir.z / dot(dir, q.gNormal_sn));
    return fs_sn * snCorrection;
}
template <int N>
float bsdfEvaluatePDF(const AnyBSDF<N>& f, const BSDFQuery<N>& q, V3 dir) {
    if (!f.nodes[0].multi) return bsdfEvaluatePDF(f.nodes[0].lobe, q, dir);
    if (!dtMatches(f.type, q.flags)) return 0;
    return multiEvaluatePDFInternal(f, 0, q, dir);
}

// SurfacePoint::createBSDF (geometry.cpp:56-58) -> SurfaceMaterial::getBSDF
// (basic_SurfaceMaterials.cpp:15-43; EmitterSurfaceMaterial forwards to its base material,
//  surface_material.h:65).  `scale * spectrum` with scale = 1.0f is an exact multiply.
// A material's spectrum slot: a constant spectrum (ConstantSpectrumTexture) or, for SLRHIP_TEXTURE_REF values, a
// CheckerBoardSpectrumTexture evaluated at the hit's texture coordinate (checker_board_textures.h:21-24).
// ImageSpectrumTexture::evaluate (Textures/image_textures.cpp:13-79) behind an OffsetAndScale2DMapping (Core/textures.h:37-41):
// the nearest texel, wrapped by fmod; RGB build: its three floats (:36-63), spectral build: (u, v, s) through
// UpsampledContinuousSpectrum::evaluate (:23-32).  The texels are the caller's (image decoding is outside the boundary).
inline const float* imageTexel(const Scene& s, const slrhip_texture& t, float texU, float texV) {
    const float x = (texU + t.offset[0]) * t.scale[0], y = (texV + t.offset[1]) * t.scale[1];
    float u = std::fmod(x, 1.0f);
    float v = std::fmod(y, 1.0f);
    u += u < 0 ? 1.0f : 0.0f;
    v += v < 0 ? 1.0f : 0.0f;
    const uint32_t w = t.reserved[0], h = t.reserved[1];
    uint32_t px = std::min((uint32_t)(w * u), w - 1);
    uint32_t py = std::min((uint32_t)(h * v), h - 1);
    return &s.textureTexels[((size_t)t.reserved[2] + (size_t)py * w + px) * 3];
}
template <int N> Spec<N> imageTextureValue(const Scene& s, const float* x, const Wls<N>& wls);
template <> inline Spec<3> imageTextureValue<3>(const Scene&, const float* x, const Wls<3>&) { Spec<3> r; r.c[0] = x[0]; r.c[1] = x[1]; r.c[2] = x[2]; return r; }
template <> inline Spec<16> imageTextureValue<16>(const Scene& s, const float* x, const Wls<16>& wls) {
    const float kEqualEnergyReflectance = 0.009355121400914532f;        // Upsampling::EqualEnergyReflectance, Spectrum.h
    return evaluateUpsampled(s, x[0], x[1], x[2] / kEqualEnergyReflectance, wls);
}
template <int N>
inline Spec<N> evalSlot(const Scene& s, int32_t slot, float texU, float texV, const Wls<N>& wls) {
    if (slot >= -1) return EvalSpectrum<N>::eval(s, slot, wls);
    const slrhip_texture& t = s.textures[-2 - slot];
    if (t.kind == SLRHIP_TEXTURE_IMAGE_SPECTRUM) return imageTextureValue<N>(s, imageTexel(s, t, texU, texV), wls);
    return EvalSpectrum<N>::eval(s, t.spectrum[checkerIndex(t, texU, texV)], wls);
}

template <int N>
BSDF<N> createLobe(const Scene& s, const slrhip_material& m, const Wls<N>& wls, float scale, float texU = 0.0f, float texV = 0.0f) {
    const uint16_t wlFlags = wls.flags;
    BSDF<N> f;
    f.kind = m.type;
    f.param = m.param;
    f.param2 = m.param2;
    f.onA = f.onB = 0.0f;
    switch (m.type) {
    case SLRHIP_MATERIAL_WARD:
        f.type = DT_Reflection | DT_HighFreq;                                  // ModifiedWardDurBRDF.h:29
        f.a = scale * evalSlot<N>(s, m.spectrum[0], texU, texV, wls);
        break;
    case SLRHIP_MATERIAL_ASHIKHMIN:
        f.type = DT_Reflection | DT_HighFreq | DT_LowFreq;                     // AshikhminShirleyBRDF.h:29
        f.a = scale * evalSlot<N>(s, m.spectrum[0], texU, texV, wls);             // scale * Rs
        f.b = scale * evalSlot<N>(s, m.spectrum[1], texU, texV, wls);             // scale * Rd
        break;
    case SLRHIP_MATERIAL_MATTE:
        f.type = DT_Reflection | DT_LowFreq;                                   // basic_BSDFs.h:27, OrenNayerBRDF.h:29
        f.a = scale * evalSlot<N>(s, m.spectrum[0], texU, texV, wls);
        if (m.param >= 0.0f) {                                                 // OrenNayerBRDF.h:28-30 (double literals)
            float sigma = m.param;
            f.onA = (float)(1.0f - 0.5f * sigma * sigma / (sigma * sigma + 0.33));
            f.onB = (float)(0.45 * sigma * sigma / (sigma * sigma + 0.09));
        }
        break;
    case SLRHIP_MATERIAL_MICROFACET_METAL:
        f.type = DT_Reflection | DT_HighFreq;                                  // MicrofacetBSDF.h:27-28
        f.b = evalSlot<N>(s, m.spectrum[1], texU, texV, wls);
        f.c = evalSlot<N>(s, m.spectrum[2], texU, texV, wls);
        break;
    case SLRHIP_MATERIAL_MICROFACET_GLASS:
        f.type = DT_Reflection | DT_Transmission | DT_HighFreq;                // MicrofacetBSDF.h:44-46
        f.b = evalSlot<N>(s, m.spectrum[1], texU, texV, wls);
        f.c = evalSlot<N>(s, m.spectrum[2], texU, texV, wls);
        break;
    case SLRHIP_MATERIAL_METAL:
        f.type = DT_Reflection | DT_Delta0D;                                   // basic_BSDFs.h:43
        f.a = scale * evalSlot<N>(s, m.spectrum[0], texU, texV, wls);
        f.b = evalSlot<N>(s, m.spectrum[1], texU, texV, wls);
        f.c = evalSlot<N>(s, m.spectrum[2], texU, texV, wls);
        break;
    case SLRHIP_MATERIAL_GLASS:
        // dispersive = !wls.lambdaSelected()  basic_SurfaceMaterials.cpp:42, basic_BSDFs.h:59-61
        f.type = DT_Reflection | DT_Transmission | DT_Delta0D | ((wlFlags & 1) ? 0u : (uint32_t)DT_Dispersive);
        f.a = scale * evalSlot<N>(s, m.spectrum[0], texU, texV, wls);
        f.b = evalSlot<N>(s, m.spectrum[1], texU, texV, wls);
        f.c = evalSlot<N>(s, m.spectrum[2], texU, texV, wls);
        break;
    default:
        f.type = 0;
        break;
    }
    return f;
}

// SummedSurfaceMaterial.cpp:13-20 / MixedSurfaceMaterial.cpp:14-22 / InverseSurfaceMaterial basic_SurfaceMaterials.cpp:47-50:
// getBSDF(surfPt, wls, mem, scale) recursively; a "mix" hands scale * (1 - factor) and scale * factor down, a "sum" scale itself.
template <int N>
int buildBSDFNode(AnyBSDF<N>& f, const Scene& s, const slrhip_material& m, const Wls<N>& wls, float scale, float texU, float texV) {
    const int idx = f.numNodes++;
    typename AnyBSDF<N>::Node& n = f.nodes[idx];
    n.inverse = false;
    n.child[0] = n.child[1] = -1;
    if (m.type != SLRHIP_MATERIAL_MULTI) {
        n.multi = false;
        n.lobe = createLobe<N>(s, m, wls, scale, texU, texV);
        n.type = n.lobe.type;
        return idx;
    }
    n.multi = true;
    const float scales[2] = {scale * m.param, scale * m.param2};
    uint32_t type = 0;
    for (int i = 0; i < 2; ++i) {
        const int c = buildBSDFNode<N>(f, s, s.materials[m.spectrum[i]], wls, scales[i], texU, texV);
        f.nodes[idx].child[i] = c;
        if ((m.spectrum[2] >> i) & 1) {                    // InverseSurfaceMaterial over a single lobe (validated at scene creation)
            f.nodes[c].inverse = true;
            f.nodes[c].type = dtFlip(f.nodes[c].type);     // InverseBSDF ctor, basic_BSDFs.h:71
        }
        type |= f.nodes[c].type;                           // MultiBSDF::add :16
    }
    f.nodes[idx].type = type;
    return idx;
}
template <int N>
AnyBSDF<N> createBSDFOf(const Scene& s, const slrhip_material& m, const Wls<N>& wls, float texU = 0.0f, float texV = 0.0f) {
    AnyBSDF<N> f;
    f.numNodes = 0;
    buildBSDFNode<N>(f, s, m, wls, 1.0f, texU, texV);
    f.type = f.nodes[0].type;
    return f;
}
template <int N>
inline AnyBSDF<N> createBSDF(const Scene& s, const SurfPt& sp, const Wls<N>& wls) { return createBSDFOf<N>(s, s.materials[s.tris[sp.tri].material], wls, sp.texU, sp.texV); }

inline bool isEmitting(const Scene& s, uint32_t tri) { return tri == kEnvObject || s.materials[s.tris[tri].material].emittance >= 0; }
template <int N>
inline Spec<N> emittance(const Scene& s, uint32_t tri, const Wls<N>& wls) { return EvalSpectrum<N>::eval(s, s.materials[s.tris[tri].material].emittance, wls); }
// SurfacePoint::emittance x EDF::evaluate for either kind of emitter: DiffuseEDF (basic_EDFs.cpp:19-23) for triangles,
// IBLEDF::evaluate (EDFs/IBLEDF.cpp:19-23: 1 / pi in every direction) for the environment sphere.
template <int N>
inline Spec<N> emittedRadiance(const Scene& s, const SurfPt& sp, const Wls<N>& wls, V3 dirLocal) {
    if (sp.tri == kEnvObject) return envEmittanceT<N>(s, sp.texU, sp.texV, wls) * Spec<N>((float)(1.0f / M_PI));
    return emittance(s, sp.tri, wls) * Spec<N>(dirLocal.z > 0.0f ? (float)(1.0f / M_PI) : 0.0f);
}
// EDFs/basic_EDFs.cpp:19-23  DiffuseEDF::evaluate: `dir.z > 0 ? 1.0f / M_PI : 0.0f` (double) -> SampledSpectrum(float)
template <int N>
inline Spec<N> diffuseEDFEvaluate(V3 dir) { return Spec<N>(dir.z > 0.0f ? (float)(1.0f / M_PI) : 0.0f); }

// ------------------------------------------------------------------------------------------
// Cameras/PerspectiveCamera.cpp
// ------------------------------------------------------------------------------------------
void setupCamera(Camera& c, const slrhip_camera& in) {
    std::memcpy(c.mat, in.local_to_world, sizeof(c.mat));
    std::memcpy(c.matInv, in.world_to_local, sizeof(c.matInv));
    c.aspect = in.aspect; c.fovY = in.fov_y; c.lensRadius = in.lens_radius;
    c.imgPlaneDistance = in.img_plane_distance; c.objPlaneDistance = in.obj_plane_distance;
    // :15-24
    c.opHeight = 2.0f * c.objPlaneDistance * std::tan(c.fovY * 0.5f);
    c.opWidth = c.opHeight * c.aspect;
    c.imgPlaneArea = (float)((double)(c.opWidth * c.opHeight) * std::pow((double)(c.imgPlaneDistance / c.objPlaneDistance), 2.0));
    c.sensitivity = in.sensitivity > 0 ? in.sensitivity : (float)(1.0f / (M_PI * (double)c.lensRadius * (double)c.lensRadius));
}

// Matrix4x4.h:75-81  mat * Point3 (column-major m[c*4+r])
// ------------------------------------------------------------------------------------------
// Scene light selection (Core/SurfaceObject.cpp:279-299, 432-466)
// ------------------------------------------------------------------------------------------
inline uint32_t aggregateSelectLight(const Scene& s, float u, float* prob) {   // SurfaceObject.cpp:279-286
    uint32_t lIdx = s.lightDist.sample(u, prob);      // remapped u is unused by SingleSurfaceObject::selectLight
    *prob *= 1.0f;                                    // cProb = 1 (SurfaceObject.cpp:73-76)
    return s.lightTris[lIdx];
}
// Scene::selectLight, SurfaceObject.cpp:432-450.  Returns a triangle index or kEnvObject.
inline uint32_t selectLight(const Scene& s, float u, float* prob) {
    if (s.hasEnv) {
        const float aggImp = s.lightDist.integral, envImp = 1.0f;      // importance(): :275-277, :154-156
        float sumImps = aggImp + envImp;
        float su = sumImps * u;
        if (su < aggImp) {
            u = u / (aggImp / sumImps);
            uint32_t t = aggregateSelectLight(s, u, prob);
            *prob *= aggImp / sumImps;
            return t;
        }
        else {
            // u = (u - aggImp) / (envImp / sumImps): the reference's (un-normalised) remap is unused by the sphere
            *prob = 1.0f;                              // SingleSurfaceObject::selectLight :73-76
            *prob *= envImp / sumImps;
            return kEnvObject;
        }
    }
    return aggregateSelectLight(s, u, prob);
}
// Scene::evaluateProb, SurfaceObject.cpp:452-466
inline float evaluateLightProb(const Scene& s, uint32_t tri) {
    if (s.hasEnv) {
        const float aggImp = s.lightDist.integral, envImp = 1.0f;
        float sumImps = aggImp + envImp;
        if (tri == kEnvObject) return envImp / sumImps;
        int32_t li = s.tris[tri].lightIndex;
        float aggProb = li < 0 ? 0.0f : s.lightDist.PMF[li] * 1.0f;
        return aggImp / sumImps * aggProb;
    }
    int32_t li = s.tris[tri].lightIndex;
    if (li < 0) return 0.0f;
    return s.lightDist.PMF[li] * 1.0f;
}

// InfiniteSphereSurfaceObject::sample, SurfaceObject.cpp:158-185 (returns the emittance M)
template <int N>
Spec<N> envSample(const Scene& s, const Wls<N>& wls, float u0, float u1, SurfPt* sp, float* areaPDF) {
    float uvPDF, theta, phi;
    s.envDist.sample(u0, u1, &phi, &theta, &uvPDF);
    phi = (float)(phi * (2 * M_PI));
    theta = (float)(theta * M_PI);
    sp->p = V3(-std::sin(phi) * std::sin(theta), std::cos(theta), std::cos(phi) * std::sin(theta));
    sp->atInfinity = true;
    sp->gNormal = -sp->p;
    sp->u = phi;
    sp->v = theta;
    sp->texU = (float)(phi / (2 * M_PI));
    sp->texV = (float)(theta / M_PI);
    V3 tc0 = normalize(V3(-std::cos(phi), 0.0f, -std::sin(phi)));
    sp->frame.x = tc0;
    sp->frame.z = sp->gNormal;
    sp->frame.y = cross(sp->frame.z, sp->frame.x);
    sp->tri = kEnvObject;
    *areaPDF = (float)(uvPDF / (2 * M_PI * M_PI * std::sin(theta)));
    return envEmittanceT<N>(s, sp->texU, sp->texV, wls);
}
// InfiniteSphereSurfaceObject::evaluateAreaPDF, SurfaceObject.cpp:217-222
inline float envEvaluateAreaPDF(const Scene& s, const SurfPt& sp) {
    float phi = sp.u, theta = sp.v;
    float uvPDF = s.envDist.evaluatePDF((float)(phi / (2 * M_PI)), (float)(theta / M_PI));
    return (float)(uvPDF / (2 * M_PI * M_PI * std::sin(theta)));
}

// ------------------------------------------------------------------------------------------
// Renderers/PathTracingRenderer.cpp:137-262  Job::contribution
// ------------------------------------------------------------------------------------------
template <int N>
Spec<N> contribution(const Scene& scene, const Wls<N>& initWLs, const Ray& initRay, XorShift& rng, slr_oracle_counters* ctr) {
    Wls<N> wls = initWLs;
    const uint16_t selectedLambda = wls.selectedLambda;
    Ray ray = initRay;
    SurfPt surfPt;
    Spec<N> alpha(1.0f);
    float initY = importance(alpha, selectedLambda);
    Kahan<Spec<N>> sp;
    uint32_t pathLength = 0;

    Isect isect;
    if (!sceneIntersect(scene, ray, &isect, ctr)) return Spec<N>();
    getSurfacePoint(scene, isect, &surfPt);

    V3 dirOut_sn = surfPt.frame.toLocal(-ray.dir);
    if (isEmitting(scene, surfPt.tri)) {
        Spec<N> Le = emittedRadiance(scene, surfPt, wls, dirOut_sn);
        sp.add(alpha * Le);
    }
    if (surfPt.atInfinity) return sp.result;

    while (true) {
        ++pathLength;
        if (pathLength >= 100) break;
        if (ctr) ++ctr->loop_iterations;
        V3 gNorm_sn = surfPt.frame.toLocal(surfPt.gNormal);
        AnyBSDF<N> bsdf = createBSDF(scene, surfPt, wls);
        BSDFQuery<N> fsQuery;
        fsQuery.dir_sn = dirOut_sn; fsQuery.gNormal_sn = gNorm_sn; fsQuery.wlHint = (int16_t)selectedLambda; fsQuery.flags = DT_All;

        // Next Event Estimation  :169-204
        if (dtMatches(bsdf.type, DT_WholeSphere | DT_NonDelta)) {
            float lightProb;
            uint32_t lightTri = selectLight(scene, rng.getFloat0cTo1o(), &lightProb);
            float lu0 = rng.getFloat0cTo1o();
            float lu1 = rng.getFloat0cTo1o();
            SurfPt lp; float areaPDF;
            Spec<N> M;
            if (lightTri == kEnvObject) M = envSample<N>(scene, wls, lu0, lu1, &lp, &areaPDF);
            else {
                triSample(scene, lightTri, lu0, lu1, &lp, &areaPDF);
                M = emittance(scene, lightTri, wls);                       // SingleSurfaceObject::sample :82-91
            }

            if (testVisibility(scene, surfPt, lp, ctr)) {
                // SurfacePoint::getDirectionFrom geometry.cpp:32-43
                float dist2;
                V3 shadowDir;
                if (lp.atInfinity) { dist2 = 1.0f; shadowDir = normalize(lp.p); }
                else {
                    V3 d = lp.p - surfPt.p;
                    dist2 = sqLength(d);
                    shadowDir = d / std::sqrt(dist2);
                }
                V3 shadowDir_l = lp.frame.toLocal(-shadowDir);
                V3 shadowDir_sn = surfPt.frame.toLocal(shadowDir);

                Spec<N> Le = lp.atInfinity ? M * Spec<N>((float)(1.0f / M_PI)) : M * diffuseEDFEvaluate<N>(shadowDir_l);
                float lightPDF = lightProb * areaPDF;

                Spec<N> fs = bsdfEvaluate(bsdf, fsQuery, shadowDir_sn);
                float cosLight = absDot(-shadowDir, lp.gNormal);
                float bsdfPDF = bsdfEvaluatePDF(bsdf, fsQuery, shadowDir_sn) * cosLight / dist2;

                float MISWeight = 1.0f;
                if (!std::isinf(areaPDF))    // posType = LowFreq is never delta (SurfaceObject.cpp:88)
                    MISWeight = (lightPDF * lightPDF) / (lightPDF * lightPDF + bsdfPDF * bsdfPDF);

                float G = absDot(shadowDir_sn, gNorm_sn) * cosLight / dist2;
                sp.add(alpha * Le * fs * (G * MISWeight / lightPDF));
            }
        }

        // BSDF sampling :206-221
        BSDFResult fsResult;
        float uComp = rng.getFloat0cTo1o();
        float uDir[2];
        uDir[0] = rng.getFloat0cTo1o();
        uDir[1] = rng.getFloat0cTo1o();
        Spec<N> fs = bsdfSample(bsdf, fsQuery, uComp, uDir, &fsResult);
        if (fs.isZero() || fsResult.dirPDF == 0.0f) break;
        if (dtIsDispersive(fsResult.dirType)) {
            fsResult.dirPDF /= N;                   // WavelengthSamples::NumComponents (RGBTypes.h:47-48 / SpectrumTypes.h:66-67)
            wls.flags |= 1;                         // LambdaIsSelected
        }
        alpha = alpha * (fs * absDot(fsResult.dir_sn, gNorm_sn) / fsResult.dirPDF);

        V3 dirIn = surfPt.frame.fromLocal(fsResult.dir_sn);
        ray.org = surfPt.p; ray.dir = dirIn; ray.distMin = 0.0001f; ray.distMax = INFINITY;

        isect = Isect();
        if (!sceneIntersect(scene, ray, &isect, ctr)) break;
        getSurfacePoint(scene, isect, &surfPt);

        dirOut_sn = surfPt.frame.toLocal(-ray.dir);

        // implicit light sampling :232-249
        if (isEmitting(scene, surfPt.tri)) {
            float bsdfPDF = fsResult.dirPDF;
            Spec<N> Le = emittedRadiance(scene, surfPt, wls, dirOut_sn);
            float lightProb = evaluateLightProb(scene, surfPt.tri);
            float dist2 = surfPt.atInfinity ? 1.0f : sqLength(ray.org - surfPt.p);   // getSquaredDistance geometry.h:249
            float areaPDFhit = surfPt.atInfinity ? envEvaluateAreaPDF(scene, surfPt) : (1.0f / triArea(scene, surfPt.tri));
            float lightPDF = lightProb * areaPDFhit * dist2 / absDot(ray.dir, surfPt.gNormal);
            float MISWeight = 1.0f;
            if (!dtIsDelta(fsResult.dirType))
                MISWeight = (bsdfPDF * bsdfPDF) / (lightPDF * lightPDF + bsdfPDF * bsdfPDF);
            sp.add(alpha * Le * MISWeight);
        }
        if (surfPt.atInfinity) break;

        // Russian roulette :254-258
        float continueProb = std::min(importance(alpha, selectedLambda) / initY, 1.0f);
        if (rng.getFloat0cTo1o() < continueProb) alpha = alpha / continueProb;
        else break;
    }
    return sp.result;
}

// ------------------------------------------------------------------------------------------
// Renderers/PathTracingRenderer.cpp:100-135  Job::kernel body for ONE pixel sample.
// Draw order is left to right (the pinned clang build).
// ------------------------------------------------------------------------------------------
template <int N>
void pixelSample(const Scene& scene, const slrhip_render_settings& st, uint32_t basePixelX, uint32_t basePixelY, XorShift& rng,
                 slr_oracle_counters* ctr, float* px, float* py, Spec<N>* out, Wls<N>* outWls) {
    const Camera& cam = scene.camera;
    float v = rng.getFloat0cTo1o();
    float time = st.time_start * (1 - v) + st.time_end * v;                 // light_path_samplers.h:50
    (void)time;
    float pxx = basePixelX + rng.getFloat0cTo1o();                          // :51 (uint32 + float)
    float pyy = basePixelY + rng.getFloat0cTo1o();

    // createWithEqualOffsets: RGBTypes.h:37-45 (offset unused, PDF 1) / SpectrumTypes.h:54-64
    float wlOffset = rng.getFloat0cTo1o();
    float uLambda = rng.getFloat0cTo1o();
    Wls<N> wls;
    float selectWLPDF;
    for (int i = 0; i < N; ++i)
        wls.lambdas[i] = kWavelengthLowBound + (kWavelengthHighBound - kWavelengthLowBound) * (i + wlOffset) / N;
    wls.selectedLambda = std::min(uint16_t(N * uLambda), uint16_t(N - 1));
    wls.flags = 0;
    selectWLPDF = N == 3 ? 1.0f : N / (kWavelengthHighBound - kWavelengthLowBound);

    // camera->sample PerspectiveCamera.cpp:33-57
    float lu0 = rng.getFloat0cTo1o();
    float lu1 = rng.getFloat0cTo1o();
    float lx, ly;
    concentricSampleDisk(lu0, lu1, &lx, &ly);
    V3 orgLocal(cam.lensRadius * lx, cam.lensRadius * ly, 0.0f);
    V3 lensP = mulPoint(cam.mat, orgLocal);
    V3 lensN = mulNormal(cam.matInv, V3(0, 0, 1));
    Frame lensFrame;
    lensFrame.z = lensN;
    lensFrame.x = mulVector(cam.mat, V3(1, 0, 0));
    lensFrame.y = cross(lensFrame.z, lensFrame.x);
    float areaPDF = cam.lensRadius > 0.0f ? (float)(1.0f / (M_PI * (double)cam.lensRadius * (double)cam.lensRadius)) : 1.0f;

    // createIDF :59-61, PerspectiveIDF::sample :63-74 with IDFSample(p.x / W, p.y / H) (PathTracingRenderer.cpp:115)
    float sx = pxx / (float)(uint32_t)st.image_width;
    float sy = pyy / (float)(uint32_t)st.image_height;
    V3 idfOrg(cam.lensRadius * lx, cam.lensRadius * ly, 0.0f);
    V3 pFocus(cam.opWidth * (0.5f - sx), cam.opHeight * (0.5f - sy), cam.objPlaneDistance);
    V3 dirLocal = normalize(pFocus - idfOrg);
    float dirPDF = cam.imgPlaneDistance * cam.imgPlaneDistance / ((dirLocal.z * dirLocal.z * dirLocal.z) * cam.imgPlaneArea);

    Ray ray;
    ray.org = lensP;
    ray.dir = lensFrame.fromLocal(dirLocal);
    ray.distMin = 0.0f;
    ray.distMax = INFINITY;
    Spec<N> C = contribution<N>(scene, wls, ray, rng, ctr);

    // :126  weight = (We0 * We1) * (absDot(ray.dir, gNormal) / (areaPDF * dirPDF * selectWLPDF))
    Spec<N> weight = (Spec<N>(1.0f) * Spec<N>(1.0f)) * (absDot(ray.dir, lensN) / (areaPDF * dirPDF * selectWLPDF));
    *out = weight * C;
    *outWls = wls;
    *px = pxx;
    *py = pyy;
}

// SpectrumStorage::add.  RGB: value += val (RGBTypes.h:176-179).  Spectral: each sample goes to the storage bin of
// its wavelength, scaled by the reciprocal bin width, and the 16-bin addend is Kahan-added (SpectrumTypes.h:818-836).
inline void storageAdd(Kahan<Spec<3>>& px, const Wls<3>&, const Spec<3>& val) { px.add(val); }
inline void storageAdd(Kahan<Spec<16>>& px, const Wls<16>& wls, const Spec<16>& val) {
    const uint32_t numStrata = 16;
    const float recBinWidth = numStrata / (kWavelengthHighBound - kWavelengthLowBound);
    Spec<16> addend(0.0f);
    for (int i = 0; i < 16; ++i) {
        uint32_t sBin = std::min(uint32_t((wls.lambdas[i] - kWavelengthLowBound) / (kWavelengthHighBound - kWavelengthLowBound) * numStrata), numStrata - 1);
        addend[sBin] += val[i] * recBinWidth;
    }
    px.add(addend);
}

int32_t sampleSeed(int32_t rngSeed, uint32_t px, uint32_t py, uint32_t pass) {
    auto fmix = [](uint32_t h) { h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16; return h; };
    uint32_t h = (uint32_t)rngSeed;
    h = fmix(h ^ (pass * 0x9E3779B1u));
    h = fmix(h ^ (py * 0x85EBCA77u + 0x165667B1u));
    h = fmix(h ^ (px * 0xC2B2AE3Du + 0x27D4EB2Fu));
    return (int32_t)h;
}

void addCounters(slr_oracle_counters* dst, const slr_oracle_counters& src) {
    dst->samples += src.samples; dst->extension_rays += src.extension_rays; dst->shadow_rays += src.shadow_rays;
    dst->loop_iterations += src.loop_iterations; dst->rng_draws += src.rng_draws;
    dst->nodes_visited += src.nodes_visited; dst->tris_tested += src.tris_tested;
}

} // namespace

namespace {
// Function-level known answers: Scene::selectLight + Light::sample as the integrator calls them (PathTracingRenderer.cpp:169-177).
template <int N>
int lightKatT(const slr_oracle_scene* s, uint32_t n, const float* in, float wlOffset, float uLambda, float* out) {
    Wls<N> wls;
    for (int i = 0; i < N; ++i)
        wls.lambdas[i] = kWavelengthLowBound + (kWavelengthHighBound - kWavelengthLowBound) * (i + wlOffset) / N;
    wls.selectedLambda = std::min(uint16_t(N * uLambda), uint16_t(N - 1));
    wls.flags = 0;
    const int stride = 16 + N;
    for (uint32_t i = 0; i < n; ++i) {
        const float* q = in + 3 * (size_t)i;
        float* o = out + stride * (size_t)i;
        float lightProb;
        uint32_t lightTri = selectLight(*s, q[0], &lightProb);
        SurfPt lp; float areaPDF;
        Spec<N> M;
        if (lightTri == kEnvObject) M = envSample<N>(*s, wls, q[1], q[2], &lp, &areaPDF);
        else {
            triSample(*s, lightTri, q[1], q[2], &lp, &areaPDF);
            M = emittance(*s, lightTri, wls);
        }
        o[0] = lightTri == kEnvObject ? -1.0f : (float)lightTri;
        o[1] = lightProb;
        o[2] = lp.p.x; o[3] = lp.p.y; o[4] = lp.p.z;
        o[5] = lp.gNormal.x; o[6] = lp.gNormal.y; o[7] = lp.gNormal.z;
        o[8] = lp.frame.x.x; o[9] = lp.frame.x.y; o[10] = lp.frame.x.z;
        o[11] = lp.frame.z.x; o[12] = lp.frame.z.y; o[13] = lp.frame.z.z;
        o[14] = areaPDF;
        o[15] = lp.atInfinity ? 1.0f : 0.0f;
        for (int k = 0; k < N; ++k) o[16 + k] = M[k];
    }
    return 0;
}

// Function-level known answers: the three public BSDF calls of DDF.h:231-279 on one material.
template <int N>
int bsdfKatT(const slr_oracle_scene* s, uint32_t material, uint32_t n, const float* in, float wlOffset, float uLambda, float* out) {
    Wls<N> wls;
    for (int i = 0; i < N; ++i)
        wls.lambdas[i] = kWavelengthLowBound + (kWavelengthHighBound - kWavelengthLowBound) * (i + wlOffset) / N;
    wls.selectedLambda = std::min(uint16_t(N * uLambda), uint16_t(N - 1));
    wls.flags = 0;
    AnyBSDF<N> bsdf = createBSDFOf<N>(*s, s->materials[material], wls);
    const int stride = 6 + 2 * N;
    for (uint32_t i = 0; i < n; ++i) {
        const float* q = in + 12 * (size_t)i;
        float* o = out + stride * (size_t)i;
        BSDFQuery<N> query;
        query.dir_sn = V3(q[0], q[1], q[2]); query.gNormal_sn = V3(q[3], q[4], q[5]);
        query.wlHint = (int16_t)wls.selectedLambda; query.flags = DT_All;
        V3 dirIn(q[6], q[7], q[8]);
        float uDir[2] = {q[10], q[11]};
        BSDFResult r; r.dir_sn = V3(0, 0, 0); r.dirPDF = 0.0f; r.dirType = 0;
        Spec<N> fs = bsdfSample(bsdf, query, q[9], uDir, &r);
        for (int k = 0; k < stride; ++k) o[k] = 0.0f;
        if (r.dirPDF != 0.0f) {
            o[0] = r.dir_sn.x; o[1] = r.dir_sn.y; o[2] = r.dir_sn.z; o[3] = r.dirPDF; o[4] = (float)r.dirType;
            for (int k = 0; k < N; ++k) o[5 + k] = fs[k];
        }
        Spec<N> fe = bsdfEvaluate(bsdf, query, dirIn);
        for (int k = 0; k < N; ++k) o[5 + N + k] = fe[k];
        o[5 + 2 * N] = bsdfEvaluatePDF(bsdf, query, dirIn);
    }
    return 0;
}
} // namespace

extern "C" {

slr_oracle_scene* slr_oracle_create(const slrhip_scene_desc* d, int mode) {
    if (!d || !d->vertices || !d->triangles || !d->materials || d->num_triangles == 0) return nullptr;
    if (mode != SLRHIP_MODE_RGB && mode != SLRHIP_MODE_SPECTRAL) return nullptr;
    if (mode == SLRHIP_MODE_SPECTRAL && !d->spectrum_data) return nullptr;
    Scene* s = new Scene();
    s->mode = mode;
    s->vertices.assign(d->vertices, d->vertices + d->num_vertices);
    s->materials.assign(d->materials, d->materials + d->num_materials);
    if (d->spectra) s->spectra.assign(d->spectra, d->spectra + d->num_spectra);
    if (d->spectrum_data) s->spectrumData.assign(d->spectrum_data, d->spectrum_data + d->num_spectrum_data);
    if (d->textures) s->textures.assign(d->textures, d->textures + d->num_textures);
    bool anyImageTexture = false;
    for (const slrhip_texture& t : s->textures) {              // every index a texture names must exist
        bool ok = t.kind <= SLRHIP_TEXTURE_IMAGE_SPECTRUM;
        if (ok && t.kind == SLRHIP_TEXTURE_CHECKER_SPECTRUM)
            ok = t.spectrum[0] >= 0 && t.spectrum[1] >= 0 && (uint32_t)t.spectrum[0] < d->num_spectra && (uint32_t)t.spectrum[1] < d->num_spectra;
        if (ok && t.kind == SLRHIP_TEXTURE_IMAGE_SPECTRUM) {
            ok = t.reserved[0] > 0 && t.reserved[1] > 0 && d->texture_texels &&
                 (uint64_t)t.reserved[2] + (uint64_t)t.reserved[0] * t.reserved[1] <= d->num_texture_texels && (mode != SLRHIP_MODE_SPECTRAL || d->upsampling);
            anyImageTexture = true;
        }
        if (!ok) { delete s; return nullptr; }
    }
    if (anyImageTexture) s->textureTexels.assign(d->texture_texels, d->texture_texels + (size_t)d->num_texture_texels * 3);
    if (mode == SLRHIP_MODE_SPECTRAL && d->upsampling && (anyImageTexture || d->env)) {
        const slrhip_upsampling_tables* t = d->upsampling;
        if (!t->cells || !t->point_uv || !t->point_spectrum) { delete s; return nullptr; }
        s->gridWidth = t->grid_width; s->gridHeight = t->grid_height;
        s->gridCells.assign(t->cells, t->cells + (size_t)t->grid_width * t->grid_height * 8);
        s->pointUV.assign(t->point_uv, t->point_uv + (size_t)t->num_points * 2);
        s->pointSpectrum.assign(t->point_spectrum, t->point_spectrum + (size_t)t->num_points * 95);
    }
    for (uint32_t i = 0; i < d->num_materials; ++i) {          // texture references of single-lobe materials
        const slrhip_material& m = s->materials[i];
        bool ok = (m.reserved & 0xFFFFu) <= s->textures.size() && (m.reserved >> 16) <= s->textures.size();
        if (ok && (m.reserved & 0xFFFFu)) ok = s->textures[(m.reserved & 0xFFFFu) - 1].kind == SLRHIP_TEXTURE_CHECKER_NORMAL;
        if (ok && (m.reserved >> 16)) ok = s->textures[(m.reserved >> 16) - 1].kind == SLRHIP_TEXTURE_CHECKER_FLOAT;
        for (int k = 0; k < 3 && ok && m.type != SLRHIP_MATERIAL_MULTI; ++k)
            if (m.spectrum[k] < -1)
                ok = (uint32_t)(-2 - m.spectrum[k]) < s->textures.size() && (s->textures[-2 - m.spectrum[k]].kind == SLRHIP_TEXTURE_CHECKER_SPECTRUM ||
                                                                                 s->textures[-2 - m.spectrum[k]].kind == SLRHIP_TEXTURE_IMAGE_SPECTRUM);
        if (!ok) { delete s; return nullptr; }
    }
    for (uint32_t i = 0; i < d->num_materials; ++i) {          // the restrictions include/slrhip.h states for MULTI
        const slrhip_material& m = s->materials[i];
        if (m.type != SLRHIP_MATERIAL_MULTI) continue;
        bool ok = (uint32_t)m.spectrum[2] <= 3u;
        for (int k = 0; k < 2 && ok; ++k) {
            ok = m.spectrum[k] >= 0 && (uint32_t)m.spectrum[k] < i;
            if (!ok) break;
            const slrhip_material& c = s->materials[m.spectrum[k]];
            if (c.type == SLRHIP_MATERIAL_MULTI) {
                // one level of nesting: the components of a component are single lobes (<= 4 lobes in all), and it is not inverted
                ok = !((m.spectrum[2] >> k) & 1) && s->materials[c.spectrum[0]].type < SLRHIP_MATERIAL_MULTI &&
                     s->materials[c.spectrum[1]].type < SLRHIP_MATERIAL_MULTI;
            }
            else if ((m.spectrum[2] >> k) & 1) ok = c.type != SLRHIP_MATERIAL_GLASS && c.type != SLRHIP_MATERIAL_MICROFACET_GLASS;
        }
        if (!ok) { delete s; return nullptr; }
    }
    s->tris.resize(d->num_triangles);
    // instances (slrhip_instance): ranges inside the triangle array, pairwise equal or disjoint; an instanced triangle is not an
    // object of the top-level aggregate, so it is not in its light list either — and must not emit (include/slrhip.h)
    std::vector<char> instanced(d->num_triangles, 0);
    if (d->instances && d->num_instances) {
        s->instances.assign(d->instances, d->instances + d->num_instances);
        for (size_t a = 0; a < s->instances.size(); ++a) {
            const slrhip_instance& ia = s->instances[a];
            bool ok = ia.num_triangles > 0 && (uint64_t)ia.first_triangle + ia.num_triangles <= d->num_triangles;
            for (size_t b = 0; b < a && ok; ++b) {
                const slrhip_instance& ib = s->instances[b];
                const bool same = ia.first_triangle == ib.first_triangle && ia.num_triangles == ib.num_triangles;
                const bool disjoint = ia.first_triangle + ia.num_triangles <= ib.first_triangle || ib.first_triangle + ib.num_triangles <= ia.first_triangle;
                ok = same || disjoint;
            }
            for (uint32_t t = 0; t < ia.num_triangles && ok; ++t) {
                instanced[ia.first_triangle + t] = 1;
                ok = s->materials[d->triangles[ia.first_triangle + t].material].emittance < 0;
            }
            if (!ok) { delete s; return nullptr; }
        }
    }
    std::vector<float> importances;
    for (uint32_t i = 0; i < d->num_triangles; ++i) {
        Tri& t = s->tris[i];
        for (int k = 0; k < 3; ++k) t.v[k] = d->triangles[i].v[k];
        t.material = d->triangles[i].material;
        t.lightIndex = -1;
        if (!instanced[i] && s->materials[t.material].emittance >= 0) {     // SurfaceObject.cpp:232-249
            t.lightIndex = (int32_t)s->lightTris.size();
            s->lightTris.push_back(i);
            importances.push_back(1.0f);                   // SingleSurfaceObject::importance :69-71
        }
    }
    s->lightDist.build(importances);
    s->hasEnv = d->env != nullptr;
    if (d->env) {
        const slrhip_envmap& e = *d->env;
        if (!e.texels || !e.importance || e.width == 0 || e.height == 0 || e.map_width == 0 || e.map_height == 0) {
            delete s;
            return nullptr;
        }
        s->envWidth = e.width; s->envHeight = e.height; s->envScale = e.scale;
        s->envTexels.assign(e.texels, e.texels + (size_t)e.width * e.height * 3);
        if (mode == SLRHIP_MODE_SPECTRAL && !d->upsampling) { delete s; return nullptr; }      // (tables copied above)
        // createIBLImportanceMap's pickFunc, image_textures.cpp:131: sin(M_PI * (y + 0.5f) / mapHeight) * luminance
        std::vector<float> values((size_t)e.map_width * e.map_height);
        for (uint32_t y = 0; y < e.map_height; ++y)
            for (uint32_t x = 0; x < e.map_width; ++x)
                values[(size_t)y * e.map_width + x] =
                    (float)(std::sin(M_PI * (y + 0.5f) / e.map_height) * e.importance[(size_t)y * e.map_width + x]);
        s->envDist.build(e.map_width, e.map_height, values);
    }
    setupCamera(s->camera, d->camera);
    buildBVH(*s);
    return s;
}

void slr_oracle_destroy(slr_oracle_scene* s) { delete s; }

int slr_oracle_components(const slr_oracle_scene* s) { return s->mode == SLRHIP_MODE_RGB ? 3 : 16; }

}  // extern "C"

namespace {

template <int N>
int renderT(slr_oracle_scene* s, const slrhip_render_settings* st, slrhip_shard shard, uint32_t sppBegin, uint32_t sppCount,
            int threads, float* fbSum, float* fbComp, slr_oracle_counters* counters) {
    const uint32_t W = (uint32_t)st->image_width, H = (uint32_t)st->image_height;
    const uint32_t tilesX = (W + 7) >> 3;                    // ImageSensor.cpp:43-44
    if (threads <= 0) threads = (int)std::thread::hardware_concurrency();
    if (threads <= 0) threads = 1;
    std::atomic<uint32_t> nextRow(0);
    std::vector<slr_oracle_counters> ctrs(threads);
    std::memset(ctrs.data(), 0, sizeof(slr_oracle_counters) * threads);
    auto worker = [&](int tid) {
        slr_oracle_counters& c = ctrs[tid];
        for (;;) {
            uint32_t y = nextRow.fetch_add(1);
            if (y >= H) break;
            for (uint32_t x = 0; x < W; ++x) {
                uint32_t tile = (y >> 3) * tilesX + (x >> 3);
                if (tile % shard.shard_count != shard.shard_index) continue;
                size_t o = ((size_t)y * W + x) * N;
                Kahan<Spec<N>> acc;
                for (int k = 0; k < N; ++k) { acc.result[k] = fbSum[o + k]; acc.comp[k] = fbComp[o + k]; }
                for (uint32_t p = sppBegin; p < sppBegin + sppCount; ++p) {
                    XorShift rng(sampleSeed(st->rng_seed, x, y, p), &c.rng_draws);
                    float px, py; Spec<N> contrib; Wls<N> wls;
                    pixelSample<N>(*s, *st, x, y, rng, &c, &px, &py, &contrib, &wls);
                    storageAdd(acc, wls, contrib);
                    ++c.samples;
                }
                for (int k = 0; k < N; ++k) { fbSum[o + k] = acc.result[k]; fbComp[o + k] = acc.comp[k]; }
            }
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(worker, t);
    worker(0);
    for (auto& t : pool) t.join();
    if (counters) for (int t = 0; t < threads; ++t) addCounters(counters, ctrs[t]);
    return 0;
}

// out[0..N) = what ImageSensor::add would add to the pixel (spectral: the binned, scaled addend), then p.x, p.y
template <int N>
int sampleT(slr_oracle_scene* s, const slrhip_render_settings* st, uint32_t px, uint32_t py, uint32_t pass, float* out) {
    XorShift rng(sampleSeed(st->rng_seed, px, py, pass));
    float fx, fy; Spec<N> contrib; Wls<N> wls;
    pixelSample<N>(*s, *st, px, py, rng, nullptr, &fx, &fy, &contrib, &wls);
    Kahan<Spec<N>> acc;
    storageAdd(acc, wls, contrib);
    for (int k = 0; k < N; ++k) out[k] = acc.result[k];
    out[N] = fx; out[N + 1] = fy;
    return 0;
}

// PathTracingRenderer.cpp:27-98 with numThreads == 1: topRand(seed); sampler(topRand.getUInt());
// passes outermost, tiles row-major (:74-79), pixels row-major inside a tile (:103-104).
template <int N>
int renderSerialT(slr_oracle_scene* s, const slrhip_render_settings* st, uint32_t spp, float* fbSum, slr_oracle_counters* counters) {
    const uint32_t W = (uint32_t)st->image_width, H = (uint32_t)st->image_height;
    const uint32_t tilesX = (W + 7) >> 3, tilesY = (H + 7) >> 3;
    XorShift topRand(st->rng_seed);
    slr_oracle_counters c;
    std::memset(&c, 0, sizeof(c));
    XorShift rng((int32_t)topRand.getUInt(), &c.rng_draws);
    std::vector<Kahan<Spec<N>>> fb((size_t)W * H);
    for (uint32_t p = 0; p < spp; ++p)
        for (uint32_t ty = 0; ty < tilesY; ++ty)
            for (uint32_t tx = 0; tx < tilesX; ++tx)
                for (uint32_t ly = 0; ly < 8; ++ly)
                    for (uint32_t lx = 0; lx < 8; ++lx) {
                        float px, py; Spec<N> contrib; Wls<N> wls;
                        pixelSample<N>(*s, *st, tx * 8 + lx, ty * 8 + ly, rng, &c, &px, &py, &contrib, &wls);
                        // ImageSensor::add ImageSensor.cpp:124-129
                        uint32_t ipx = std::min((uint32_t)px, W - 1), ipy = std::min((uint32_t)py, H - 1);
                        storageAdd(fb[(size_t)ipy * W + ipx], wls, contrib);
                        ++c.samples;
                    }
    for (size_t i = 0; i < fb.size(); ++i) for (int k = 0; k < N; ++k) fbSum[i * N + k] = fb[i].result[k];
    if (counters) addCounters(counters, c);
    return 0;
}

} // namespace

extern "C" {

int slr_oracle_render(slr_oracle_scene* s, const slrhip_render_settings* st, slrhip_shard shard, uint32_t sppBegin, uint32_t sppCount,
                      int threads, float* fbSum, float* fbComp, slr_oracle_counters* counters) {
    if (!s || !st || !fbSum || !fbComp || shard.shard_count == 0) return 1;
    return s->mode == SLRHIP_MODE_RGB ? renderT<3>(s, st, shard, sppBegin, sppCount, threads, fbSum, fbComp, counters)
                                      : renderT<16>(s, st, shard, sppBegin, sppCount, threads, fbSum, fbComp, counters);
}

int slr_oracle_sample(slr_oracle_scene* s, const slrhip_render_settings* st, uint32_t px, uint32_t py, uint32_t pass, float* out) {
    if (!s || !st || !out) return 1;
    return s->mode == SLRHIP_MODE_RGB ? sampleT<3>(s, st, px, py, pass, out) : sampleT<16>(s, st, px, py, pass, out);
}

int slr_oracle_bsdf_kat(slr_oracle_scene* s, uint32_t material, uint32_t n, const float* in, float wlOffset, float uLambda, float* out) {
    if (!s || !in || !out || material >= s->materials.size()) return 1;
    return s->mode == SLRHIP_MODE_RGB ? bsdfKatT<3>(s, material, n, in, wlOffset, uLambda, out)
                                      : bsdfKatT<16>(s, material, n, in, wlOffset, uLambda, out);
}

int slr_oracle_light_kat(slr_oracle_scene* s, uint32_t n, const float* in, float wlOffset, float uLambda, float* out) {
    if (!s || !in || !out) return 1;
    if (s->lightTris.empty() && !s->hasEnv) return 1;
    return s->mode == SLRHIP_MODE_RGB ? lightKatT<3>(s, n, in, wlOffset, uLambda, out) : lightKatT<16>(s, n, in, wlOffset, uLambda, out);
}

int slr_oracle_render_serial(slr_oracle_scene* s, const slrhip_render_settings* st, uint32_t spp, float* fbSum,
                             slr_oracle_counters* counters) {
    if (!s || !st || !fbSum) return 1;
    return s->mode == SLRHIP_MODE_RGB ? renderSerialT<3>(s, st, spp, fbSum, counters) : renderSerialT<16>(s, st, spp, fbSum, counters);
}

int slr_oracle_eval_spectrum(const slrhip_scene_desc* d, uint32_t index, float offset, float* out) {
    if (!d || !out || index >= d->num_spectra) return 1;
    Scene tmp;
    tmp.spectra.assign(d->spectra, d->spectra + d->num_spectra);
    if (d->spectrum_data) tmp.spectrumData.assign(d->spectrum_data, d->spectrum_data + d->num_spectrum_data);
    Wls<16> wls;
    for (int i = 0; i < 16; ++i) wls.lambdas[i] = kWavelengthLowBound + (kWavelengthHighBound - kWavelengthLowBound) * (i + offset) / 16;
    wls.selectedLambda = 0; wls.flags = 0;
    Spec<16> v = EvalSpectrum<16>::eval(tmp, (int32_t)index, wls);
    for (int k = 0; k < 16; ++k) out[k] = v[k];
    return 0;
}

int slr_oracle_trace(slr_oracle_scene* s, const slr_oracle_ray* rays, uint32_t n, slr_oracle_hit* hits) {
    if (!s || !rays || !hits) return 1;
    for (uint32_t i = 0; i < n; ++i) {
        Ray r;
        r.org = V3(rays[i].org[0], rays[i].org[1], rays[i].org[2]);
        r.dir = V3(rays[i].dir[0], rays[i].dir[1], rays[i].dir[2]);
        r.distMin = rays[i].dist_min; r.distMax = rays[i].dist_max;
        Isect isect;
        if (aggregateIntersect(*s, r, &isect, nullptr)) {
            hits[i].triangle = isect.tri; hits[i].dist = isect.dist; hits[i].b0 = isect.u; hits[i].b1 = isect.v;
        }
        else {
            hits[i].triangle = 0xFFFFFFFFu; hits[i].dist = INFINITY; hits[i].b0 = 0; hits[i].b1 = 0;
        }
    }
    return 0;
}

void slr_oracle_rng(int32_t seed, uint32_t n, uint32_t* uints, float* floats) {
    XorShift a(seed);
    for (uint32_t i = 0; i < n; ++i) uints[i] = a.getUInt();
    XorShift b(seed);
    for (uint32_t i = 0; i < n; ++i) floats[i] = b.getFloat0cTo1o();
}

} // extern "C"
