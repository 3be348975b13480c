/*
 * surf_host.hpp -- C++ host API of the MI355X wavefront path tracer.
 *
 * Same class names, constructor shapes and semantics as the reference's host
 * API, so a caller of the reference GPU path (main.cpp) switches by swapping
 * includes:
 *   Float2/Float3/Float4 + operators ...... headers/surf_math.h:25-200
 *   Mat4 / translate / scale / rotate ...... glm subset used by main.cpp:204-341, bvh.cpp:486-594
 *   Triangle / TriExtension / Mesh ......... headers/mesh.h:12-75, sources/mesh.cpp
 *   AABB / BvhNode / BvhBLAS ............... headers/bvh.h:12-90, sources/bvh.cpp:17-465
 *   Material ............................... headers/material.h:6-19
 *   GPUInstance / Instance ................. headers/bvh.h:93-147, sources/bvh.cpp:467-594
 *   BvhTLAS ................................ headers/bvh.h:149-193, sources/bvh.cpp:596-993
 *   SceneBackground / GPULightData ......... headers/scene.h:12-71
 *   GPUBatchInfo / GPUBatcher .............. headers/scene.h:73-88, sources/scene.cpp:61-157
 *   GPUScene ............................... headers/scene.h:90-123, sources/scene.cpp:159-282
 *   Camera / CameraUBO ..................... headers/camera.h, sources/camera.cpp
 *   RendererConfig / IRenderer / WaveFrontRenderer ... headers/renderer.h:24-97,207-436
 *
 * Differences, all deliberate: `RenderContext` is a HIP device handle (no
 * Vulkan), the UIManager argument is accepted and ignored (headless), and
 * WaveFrontRenderer adds headless readback (readAccumulator / finalizeRGBA8).
 * Record layouts are byte-identical to the reference (static_asserts below).
 * All GPU work goes through the C-ABI in surf_hip.h.
 */
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../surf_hip.h"

namespace surf {

using U32 = uint32_t;
using I32 = int32_t;
using F32 = float;
using SizeType = size_t;

constexpr F32 F32_FAR_AWAY = 1e30f;
constexpr F32 F32_EPSILON = 1e-5f;
constexpr F32 F32_PI = 3.14159265358979323846264f;
constexpr F32 F32_INV_PI = 0.31830988618379067153777f;
constexpr U32 UNSET_INDEX = ~0u;

/* ------------------------------------------------------------ vectors */
struct Float2 {
    F32 x, y;
    Float2() : x(0.0f), y(0.0f) {}
    explicit Float2(F32 s) : x(s), y(s) {}
    Float2(F32 x_, F32 y_) : x(x_), y(y_) {}
};

struct Float3 {
    F32 x, y, z;
    Float3() : x(0.0f), y(0.0f), z(0.0f) {}
    Float3(F32 s) : x(s), y(s), z(s) {}          /* implicit like the reference: F32 * Float3 */
    Float3(F32 x_, F32 y_, F32 z_) : x(x_), y(y_), z(z_) {}
    F32 operator[](SizeType i) const { return i == 0 ? x : (i == 1 ? y : z); }
    F32 dot(const Float3& o) const { return x * o.x + y * o.y + z * o.z; }
    Float3 cross(const Float3& o) const { return Float3(y * o.z - z * o.y, z * o.x - x * o.z, x * o.y - y * o.x); }
    F32 magnitude() const { return sqrtf(dot(*this)); }
    inline Float3 normalize() const;
};
inline Float3 operator+(const Float3& a, const Float3& b) { return Float3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Float3 operator-(const Float3& a, const Float3& b) { return Float3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline Float3 operator*(const Float3& a, const Float3& b) { return Float3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline Float3 operator/(const Float3& a, const Float3& b) { return Float3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline Float3 operator*(const Float3& a, F32 s) { return Float3(a.x * s, a.y * s, a.z * s); }
inline Float3 operator/(const Float3& a, F32 s) { return Float3(a.x / s, a.y / s, a.z / s); }
inline Float3& operator+=(Float3& a, const Float3& b) { a = a + b; return a; }
inline Float3& operator*=(Float3& a, const Float3& b) { a = a * b; return a; }
inline Float3 Float3::normalize() const { F32 inv = 1.0f / sqrtf(dot(*this)); return *this * inv; }
inline Float3 min(const Float3& a, const Float3& b) { return Float3(a.x < b.x ? a.x : b.x, a.y < b.y ? a.y : b.y, a.z < b.z ? a.z : b.z); }
inline Float3 max(const Float3& a, const Float3& b) { return Float3(a.x > b.x ? a.x : b.x, a.y > b.y ? a.y : b.y, a.z > b.z ? a.z : b.z); }

struct Float4 {
    F32 x, y, z, w;
    Float4() : x(0), y(0), z(0), w(0) {}
    Float4(F32 x_, F32 y_, F32 z_, F32 w_) : x(x_), y(y_), z(z_), w(w_) {}
    Float4(const Float3& v, F32 w_) : x(v.x), y(v.y), z(v.z), w(w_) {}
};

const Float3 WORLD_FORWARD(0.0f, 0.0f, -1.0f);   /* camera.h:7-9 */
const Float3 WORLD_RIGHT(1.0f, 0.0f, 0.0f);
const Float3 WORLD_UP(0.0f, 1.0f, 0.0f);

/* radians() of surf_math.h:231 (not glm::radians) */
inline F32 radians(F32 deg) { return (deg * F32_PI) * 0.005555555555555f; }

/* ------------------------------------------------------------ Mat4 (glm subset) */
struct Mat4 {
    F32 c[4][4];                         /* column major, glm::mat4 layout */
    explicit Mat4(F32 diag = 1.0f);
    Float4 operator*(const Float4& v) const;
};
Mat4 translate(const Mat4& m, const Float3& v);
Mat4 scale(const Mat4& m, const Float3& v);
Mat4 rotate(const Mat4& m, F32 angle, const Float3& axis);
Mat4 inverse(const Mat4& m);

/* ------------------------------------------------------------ mesh */
struct alignas(16) Triangle {
    alignas(16) Float3 v0;
    alignas(16) Float3 v1;
    alignas(16) Float3 v2;
    alignas(16) Float3 centroid;
    Triangle(Float3 v1, Float3 v0, Float3 v2);   /* argument order of mesh.cpp:13 */
};

struct alignas(16) TriExtension {
    alignas(16) Float3 n0;
    alignas(16) Float3 n1;
    alignas(16) Float3 n2;
    alignas(8) Float2 uv0;
    alignas(8) Float2 uv1;
    alignas(8) Float2 uv2;
};

class Mesh {
public:
    explicit Mesh(const std::string& path);      /* reads .obj or .obj.gz; throws std::runtime_error */
    Mesh(const std::string& path, unsigned threads);   /* parallel parse; same arrays for any thread count */
    Mesh() = default;
    std::vector<Triangle> triangles;
    std::vector<TriExtension> triExtensions;
};

/* ------------------------------------------------------------ BVH */
struct alignas(16) AABB {
    alignas(16) Float3 bbMin = Float3(INFINITY);
    alignas(16) Float3 bbMax = Float3(-INFINITY);
    void grow(const Float3& p) { bbMin = min(bbMin, p); bbMax = max(bbMax, p); }
    void grow(const AABB& b) { bbMin = min(bbMin, b.bbMin); bbMax = max(bbMax, b.bbMax); }
    F32 area() const;
    Float3 center() const;                        /* the reference's half-extent quirk, bvh.cpp:35-38 */
};

struct alignas(16) BvhNode {
    U32 leftFirst;
    U32 count;
    AABB boundingBox;
    bool isLeaf() const { return count != 0; }
};

/* Threads of the parallel BVH build: SURF_BUILD_THREADS, else OMP_NUM_THREADS,
 * else the hardware concurrency (capped at 64). */
unsigned defaultBuildThreads();

class BvhBLAS {
public:
    explicit BvhBLAS(Mesh* mesh);
    BvhBLAS(Mesh* mesh, unsigned threads);
    void build();                                 /* SURF_BUILD_THREADS / OMP_NUM_THREADS threads */
    void build(unsigned threads);                 /* same arrays for every thread count */
    void refit();
    const Mesh* mesh() const { return m_mesh; }
    SizeType triCount() const { return m_mesh->triangles.size(); }
    const U32* indices() const { return m_indices.data(); }
    U32 nodesUsed() const { return m_nodesUsed; }
    const BvhNode* nodePool() const { return m_nodes.data(); }
    const AABB& bounds() const { return m_nodes[0].boundingBox; }
    U32 depth() const;
private:
    Mesh* m_mesh;
    std::vector<U32> m_indices;
    std::vector<BvhNode> m_nodes;
    U32 m_nodesUsed = 2;
};

struct Material {
    alignas(4) F32 emissionStrength = 0.0f;
    alignas(4) F32 reflectivity = 0.0f;
    alignas(4) F32 refractivity = 0.0f;
    alignas(4) F32 indexOfRefraction = 1.0f;
    alignas(16) Float3 emissionColor = Float3(0.0f);
    alignas(16) Float3 albedo = Float3(0.0f);
    alignas(16) Float3 absorption = Float3(0.0f);
    bool isLight() const { return emissionStrength > 0.0f && (emissionColor.x > 0.0f || emissionColor.y > 0.0f || emissionColor.z > 0.0f); }
};

using GPUInstance = surf_gpu_instance;

class Instance {
public:
    Instance(BvhBLAS* blas, Material* material, Mat4 transform);
    const Mat4& transform() const { return m_transform; }
    void setTransform(const Mat4& transform);
    GPUInstance toGPUInstance() const;
    void updateInstanceData() { updateBounds(); }
    BvhBLAS* bvh;
    Material* material;
    AABB bounds;
    F32 area = 0.0f;
private:
    void updateBounds();
    void calculateMeshArea();
    Mat4 m_transform;
    Mat4 m_invTransform;
};

class BvhTLAS {
public:
    explicit BvhTLAS(std::vector<Instance> instances);
    void build();
    void refit();
    Instance& instance(SizeType i) { return m_instances[i]; }
    const std::vector<Instance>& instances() const { return m_instances; }
    const U32* indices() const { return m_indices.data(); }
    U32 nodesUsed() const { return m_nodesUsed; }
    const BvhNode* nodePool() const { return m_nodes.data(); }
    U32 depth() const;
private:
    std::vector<Instance> m_instances;
    std::vector<U32> m_indices;
    std::vector<BvhNode> m_nodes;
    U32 m_nodesUsed = 2;
};

/* ------------------------------------------------------------ scene */
enum class BackgroundType : U32 { SolidColor = 0, ColorGradient = 1 };

struct SceneBackground {
    alignas(4) BackgroundType type = BackgroundType::SolidColor;
    alignas(16) Float3 color = Float3(0.0f);
    struct {
        alignas(16) Float3 colorA = Float3(0.0f);
        alignas(16) Float3 colorB = Float3(0.0f);
    } gradient;
};

struct GPULightData { U32 lightInstanceIdx; U32 primitiveCount; };

struct GPUBatchInfo {
    std::vector<Triangle> triBuffer;
    std::vector<TriExtension> triExtBuffer;
    std::vector<U32> BLASIndices;
    std::vector<BvhNode> BLASNodes;
    std::vector<Material> materials;
    std::vector<GPUInstance> gpuInstances;
    std::vector<GPULightData> lights;
};

class GPUBatcher {
public:
    /* First-use order for meshes, BLASes and materials (the reference keys them
     * by pointer, an address-dependent but equivalent order). */
    static GPUBatchInfo createBatchInfo(const std::vector<Instance>& instances);
};

/* HIP device handle standing in for the reference's Vulkan RenderContext. */
struct RenderContext {
    int hipDevice = 0;
};

class GPUScene {
public:
    GPUScene(RenderContext* context, SceneBackground background, std::vector<Instance> instances);
    const SceneBackground& backgroundSettings() const { return m_background; }
    /* Scene::update / GPUScene::update (scene.cpp:267-282): rotate instance 3, refit, re-batch. */
    void update(F32 deltaTime);
    /* The scene as the C-ABI takes it (pointers into this object). */
    surf_scene_desc descriptor() const;
    const BvhTLAS& tlas() const { return m_sceneTlas; }
    U32 generation() const { return m_generation; }
    RenderContext* context() const { return m_context; }
private:
    RenderContext* m_context;
    SceneBackground m_background;
    BvhTLAS m_sceneTlas;
    GPUBatchInfo m_batchInfo;
    U32 m_generation = 0;
};

/* ------------------------------------------------------------ camera */
using CameraUBO = surf_camera_ubo;

struct ViewPlane { Float3 firstPixel, uVector, vVector; };

class Camera {
public:
    Camera(Float3 position, Float3 target, U32 screenWidth, U32 screenHeight, F32 fovY,
           F32 focalLength = 1.5f, F32 defocusAngle = 0.0f);
    Float3 right() const { return up.cross(forward).normalize(); }
    void generateViewPlane();
    CameraUBO toUBO() const;                      /* renderer.cpp:972-979 */
    Float3 position, forward, up;
    F32 screenWidth, screenHeight, fovY, focalLength, defocusAngle;
    ViewPlane viewPlane;
};

/* ------------------------------------------------------------ renderer */
struct RendererConfig {
    U32 maxBounces = 5;          /* unused by the reference's iterative path; kept */
    U32 samplesPerFrame = 1;     /* > 1: the throughput cutoff is off (surf_set_zero_cutoff's automatic default), so a
                                    lens TIR orbit runs to its end as in the reference -- up to millions of segments
                                    (seconds) for the frame holding it; maxSegments bounds it (surf_hip.h) */
    U32 maxSegments = 0;         /* 0: unbounded + Russian roulette (reference); N: cap (config C2) */
    bool lumenOutput = false;    /* WF_LUMEN_OUTPUT (renderer.cpp:31, default 0): frameInfo().energy from the
                                    accumulator; reading it drains the sample stream, so it is computed only
                                    when frameInfo() is read after a render */
};

struct FrameInstrumentationData {
    F32 energy = 0.0f;
    U32 totalSamples = 0;
};

struct FramebufferSize { U32 width, height; };

class UIManager;   /* accepted for signature compatibility, never used */

class IRenderer {
public:
    virtual ~IRenderer() = default;
    virtual void clearAccumulator() = 0;
    virtual void render(F32 deltaTime) = 0;
    virtual RendererConfig& config() = 0;
    virtual const FrameInstrumentationData& frameInfo() = 0;
};

class WaveFrontRenderer : public IRenderer {
public:
    WaveFrontRenderer(RenderContext* context, UIManager* uiManager, RendererConfig config,
                      FramebufferSize resolution, Camera& camera, GPUScene& scene);
    ~WaveFrontRenderer() override;
    WaveFrontRenderer(const WaveFrontRenderer&) = delete;
    WaveFrontRenderer& operator=(const WaveFrontRenderer&) = delete;

    void clearAccumulator() override;
    void render(F32 deltaTime) override;
    RendererConfig& config() override { return m_config; }
    const FrameInstrumentationData& frameInfo() override;

    /* headless additions */
    std::vector<F32> readAccumulator();           /* width*height*4 floats */
    std::vector<U32> finalizeRGBA8();             /* width*height RGBA8 words */
    std::vector<U32> displayRGBA8();              /* finalize image through fs_quad.frag's sqrt gamma */
    void synchronize();                           /* waits until every frame rendered so far is accumulated */
    /* first-hit feature buffers of the current camera and scene state (surf_read_aov;
     * width*height*4 values each): a float plane (position, normal or albedo), and the id plane */
    std::vector<F32> readAOV(surf_aov plane);
    std::vector<U32> readAOVIds();
    /* ... and one of the four to a buffer of width*height*16 bytes on the renderer's device, with no host
     * trip (surf_copy_aov_device): e.g. the position and normal planes for setSurfelSensorDevice */
    void copyAOVDevice(surf_aov plane, void* dstDevice);
    /* the same planes traced through mirrors and glass to the first surface that is neither, or to
     * link maxLinks (surf_read_aov_chain, which defines the chain; 0..SURF_AOV_CHAIN_MAX_LINKS) */
    std::vector<F32> readAOVChain(surf_aov plane, U32 maxLinks = 8);
    std::vector<U32> readAOVChainIds(U32 maxLinks = 8);
    /* which planes denoise() and denoiseSampled() read (surf_set_filter_guides): the first-hit
     * planes (the default) or the chain's at maxLinks; every other filter keeps the first-hit planes */
    void setFilterGuides(surf_guides guides, U32 maxLinks = 8);
    /* the sampled feature buffers (surf_read_aov_sampled, which states their arithmetic): the
     * first-hit features of the camera rays render() traces for frames first_sample ..
     * first_sample + samples - 1, reduced per pixel; a float plane (position, normal or albedo),
     * and an integer plane (id, matte key or matte count) */
    std::vector<F32> readAOVSampled(surf_aovs plane, const surf_aov_sampled_params& params);
    std::vector<U32> readAOVSampledIds(surf_aovs plane, const surf_aov_sampled_params& params);
    /* ... as the planes denoise(), denoiseSampled() and the regression filter read
     * (surf_set_filter_guides_sampled); setFilterGuides switches back */
    void setFilterGuidesSampled(const surf_aov_sampled_params& params);
    /* ray-traced ambient occlusion (surf_read_ao, which states the arithmetic): the openness plane
     * (bent normal, open share; width*height*4 floats) and the bits plane (sample mask, open count,
     * valid flag; width*height*4 words) of the current camera and scene */
    std::vector<F32> readAO(const surf_ao_params& params);
    std::vector<U32> readAOBits(const surf_ao_params& params);
    /* the rendered radiance through the edge-avoiding a-trous filter (surf_denoise; width*height*4
     * floats, w = 1): the accumulator and the feature buffers of the camera and scene of the last
     * render() call; the accumulator is left untouched.  The form without arguments takes
     * surf_denoise_default_params. */
    std::vector<F32> denoise(const surf_denoise_params& params);
    std::vector<F32> denoise();
    /* temporal accumulation for animated frames (surf_temporal_accumulate; width*height*4 floats,
     * w = 1): the samples since the last clear blended with the reprojected result of the previous
     * call.  Per displayed frame: move the scene and the camera, clearAccumulatorKeepSeed(),
     * render(), temporal().  spatial non-NULL: the returned image also went through the a-trous
     * filter.  The form without arguments takes surf_temporal_default_params and no spatial filter. */
    std::vector<F32> temporal(const surf_temporal_params& params, const surf_denoise_params* spatial);
    std::vector<F32> temporal();
    void resetTemporal();                         /* the next temporal() is a first frame */
    /* the same loop through the variance-guided filter (surf_svgf_accumulate): it shares temporal()'s
     * stored state, the two may be mixed.  The form without arguments takes both sets of default parameters. */
    std::vector<F32> svgf(const surf_temporal_params& params, const surf_svgf_params& filter);
    /* ... with the firefly clamp and / or the filtered-history feedback (surf_svgf_accumulate_ex; all zero: the form above) */
    std::vector<F32> svgf(const surf_temporal_params& params, const surf_svgf_params& filter, const surf_svgf_ext& ext);
    std::vector<F32> svgf();
    /* the per-sample second moments beside the accumulator (surf_set_sample_squares): switch them on
     * before the first render() or right after a clearAccumulator(); readSampleSquares() is the plane,
     * width*height*4 floats */
    void setSampleSquares(bool enabled);
    std::vector<F32> readSampleSquares();
    /* the rendered radiance through the sample-variance-guided filter (surf_denoise_sampled;
     * width*height*4 floats, w = 1), for stills from about 16 samples per pixel; needs
     * setSampleSquares(true).  The form without arguments takes surf_svgf_default_params. */
    std::vector<F32> denoiseSampled(const surf_svgf_params& params);
    std::vector<F32> denoiseSampled();
    /* per pixel the relative standard error of its mean luminance and their summary
     * (surf_noise_estimate); error non-NULL: it receives the image, width*height floats.  The form
     * without arguments takes surf_noise_default_params and writes no image. */
    surf_noise_summary noiseEstimate(const surf_noise_params& params, std::vector<F32>* error = nullptr);
    surf_noise_summary noiseEstimate();
    /* M partial accumulators per pixel beside the accumulator (surf_set_sample_buckets; M = 2, 4, 8 or
     * 16, 0 = off): switch them on before the first render() or right after a clearAccumulator();
     * readSampleBuckets() is the M planes, bucket-major, M*width*height*4 floats */
    void setSampleBuckets(U32 M);
    std::vector<F32> readSampleBuckets();
    /* the median-of-means estimate of the accumulator from the buckets (surf_robust_accumulator): an
     * accumulator plane, width*height*4 floats, the mean is rgb / w; trim non-NULL: it receives per
     * pixel the bucket means dropped at either end, width*height bytes; summary non-NULL: the counts.
     * The form without arguments takes surf_robust_default_params. */
    std::vector<F32> robust(const surf_robust_params& params, std::vector<uint8_t>* trim = nullptr, surf_robust_summary* summary = nullptr);
    std::vector<F32> robust();
    /* the dual-buffer non-local-means filter on the buckets' two half images (surf_denoise_nlm; needs
     * setSampleBuckets): the filtered image, width*height*4 floats (rgb, 1); err non-NULL: it receives
     * the per-pixel error estimate from the two filtered halves' difference, the same size.  Reads no
     * feature buffer.  The form without arguments takes surf_nlm_default_params. */
    std::vector<F32> denoiseNlm(const surf_nlm_params& params, std::vector<F32>* err = nullptr);
    std::vector<F32> denoiseNlm();
    /* the first-order feature regression filter on the same two half images and the feature buffers
     * surf_set_filter_guides selects (surf_denoise_regress; needs setSampleBuckets): the filtered image
     * and, err non-NULL, its error estimate, as denoiseNlm returns them.  The form without arguments
     * takes surf_regress_default_params. */
    std::vector<F32> denoiseRegress(const surf_regress_params& params, std::vector<F32>* err = nullptr);
    std::vector<F32> denoiseRegress();
    /* the active-pixel mask (surf_set_pixel_mask): width*height bytes, nonzero = active, render()
     * then traces those pixels only; an empty vector = every pixel.  pixelMask: the mask as set and,
     * where asked for, its active count. */
    void setPixelMask(const std::vector<uint8_t>& mask);
    std::vector<uint8_t> pixelMask(U32* activeCount = nullptr);
    /* the surfel sensor (surf_set_surfel_sensor, whose header comment defines it): width*height float4
     * records each, position and normal (w ignored; a (0, 0, 0) normal marks an invalid texel); render()
     * then starts its samples at those points and the accumulator holds their light map.  The device form
     * takes two pointers on the renderer's device (surf_set_surfel_sensor_device).  clearSurfelSensor:
     * back to the camera.  surfelSensor: whether one is set and, where asked for, its valid texels. */
    void setSurfelSensor(const std::vector<F32>& position, const std::vector<F32>& normal);
    void setSurfelSensorDevice(const void* positionDevice, const void* normalDevice);
    void clearSurfelSensor();
    bool surfelSensor(U32* validTexels = nullptr);
    /* the light-map atlas (surf_atlas_*, whose header comment defines the three stages) on the renderer's scene.
     * buildAtlas: the charts' UV layouts rasterized into one surfel per texel of a W x H atlas of its own size:
     * position, normal (what setSurfelSensor takes when W x H is the renderer's frame), albedo, ids, the summary.
     * buildAtlasDevice: the same into four planes on the renderer's device (NULL: not wanted).  finishAtlas: an
     * accumulator-form plane and the build's albedo plane to the light map, its valid bytes into *valid.
     * dilateAtlas: `iterations` gutter-fill passes; valid is read and replaced. */
    struct AtlasPlanes {
        std::vector<F32> position, normal, albedo;
        std::vector<U32> ids;
        surf_atlas_summary summary;
    };
    AtlasPlanes buildAtlas(const std::vector<surf_atlas_chart>& charts, U32 W, U32 H);
    surf_atlas_summary buildAtlasDevice(const std::vector<surf_atlas_chart>& charts, U32 W, U32 H, void* positionDevice, void* normalDevice,
                                        void* albedoDevice, void* idsDevice);
    std::vector<F32> finishAtlas(U32 W, U32 H, const std::vector<F32>& acc, const std::vector<F32>& albedo, std::vector<uint8_t>* valid = nullptr);
    std::vector<F32> dilateAtlas(U32 W, U32 H, const std::vector<F32>& rgba, std::vector<uint8_t>& valid, U32 iterations);
    /* builds the mask from the noise estimate and sets it (surf_mask_from_noise); returns the active
     * count.  Needs setSampleSquares(true). */
    U32 maskFromNoise(const surf_adaptive_mask_params& params);
    /* renders until converged (surf_render_adaptive, whose header comment defines the loop): 1-sample
     * frames from the renderer's next sample index on an empty accumulator, with
     * setSampleSquares(true); the camera and the scene are pushed first, as render() pushes them.
     * roundActive non-NULL: the active count of each round.  params' first_sample_index and
     * max_segments are replaced by the renderer's.  The form without arguments takes
     * surf_adaptive_default_params. */
    surf_adaptive_summary renderAdaptive(const surf_adaptive_params& params, std::vector<U32>* roundActive = nullptr);
    surf_adaptive_summary renderAdaptive();
    /* filters the buckets' halves, builds the mask from the filter's error estimate and sets it
     * (surf_mask_from_nlm); returns the active count.  Needs setSampleBuckets. */
    U32 maskFromNlm(const surf_nlm_params& nlm, const surf_error_mask_params& params);
    /* renders until the filtered picture has converged (surf_render_adaptive_nlm, whose header comment
     * defines the loop): 1-sample frames from the renderer's next sample index on an empty
     * accumulator, with setSampleBuckets; the camera and the scene are pushed first, as render()
     * pushes them.  image and err non-NULL: the filter's two outputs of the final state, width*height*4
     * floats each; roundActive non-NULL: the active count of each round.  params' first_sample_index
     * and max_segments are replaced by the renderer's.  The form without params takes
     * surf_adaptive_nlm_default_params. */
    surf_adaptive_nlm_summary renderAdaptiveNlm(const surf_adaptive_nlm_params& params, std::vector<F32>* image = nullptr,
                                                std::vector<F32>* err = nullptr, std::vector<U32>* roundActive = nullptr);
    surf_adaptive_nlm_summary renderAdaptiveNlm(std::vector<F32>* image = nullptr);
    /* RGBA8 with each pixel divided by its own sample count (surf_finalize_rgba8_weighted) */
    std::vector<U32> finalizeWeighted(bool display = false);
    /* the display stage on the accumulator (surf_display): metered or manual exposure, optional bloom, tone curve,
     * transfer function, ordered dither; width*height RGBA8 words, *meter (may be NULL) the meter's result */
    std::vector<U32> display(const surf_display_params& params, surf_display_meter_result* meter = nullptr);
    /* clearAccumulator() for that loop: the next render() goes on with the sample indices after
     * those already rendered instead of repeating the cleared frame's sample stream (a plain
     * clearAccumulator() starts again from sample 0, as the reference does) */
    void clearAccumulatorKeepSeed();
    surf_ctx* handle() const { return m_ctx; }
private:
    void pushSceneAndCamera();                    /* what render() re-reads per frame: instance updates, the camera */
    surf_ctx* m_ctx = nullptr;
    RendererConfig m_config;
    FramebufferSize m_resolution;
    Camera& m_camera;
    GPUScene& m_scene;
    U32 m_sceneGeneration = 0;
    U32 m_totalSamples = 0;
    U32 m_firstSample = 0;                        /* sample index of the first sample after the last clear */
    FrameInstrumentationData m_frameInfo;
    bool m_energyStale = false;
};

static_assert(sizeof(Triangle) == sizeof(surf_triangle), "Triangle layout");
static_assert(sizeof(TriExtension) == sizeof(surf_tri_extension), "TriExtension layout");
static_assert(sizeof(BvhNode) == sizeof(surf_bvh_node), "BvhNode layout");
static_assert(sizeof(Material) == sizeof(surf_material), "Material layout");
static_assert(sizeof(SceneBackground) == sizeof(surf_background), "SceneBackground layout");
static_assert(sizeof(GPULightData) == sizeof(surf_light), "GPULightData layout");

}  // namespace surf
