/*
 * renderer_host.cpp -- WaveFrontRenderer (headers/renderer.h:207-436) on top of
 * the C-ABI.  render() keeps the reference's CPU frame semantics: every call
 * adds config().samplesPerFrame samples per pixel, seeded once per frame from
 * the running sample count (renderer.cpp:169) and run in sequence on that one
 * RNG stream (renderer.cpp:171-181), and camera state is re-read per frame
 * (renderer.cpp:972-979).  render() returns once the frame's samples are
 * issued: consecutive frames form one sample stream on the device (no
 * per-frame drain); reads (accumulator, images, frameInfo() with lumenOutput)
 * drain it.  Errors throw std::runtime_error (the reference aborts through
 * VK_CHECK).
 */
#include "surf/surf_host.hpp"

#include <algorithm>
#include <stdexcept>
#include <string>

namespace surf {

namespace {
void check(int rc, surf_ctx* ctx, const char* what) {
    if (rc != SURF_OK) throw std::runtime_error(std::string(what) + ": " + surf_last_error(ctx));
}
}  // namespace

WaveFrontRenderer::WaveFrontRenderer(RenderContext* context, UIManager* /*uiManager*/, RendererConfig config,
                                     FramebufferSize resolution, Camera& camera, GPUScene& scene)
    : m_config(config), m_resolution(resolution), m_camera(camera), m_scene(scene) {
    const int dev = context ? context->hipDevice : 0;
    check(surf_create(dev, resolution.width, resolution.height, 0, resolution.height, &m_ctx), nullptr, "surf_create");
    const surf_scene_desc desc = scene.descriptor();
    check(surf_upload_scene(m_ctx, &desc), m_ctx, "surf_upload_scene");
    m_sceneGeneration = scene.generation();
}

WaveFrontRenderer::~WaveFrontRenderer() { surf_destroy(m_ctx); }

void WaveFrontRenderer::clearAccumulator() {
    check(surf_clear_accumulator(m_ctx), m_ctx, "surf_clear_accumulator");
    m_totalSamples = 0;
    m_firstSample = 0;
    m_frameInfo = FrameInstrumentationData{};
    m_energyStale = false;
}

void WaveFrontRenderer::clearAccumulatorKeepSeed() {
    const U32 next = m_firstSample + m_totalSamples;
    clearAccumulator();
    m_firstSample = next;
}

void WaveFrontRenderer::pushSceneAndCamera() {
    if (m_scene.generation() != m_sceneGeneration) {
        /* GPUScene::update (scene.cpp:267-282) re-uploads the instance records,
         * TLAS indices and TLAS nodes; geometry and BLASes stay resident */
        const surf_scene_desc desc = m_scene.descriptor();
        if (surf_update_instances(m_ctx, desc.instances, desc.instance_count, desc.tlas_indices, desc.tlas_nodes,
                                  desc.tlas_node_count, desc.lights, desc.light_count) != SURF_OK)
            check(surf_upload_scene(m_ctx, &desc), m_ctx, "surf_upload_scene");
        m_sceneGeneration = m_scene.generation();
    }
    const CameraUBO ubo = m_camera.toUBO();
    check(surf_set_camera(m_ctx, &ubo), m_ctx, "surf_set_camera");
}

void WaveFrontRenderer::render(F32 /*deltaTime*/) {
    pushSceneAndCamera();
    /* one frame of samplesPerFrame samples, seeded from the running sample
     * count, its samples chaining their RNG state (renderer.cpp:160-188) */
    const U32 spp = m_config.samplesPerFrame ? m_config.samplesPerFrame : 1u;
    check(surf_render(m_ctx, 1, m_firstSample + m_totalSamples, m_config.maxSegments, spp), m_ctx, "surf_render");
    m_totalSamples += spp;
    m_frameInfo.totalSamples = m_totalSamples;
    m_energyStale = true;       /* render() itself never waits for the stream (no per-frame drain) */
}

/* The reference computes the Lumen energy only with WF_LUMEN_OUTPUT
 * (renderer.cpp:31, off by default; :955-969), from the accumulator of the
 * frames rendered so far.  Here it is computed when asked for: the energy
 * needs every rendered frame accumulated, which drains the sample stream. */
const FrameInstrumentationData& WaveFrontRenderer::frameInfo() {
    if (m_config.lumenOutput && m_energyStale && m_totalSamples) {
        surf_stats st;
        check(surf_get_stats(m_ctx, &st), m_ctx, "surf_get_stats");
        m_frameInfo.energy = st.energy;
        m_energyStale = false;
    }
    return m_frameInfo;
}

void WaveFrontRenderer::synchronize() { check(surf_synchronize(m_ctx), m_ctx, "surf_synchronize"); }

std::vector<F32> WaveFrontRenderer::readAccumulator() {
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_accumulator(m_ctx, out.data()), m_ctx, "surf_read_accumulator");
    return out;
}

std::vector<U32> WaveFrontRenderer::finalizeRGBA8() {
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height);
    check(surf_finalize_rgba8(m_ctx, out.data()), m_ctx, "surf_finalize_rgba8");
    return out;
}

/* The feature buffers follow the camera and the scene as the next render()
 * would see them (also before the first render() call). */
std::vector<F32> WaveFrontRenderer::readAOV(surf_aov plane) {
    if (plane != SURF_AOV_POSITION && plane != SURF_AOV_NORMAL && plane != SURF_AOV_ALBEDO)
        throw std::runtime_error("readAOV: not a float plane (the id plane is readAOVIds)");
    pushSceneAndCamera();
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_aov(m_ctx, plane, out.data()), m_ctx, "surf_read_aov");
    return out;
}

void WaveFrontRenderer::copyAOVDevice(surf_aov plane, void* dstDevice) {
    pushSceneAndCamera();
    check(surf_copy_aov_device(m_ctx, plane, dstDevice), m_ctx, "surf_copy_aov_device");
}

std::vector<U32> WaveFrontRenderer::readAOVIds() {
    pushSceneAndCamera();
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_aov(m_ctx, SURF_AOV_ID, out.data()), m_ctx, "surf_read_aov");
    return out;
}

std::vector<F32> WaveFrontRenderer::readAOVChain(surf_aov plane, U32 maxLinks) {
    if (plane != SURF_AOV_POSITION && plane != SURF_AOV_NORMAL && plane != SURF_AOV_ALBEDO)
        throw std::runtime_error("readAOVChain: not a float plane (the id plane is readAOVChainIds)");
    pushSceneAndCamera();
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_aov_chain(m_ctx, plane, maxLinks, out.data()), m_ctx, "surf_read_aov_chain");
    return out;
}

std::vector<U32> WaveFrontRenderer::readAOVChainIds(U32 maxLinks) {
    pushSceneAndCamera();
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_aov_chain(m_ctx, SURF_AOV_ID, maxLinks, out.data()), m_ctx, "surf_read_aov_chain");
    return out;
}

void WaveFrontRenderer::setFilterGuides(surf_guides guides, U32 maxLinks) {
    check(surf_set_filter_guides(m_ctx, guides, maxLinks), m_ctx, "surf_set_filter_guides");
}

std::vector<F32> WaveFrontRenderer::readAOVSampled(surf_aovs plane, const surf_aov_sampled_params& params) {
    if (plane != SURF_AOVS_POSITION && plane != SURF_AOVS_NORMAL && plane != SURF_AOVS_ALBEDO)
        throw std::runtime_error("readAOVSampled: not a float plane (the id and matte planes are readAOVSampledIds)");
    pushSceneAndCamera();
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_aov_sampled(m_ctx, &params, plane, out.data()), m_ctx, "surf_read_aov_sampled");
    return out;
}

std::vector<U32> WaveFrontRenderer::readAOVSampledIds(surf_aovs plane, const surf_aov_sampled_params& params) {
    if (plane != SURF_AOVS_ID && plane != SURF_AOVS_MATTE_KEY && plane != SURF_AOVS_MATTE_COUNT)
        throw std::runtime_error("readAOVSampledIds: not an integer plane (the float planes are readAOVSampled)");
    pushSceneAndCamera();
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_aov_sampled(m_ctx, &params, plane, out.data()), m_ctx, "surf_read_aov_sampled");
    return out;
}

void WaveFrontRenderer::setFilterGuidesSampled(const surf_aov_sampled_params& params) {
    check(surf_set_filter_guides_sampled(m_ctx, &params), m_ctx, "surf_set_filter_guides_sampled");
}

std::vector<F32> WaveFrontRenderer::readAO(const surf_ao_params& params) {
    pushSceneAndCamera();
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_ao(m_ctx, &params, SURF_AO_OPENNESS, out.data()), m_ctx, "surf_read_ao");
    return out;
}

std::vector<U32> WaveFrontRenderer::readAOBits(const surf_ao_params& params) {
    pushSceneAndCamera();
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_ao(m_ctx, &params, SURF_AO_BITS, out.data()), m_ctx, "surf_read_ao");
    return out;
}

/* The filter reads the accumulator beside the feature buffers, so it keeps
 * the camera and the scene of the last render() call: those the accumulated
 * samples saw. */
std::vector<F32> WaveFrontRenderer::denoise(const surf_denoise_params& params) {
    if (m_totalSamples == 0) throw std::runtime_error("denoise: nothing rendered since the last clear");
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_denoise(m_ctx, &params, out.data()), m_ctx, "surf_denoise");
    return out;
}

std::vector<F32> WaveFrontRenderer::denoise() {
    surf_denoise_params params;
    check(surf_denoise_default_params(&params), m_ctx, "surf_denoise_default_params");
    return denoise(params);
}

/* Like denoise(), the blend keeps the camera and the scene of the last render() call. */
std::vector<F32> WaveFrontRenderer::temporal(const surf_temporal_params& params, const surf_denoise_params* spatial) {
    if (m_totalSamples == 0) throw std::runtime_error("temporal: nothing rendered since the last clear");
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_temporal_accumulate(m_ctx, &params, spatial, out.data()), m_ctx, "surf_temporal_accumulate");
    return out;
}

std::vector<F32> WaveFrontRenderer::temporal() {
    surf_temporal_params params;
    check(surf_temporal_default_params(&params), m_ctx, "surf_temporal_default_params");
    return temporal(params, nullptr);
}

std::vector<F32> WaveFrontRenderer::svgf(const surf_temporal_params& params, const surf_svgf_params& filter) {
    if (m_totalSamples == 0) throw std::runtime_error("svgf: nothing rendered since the last clear");
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_svgf_accumulate(m_ctx, &params, &filter, out.data()), m_ctx, "surf_svgf_accumulate");
    return out;
}

std::vector<F32> WaveFrontRenderer::svgf(const surf_temporal_params& params, const surf_svgf_params& filter, const surf_svgf_ext& ext) {
    if (m_totalSamples == 0) throw std::runtime_error("svgf: nothing rendered since the last clear");
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_svgf_accumulate_ex(m_ctx, &params, &filter, &ext, out.data()), m_ctx, "surf_svgf_accumulate_ex");
    return out;
}

std::vector<F32> WaveFrontRenderer::svgf() {
    surf_temporal_params params;
    surf_svgf_params filter;
    check(surf_temporal_default_params(&params), m_ctx, "surf_temporal_default_params");
    check(surf_svgf_default_params(&filter), m_ctx, "surf_svgf_default_params");
    return svgf(params, filter);
}

void WaveFrontRenderer::setSampleSquares(bool enabled) {
    check(surf_set_sample_squares(m_ctx, enabled ? 1 : 0), m_ctx, "surf_set_sample_squares");
}

std::vector<F32> WaveFrontRenderer::readSampleSquares() {
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_read_sample_squares(m_ctx, out.data()), m_ctx, "surf_read_sample_squares");
    return out;
}

/* Like denoise(), the filter keeps the camera and the scene of the last render() call. */
std::vector<F32> WaveFrontRenderer::denoiseSampled(const surf_svgf_params& params) {
    if (m_totalSamples == 0) throw std::runtime_error("denoiseSampled: nothing rendered since the last clear");
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    check(surf_denoise_sampled(m_ctx, &params, out.data()), m_ctx, "surf_denoise_sampled");
    return out;
}

std::vector<F32> WaveFrontRenderer::denoiseSampled() {
    surf_svgf_params params;
    check(surf_svgf_default_params(&params), m_ctx, "surf_svgf_default_params");
    return denoiseSampled(params);
}

surf_noise_summary WaveFrontRenderer::noiseEstimate(const surf_noise_params& params, std::vector<F32>* error) {
    if (error) error->assign((size_t)m_resolution.width * m_resolution.height, 0.0f);
    surf_noise_summary summary{};
    check(surf_noise_estimate(m_ctx, &params, error ? error->data() : nullptr, &summary), m_ctx, "surf_noise_estimate");
    return summary;
}

surf_noise_summary WaveFrontRenderer::noiseEstimate() {
    surf_noise_params params;
    check(surf_noise_default_params(&params), m_ctx, "surf_noise_default_params");
    return noiseEstimate(params, nullptr);
}

void WaveFrontRenderer::setSampleBuckets(U32 M) {
    check(surf_set_sample_buckets(m_ctx, M), m_ctx, "surf_set_sample_buckets");
}

std::vector<F32> WaveFrontRenderer::readSampleBuckets() {
    U32 M = 0;
    check(surf_get_sample_buckets(m_ctx, &M), m_ctx, "surf_get_sample_buckets");
    std::vector<F32> out((size_t)M * m_resolution.width * m_resolution.height * 4);
    check(surf_read_sample_buckets(m_ctx, out.data()), m_ctx, "surf_read_sample_buckets");
    return out;
}

std::vector<F32> WaveFrontRenderer::robust(const surf_robust_params& params, std::vector<uint8_t>* trim, surf_robust_summary* summary) {
    const size_t npx = (size_t)m_resolution.width * m_resolution.height;
    std::vector<F32> out(npx * 4);
    if (trim) trim->assign(npx, 0);
    check(surf_robust_accumulator(m_ctx, &params, out.data(), trim ? trim->data() : nullptr, summary), m_ctx, "surf_robust_accumulator");
    return out;
}

std::vector<F32> WaveFrontRenderer::robust() {
    surf_robust_params params;
    check(surf_robust_default_params(&params), m_ctx, "surf_robust_default_params");
    return robust(params);
}

std::vector<F32> WaveFrontRenderer::denoiseNlm(const surf_nlm_params& params, std::vector<F32>* err) {
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    if (err) err->assign(out.size(), 0.0f);
    check(surf_denoise_nlm(m_ctx, &params, out.data(), err ? err->data() : nullptr), m_ctx, "surf_denoise_nlm");
    return out;
}

std::vector<F32> WaveFrontRenderer::denoiseNlm() {
    surf_nlm_params params;
    check(surf_nlm_default_params(&params), m_ctx, "surf_nlm_default_params");
    return denoiseNlm(params);
}

std::vector<F32> WaveFrontRenderer::denoiseRegress(const surf_regress_params& params, std::vector<F32>* err) {
    std::vector<F32> out((size_t)m_resolution.width * m_resolution.height * 4);
    if (err) err->assign(out.size(), 0.0f);
    check(surf_denoise_regress(m_ctx, &params, out.data(), err ? err->data() : nullptr), m_ctx, "surf_denoise_regress");
    return out;
}

std::vector<F32> WaveFrontRenderer::denoiseRegress() {
    surf_regress_params params;
    check(surf_regress_default_params(&params), m_ctx, "surf_regress_default_params");
    return denoiseRegress(params);
}

void WaveFrontRenderer::setPixelMask(const std::vector<uint8_t>& mask) {
    if (!mask.empty() && mask.size() != (size_t)m_resolution.width * m_resolution.height)
        throw std::runtime_error("setPixelMask: the mask is not width*height bytes");
    check(surf_set_pixel_mask(m_ctx, mask.empty() ? nullptr : mask.data()), m_ctx, "surf_set_pixel_mask");
}

std::vector<uint8_t> WaveFrontRenderer::pixelMask(U32* activeCount) {
    std::vector<uint8_t> out((size_t)m_resolution.width * m_resolution.height);
    uint32_t n = 0;
    check(surf_get_pixel_mask(m_ctx, out.data(), &n), m_ctx, "surf_get_pixel_mask");
    if (activeCount) *activeCount = n;
    return out;
}

void WaveFrontRenderer::setSurfelSensor(const std::vector<F32>& position, const std::vector<F32>& normal) {
    const size_t n = (size_t)m_resolution.width * m_resolution.height * 4;
    if (position.size() != n || normal.size() != n)
        throw std::runtime_error("setSurfelSensor: position and normal are not width*height*4 floats each");
    check(surf_set_surfel_sensor(m_ctx, position.data(), normal.data()), m_ctx, "surf_set_surfel_sensor");
}

void WaveFrontRenderer::setSurfelSensorDevice(const void* positionDevice, const void* normalDevice) {
    if (!positionDevice || !normalDevice) throw std::runtime_error("setSurfelSensorDevice: NULL device pointer");
    check(surf_set_surfel_sensor_device(m_ctx, positionDevice, normalDevice), m_ctx, "surf_set_surfel_sensor_device");
}

WaveFrontRenderer::AtlasPlanes WaveFrontRenderer::buildAtlas(const std::vector<surf_atlas_chart>& charts, U32 W, U32 H) {
    const surf_scene_desc desc = m_scene.descriptor();
    AtlasPlanes out{};
    /* sized only for an atlas the library accepts: it refuses the others before it writes */
    const size_t n = W && H && W <= 16384 && H <= 16384 ? (size_t)W * H * 4 : 4;
    out.position.resize(n); out.normal.resize(n); out.albedo.resize(n); out.ids.resize(n);
    check(surf_atlas_build(m_ctx, &desc, charts.data(), (U32)charts.size(), W, H, out.position.data(), out.normal.data(), out.albedo.data(),
                           out.ids.data(), &out.summary), m_ctx, "surf_atlas_build");
    return out;
}

surf_atlas_summary WaveFrontRenderer::buildAtlasDevice(const std::vector<surf_atlas_chart>& charts, U32 W, U32 H, void* positionDevice,
                                                       void* normalDevice, void* albedoDevice, void* idsDevice) {
    const surf_scene_desc desc = m_scene.descriptor();
    surf_atlas_summary s{};
    check(surf_atlas_build_device(m_ctx, &desc, charts.data(), (U32)charts.size(), W, H, positionDevice, normalDevice, albedoDevice, idsDevice, &s),
          m_ctx, "surf_atlas_build_device");
    return s;
}

std::vector<F32> WaveFrontRenderer::finishAtlas(U32 W, U32 H, const std::vector<F32>& acc, const std::vector<F32>& albedo, std::vector<uint8_t>* valid) {
    const size_t npx = (size_t)W * H;
    if (acc.size() != npx * 4 || albedo.size() != npx * 4) throw std::runtime_error("finishAtlas: acc and albedo are not W*H*4 floats each");
    std::vector<F32> out(npx * 4);
    std::vector<uint8_t> v(npx);
    check(surf_atlas_finish(m_ctx, W, H, acc.data(), albedo.data(), out.data(), v.data()), m_ctx, "surf_atlas_finish");
    if (valid) valid->swap(v);
    return out;
}

std::vector<F32> WaveFrontRenderer::dilateAtlas(U32 W, U32 H, const std::vector<F32>& rgba, std::vector<uint8_t>& valid, U32 iterations) {
    const size_t npx = (size_t)W * H;
    if (rgba.size() != npx * 4 || valid.size() != npx) throw std::runtime_error("dilateAtlas: rgba is not W*H*4 floats or valid not W*H bytes");
    std::vector<F32> out(npx * 4);
    std::vector<uint8_t> v(npx);
    check(surf_atlas_dilate(m_ctx, W, H, rgba.data(), valid.data(), iterations, out.data(), v.data()), m_ctx, "surf_atlas_dilate");
    valid.swap(v);
    return out;
}

void WaveFrontRenderer::clearSurfelSensor() { check(surf_set_surfel_sensor(m_ctx, nullptr, nullptr), m_ctx, "surf_set_surfel_sensor"); }

bool WaveFrontRenderer::surfelSensor(U32* validTexels) {
    int kind = 0;
    uint32_t valid = 0;
    check(surf_get_sensor(m_ctx, &kind, &valid), m_ctx, "surf_get_sensor");
    if (validTexels) *validTexels = valid;
    return kind == SURF_SENSOR_SURFELS;
}

U32 WaveFrontRenderer::maskFromNoise(const surf_adaptive_mask_params& params) {
    uint32_t n = 0;
    check(surf_mask_from_noise(m_ctx, &params, &n), m_ctx, "surf_mask_from_noise");
    return n;
}

surf_adaptive_summary WaveFrontRenderer::renderAdaptive(const surf_adaptive_params& params, std::vector<U32>* roundActive) {
    pushSceneAndCamera();
    surf_adaptive_params p = params;
    p.first_sample_index = m_firstSample + m_totalSamples;
    p.max_segments = m_config.maxSegments;
    const U32 cap = p.batch ? (p.mask.max_samples - std::min(p.mask.min_samples, p.mask.max_samples)) / p.batch + 1u : 0u;
    if (roundActive) roundActive->assign(cap, 0u);
    surf_adaptive_summary summary{};
    check(surf_render_adaptive(m_ctx, &p, roundActive ? roundActive->data() : nullptr, roundActive ? cap : 0u, &summary), m_ctx,
          "surf_render_adaptive");
    if (roundActive) roundActive->resize(summary.rounds);
    m_totalSamples += summary.frames;
    m_frameInfo.totalSamples = m_totalSamples;
    m_energyStale = true;
    return summary;
}

surf_adaptive_summary WaveFrontRenderer::renderAdaptive() {
    surf_adaptive_params params;
    check(surf_adaptive_default_params(&params), m_ctx, "surf_adaptive_default_params");
    return renderAdaptive(params, nullptr);
}

U32 WaveFrontRenderer::maskFromNlm(const surf_nlm_params& nlm, const surf_error_mask_params& params) {
    uint32_t n = 0;
    check(surf_mask_from_nlm(m_ctx, &nlm, &params, &n), m_ctx, "surf_mask_from_nlm");
    return n;
}

surf_adaptive_nlm_summary WaveFrontRenderer::renderAdaptiveNlm(const surf_adaptive_nlm_params& params, std::vector<F32>* image,
                                                               std::vector<F32>* err, std::vector<U32>* roundActive) {
    pushSceneAndCamera();
    surf_adaptive_nlm_params p = params;
    p.first_sample_index = m_firstSample + m_totalSamples;
    p.max_segments = m_config.maxSegments;
    const U32 cap = p.batch ? (p.mask.max_samples - std::min(p.mask.min_samples, p.mask.max_samples)) / p.batch + 1u : 0u;
    if (roundActive) roundActive->assign(cap, 0u);
    const size_t floats = (size_t)m_resolution.width * m_resolution.height * 4;
    if (image) image->assign(floats, 0.0f);
    if (err) err->assign(floats, 0.0f);
    surf_adaptive_nlm_summary summary{};
    check(surf_render_adaptive_nlm(m_ctx, &p, image ? image->data() : nullptr, err ? err->data() : nullptr,
                                   roundActive ? roundActive->data() : nullptr, roundActive ? cap : 0u, &summary),
          m_ctx, "surf_render_adaptive_nlm");
    if (roundActive) roundActive->resize(summary.rounds);
    m_totalSamples += summary.frames;
    m_frameInfo.totalSamples = m_totalSamples;
    m_energyStale = true;
    return summary;
}

surf_adaptive_nlm_summary WaveFrontRenderer::renderAdaptiveNlm(std::vector<F32>* image) {
    surf_adaptive_nlm_params params;
    check(surf_adaptive_nlm_default_params(&params), m_ctx, "surf_adaptive_nlm_default_params");
    return renderAdaptiveNlm(params, image, nullptr, nullptr);
}

std::vector<U32> WaveFrontRenderer::finalizeWeighted(bool display) {
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height);
    check(surf_finalize_rgba8_weighted(m_ctx, display ? 1 : 0, out.data()), m_ctx, "surf_finalize_rgba8_weighted");
    return out;
}

std::vector<U32> WaveFrontRenderer::display(const surf_display_params& params, surf_display_meter_result* meter) {
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height);
    check(surf_display(m_ctx, &params, out.data(), meter), m_ctx, "surf_display");
    return out;
}

void WaveFrontRenderer::resetTemporal() { check(surf_temporal_reset(m_ctx), m_ctx, "surf_temporal_reset"); }

std::vector<U32> WaveFrontRenderer::displayRGBA8() {
    std::vector<U32> out((size_t)m_resolution.width * m_resolution.height);
    check(surf_display_rgba8(m_ctx, out.data()), m_ctx, "surf_display_rgba8");
    return out;
}

}  // namespace surf
