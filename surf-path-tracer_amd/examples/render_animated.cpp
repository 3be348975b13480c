/*
 * render_animated.cpp -- an animated sequence of the indoor scene at a few
 * samples per frame, through the drop-in C++ API (include/surf/surf_host.hpp)
 * and the temporal accumulation (surf_temporal_accumulate): FRAMES steps of
 * GPUScene::update(0.05f) (instance 3 rotates), each frame cleared, rendered
 * with SPP samples and blended with the reprojected result of the frames
 * before it; the last frame's blend also goes through the a-trous filter.
 *
 * usage: render_animated ASSETS_DIR WIDTH HEIGHT SPP FRAMES PREFIX
 * Writes, for the last frame, PREFIX_noisy.pfm (its own samples: radiance sum
 * over sample count), PREFIX_temporal.pfm (the blend),
 * PREFIX_temporal_denoised.pfm (the blend through the spatial filter) and
 * PREFIX_temporal_denoised.png, that image as the application would present
 * it (surf_pack_rgba8 with the display gamma); and PREFIX_svgf.pfm, the last
 * frame once more through the variance-guided filter (surf_svgf_accumulate)
 * on the state the loop left: the blend's history, no moments yet, so the
 * variance is the spatial estimate; and PREFIX_svgf_ex.pfm, that frame a
 * third time with the firefly clamp at scale 4 and the filtered-history
 * feedback (surf_svgf_accumulate_ex), on the state the call before left.
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT SPP FRAMES PREFIX\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[6];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), spp = std::atoi(argv[4]), frames = std::atoi(argv[5]);
    if (w <= 0 || h <= 0 || spp <= 0 || frames <= 0) {
        std::fprintf(stderr, "render_animated: WIDTH, HEIGHT, SPP and FRAMES must be positive\n");
        return 2;
    }
    const U32 W = (U32)w, H = (U32)h;
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        RendererConfig config;
        config.samplesPerFrame = (U32)spp;
        WaveFrontRenderer renderer(&context, nullptr, config, FramebufferSize{W, H}, worldCam, *indoor.scene);
        surf_temporal_params temporal;
        surf_denoise_params spatial;
        if (surf_temporal_default_params(&temporal) != SURF_OK || surf_denoise_default_params(&spatial) != SURF_OK) {
            std::fprintf(stderr, "render_animated: default parameters failed\n");
            return 1;
        }
        std::vector<F32> clean;
        for (int k = 0; k < frames; ++k) {
            indoor.scene->update(0.05f);
            renderer.clearAccumulatorKeepSeed();
            renderer.render(0.05f);
            const bool last = k + 1 == frames;
            clean = renderer.temporal(temporal, last ? &spatial : nullptr);
        }
        std::vector<F32> noisy = renderer.readAccumulator();
        for (size_t p = 0; p < (size_t)W * H; ++p) {
            const F32 inv = noisy[4 * p + 3] > 0.0f ? 1.0f / noisy[4 * p + 3] : 0.0f;
            for (int k = 0; k < 3; ++k) noisy[4 * p + k] = noisy[4 * p + k] * inv;
            noisy[4 * p + 3] = 1.0f;
        }
        std::vector<F32> blend((size_t)W * H * 4);       /* the stored history: the unfiltered blend (its w, the history length, is not written) */
        if (surf_temporal_history(renderer.handle(), blend.data()) != SURF_OK) {
            std::fprintf(stderr, "render_animated: %s\n", surf_last_error(renderer.handle()));
            return 1;
        }
        const std::vector<F32> guided = renderer.svgf();  /* after the history was read: the call stores its own */
        surf_svgf_params filter;
        surf_svgf_ext ext;
        if (surf_svgf_default_params(&filter) != SURF_OK || surf_svgf_default_ext(&ext) != SURF_OK) {
            std::fprintf(stderr, "render_animated: default parameters failed\n");
            return 1;
        }
        ext.firefly_scale = 4.0f;
        ext.feedback = 1;
        const std::vector<F32> guidedEx = renderer.svgf(temporal, filter, ext);
        std::vector<U32> rgba8((size_t)W * H);
        if (surf_pack_rgba8(clean.data(), W * H, 1.0f, 1, rgba8.data()) != SURF_OK) {
            std::fprintf(stderr, "render_animated: surf_pack_rgba8 failed\n");
            return 1;
        }
        const std::string paths[4] = {prefix + "_noisy.pfm", prefix + "_temporal.pfm", prefix + "_temporal_denoised.pfm",
                                      prefix + "_temporal_denoised.png"};
        const int rc[4] = {surf_write_pfm(paths[0].c_str(), W, H, noisy.data()), surf_write_pfm(paths[1].c_str(), W, H, blend.data()),
                           surf_write_pfm(paths[2].c_str(), W, H, clean.data()), surf_write_png(paths[3].c_str(), W, H, rgba8.data())};
        if (surf_write_pfm((prefix + "_svgf.pfm").c_str(), W, H, guided.data()) != SURF_OK) {
            std::fprintf(stderr, "cannot write %s_svgf.pfm\n", prefix.c_str());
            return 1;
        }
        if (surf_write_pfm((prefix + "_svgf_ex.pfm").c_str(), W, H, guidedEx.data()) != SURF_OK) {
            std::fprintf(stderr, "cannot write %s_svgf_ex.pfm\n", prefix.c_str());
            return 1;
        }
        for (int k = 0; k < 4; ++k)
            if (rc[k] != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", paths[k].c_str()); return 1; }
        std::printf("{\"width\": %u, \"height\": %u, \"spp\": %d, \"frames\": %d}\n", W, H, spp, frames);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_animated: %s\n", e.what());
        return 1;
    }
    return 0;
}
