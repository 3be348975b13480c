/*
 * render_denoised.cpp -- one frame of a few samples per pixel of the indoor
 * scene and its denoised image, through the drop-in C++ API
 * (include/surf/surf_host.hpp): scene and camera built as render_indoor.cpp
 * builds them, one render() call of SPP samples, then
 * WaveFrontRenderer::denoise() with the default parameters (the
 * edge-avoiding a-trous filter on the first-hit feature buffers, surf_denoise).
 *
 * usage: render_denoised ASSETS_DIR WIDTH HEIGHT SPP PREFIX [ADAPTIVE_MAX]
 * Writes PREFIX_noisy.pfm (radiance sum over sample count) and
 * PREFIX_denoised.pfm (colour PFM, surf_write_pfm), and PREFIX_denoised.png:
 * the denoised image as the application would present it (surf_pack_rgba8
 * with the display gamma).  With SPP >= 2 also PREFIX_sampled.pfm: the same
 * accumulator through the sample-variance-guided filter
 * (WaveFrontRenderer::denoiseSampled, surf_denoise_sampled), for which the
 * render keeps the per-sample second moments (setSampleSquares); the other
 * outputs are what they are without it.  With ADAPTIVE_MAX >= 2 the
 * accumulator is then cleared and the frame rendered again until converged
 * (WaveFrontRenderer::renderAdaptive, surf_render_adaptive: the default
 * parameters with max_samples = ADAPTIVE_MAX and min_samples = min(16,
 * ADAPTIVE_MAX)): PREFIX_adaptive.pfm is each pixel's mean over its own
 * samples, PREFIX_counts.pfm its sample count in all three channels.
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc != 6 && argc != 7) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT SPP PREFIX [ADAPTIVE_MAX]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[5];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), spp = std::atoi(argv[4]);
    if (w <= 0 || h <= 0 || spp <= 0) { std::fprintf(stderr, "render_denoised: WIDTH, HEIGHT and SPP must be positive\n"); return 2; }
    const int adaptiveMax = argc == 7 ? std::atoi(argv[6]) : 0;
    if (argc == 7 && adaptiveMax < 2) { std::fprintf(stderr, "render_denoised: ADAPTIVE_MAX must be at least 2\n"); return 2; }
    const U32 W = (U32)w, H = (U32)h;
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        RendererConfig config;
        config.samplesPerFrame = (U32)spp;
        WaveFrontRenderer renderer(&context, nullptr, config, FramebufferSize{W, H}, worldCam, *indoor.scene);
        const bool sampled = spp >= 2;    /* one sample has no variance */
        if (sampled) renderer.setSampleSquares(true);
        renderer.render(0.0f);

        std::vector<F32> noisy = renderer.readAccumulator();
        for (size_t p = 0; p < (size_t)W * H; ++p) {
            const F32 inv = noisy[4 * p + 3] > 0.0f ? 1.0f / noisy[4 * p + 3] : 0.0f;
            for (int k = 0; k < 3; ++k) noisy[4 * p + k] = noisy[4 * p + k] * inv;
            noisy[4 * p + 3] = 1.0f;
        }
        const std::vector<F32> clean = renderer.denoise();
        std::vector<U32> rgba8((size_t)W * H);
        if (surf_pack_rgba8(clean.data(), W * H, 1.0f, 1, rgba8.data()) != SURF_OK) {
            std::fprintf(stderr, "render_denoised: surf_pack_rgba8 failed\n");
            return 1;
        }
        const std::string paths[3] = {prefix + "_noisy.pfm", prefix + "_denoised.pfm", prefix + "_denoised.png"};
        const int rc[3] = {surf_write_pfm(paths[0].c_str(), W, H, noisy.data()), surf_write_pfm(paths[1].c_str(), W, H, clean.data()),
                           surf_write_png(paths[2].c_str(), W, H, rgba8.data())};
        for (int k = 0; k < 3; ++k)
            if (rc[k] != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", paths[k].c_str()); return 1; }
        if (sampled) {
            const std::string path = prefix + "_sampled.pfm";
            const std::vector<F32> guided = renderer.denoiseSampled();
            if (surf_write_pfm(path.c_str(), W, H, guided.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
        if (adaptiveMax) {
            renderer.clearAccumulator();
            renderer.setSampleSquares(true);
            surf_adaptive_params ap;
            surf_adaptive_default_params(&ap);
            ap.mask.max_samples = (U32)adaptiveMax;
            ap.mask.min_samples = ap.mask.min_samples < ap.mask.max_samples ? ap.mask.min_samples : ap.mask.max_samples;
            const surf_adaptive_summary sum = renderer.renderAdaptive(ap);
            std::vector<F32> mean = renderer.readAccumulator(), counts(mean.size());
            for (size_t p = 0; p < (size_t)W * H; ++p) {
                const F32 n = mean[4 * p + 3], inv = n > 0.0f ? 1.0f / n : 0.0f;
                for (int k = 0; k < 3; ++k) { mean[4 * p + k] = mean[4 * p + k] * inv; counts[4 * p + k] = n; }
                mean[4 * p + 3] = counts[4 * p + 3] = 1.0f;
            }
            const std::string ap0 = prefix + "_adaptive.pfm", ap1 = prefix + "_counts.pfm";
            if (surf_write_pfm(ap0.c_str(), W, H, mean.data()) != SURF_OK || surf_write_pfm(ap1.c_str(), W, H, counts.data()) != SURF_OK) {
                std::fprintf(stderr, "cannot write %s or %s\n", ap0.c_str(), ap1.c_str());
                return 1;
            }
            std::printf("{\"adaptive_frames\": %u, \"adaptive_rounds\": %u, \"adaptive_samples\": %llu}\n", sum.frames, sum.rounds,
                        (unsigned long long)sum.samples);
        }
        std::printf("{\"width\": %u, \"height\": %u, \"spp\": %d}\n", W, H, spp);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_denoised: %s\n", e.what());
        return 1;
    }
    return 0;
}
