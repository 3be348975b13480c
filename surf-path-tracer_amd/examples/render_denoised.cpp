/*
 * render_denoised.cpp -- one frame of a few samples per pixel of the indoor
 * scene and its denoised image, through the drop-in C++ API
 * (include/surf/surf_host.hpp): scene and camera built as render_indoor.cpp
 * builds them, one render() call of SPP samples, then
 * WaveFrontRenderer::denoise() with the default parameters (the
 * edge-avoiding a-trous filter on the first-hit feature buffers, surf_denoise).
 *
 * usage: render_denoised ASSETS_DIR WIDTH HEIGHT SPP PREFIX
 * Writes PREFIX_noisy.pfm (radiance sum over sample count) and
 * PREFIX_denoised.pfm (colour PFM, surf_write_pfm), and PREFIX_denoised.png:
 * the denoised image as the application would present it (surf_pack_rgba8
 * with the display gamma).  With SPP >= 2 also PREFIX_sampled.pfm: the same
 * accumulator through the sample-variance-guided filter
 * (WaveFrontRenderer::denoiseSampled, surf_denoise_sampled), for which the
 * render keeps the per-sample second moments (setSampleSquares); the other
 * outputs are what they are without it.
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT SPP PREFIX\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[5];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), spp = std::atoi(argv[4]);
    if (w <= 0 || h <= 0 || spp <= 0) { std::fprintf(stderr, "render_denoised: WIDTH, HEIGHT and SPP must be positive\n"); return 2; }
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
        std::printf("{\"width\": %u, \"height\": %u, \"spp\": %d}\n", W, H, spp);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_denoised: %s\n", e.what());
        return 1;
    }
    return 0;
}
