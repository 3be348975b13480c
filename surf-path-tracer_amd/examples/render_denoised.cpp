/*
 * render_denoised.cpp -- one frame of a few samples per pixel of the indoor
 * scene and its denoised image, through the drop-in C++ API
 * (include/surf/surf_host.hpp): scene and camera built as render_indoor.cpp
 * builds them, one render() call of SPP samples, then
 * WaveFrontRenderer::denoise() with the default parameters (the
 * edge-avoiding a-trous filter on the first-hit feature buffers, surf_denoise).
 *
 * usage: render_denoised ASSETS_DIR WIDTH HEIGHT SPP PREFIX [ADAPTIVE_MAX [ROBUST_M [NLM]]]
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
 * With ROBUST_M (2, 4, 8 or 16; ADAPTIVE_MAX may then be 0 for "no adaptive
 * render") the render also keeps ROBUST_M sample buckets (setSampleBuckets)
 * and the median-of-means estimate of the accumulator
 * (WaveFrontRenderer::robust, surf_robust_accumulator) feeds the filters in the
 * accumulator's place, through their image forms (surf_denoise_image,
 * surf_denoise_sampled_image) with the renderer's feature buffers;
 * PREFIX_robust.pfm is that estimate's mean, PREFIX_noisy.pfm stays the plain
 * mean.  Wants about 32 samples per bucket.
 * With NLM nonzero and ROBUST_M set also PREFIX_nlm.pfm: the buckets' two half
 * images through the dual-buffer non-local-means filter
 * (WaveFrontRenderer::denoiseNlm, surf_denoise_nlm) with the default
 * parameters, which reads no feature buffer; every other output is what it is
 * without it.  With NLM = 2 the accumulator is at the end cleared once more
 * and the frame rendered until the FILTERED picture has converged
 * (WaveFrontRenderer::renderAdaptiveNlm, surf_render_adaptive_nlm: the default
 * parameters with max_samples = ADAPTIVE_MAX, or 4 * SPP without one, and
 * min_samples = min(16, max_samples)): PREFIX_nlm_adaptive.pfm is the filter's
 * image of the final state; every other output is what it is with NLM = 1.
 * With NLM = 3 also PREFIX_regress.pfm: the two half images and the first-hit
 * feature buffers through the first-order feature regression filter
 * (WaveFrontRenderer::denoiseRegress, surf_denoise_regress) with the default
 * parameters; every other output is what it is with NLM = 1.
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc < 6 || argc > 9) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT SPP PREFIX [ADAPTIVE_MAX [ROBUST_M [NLM]]]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[5];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), spp = std::atoi(argv[4]);
    if (w <= 0 || h <= 0 || spp <= 0) { std::fprintf(stderr, "render_denoised: WIDTH, HEIGHT and SPP must be positive\n"); return 2; }
    const int adaptiveMax = argc >= 7 ? std::atoi(argv[6]) : 0;
    if (argc >= 7 && adaptiveMax < 2 && !(argc >= 8 && adaptiveMax == 0)) {
        std::fprintf(stderr, "render_denoised: ADAPTIVE_MAX must be at least 2\n");
        return 2;
    }
    const int robustM = argc >= 8 ? std::atoi(argv[7]) : 0;
    if (argc >= 8 && robustM != 2 && robustM != 4 && robustM != 8 && robustM != 16) {
        std::fprintf(stderr, "render_denoised: ROBUST_M must be 2, 4, 8 or 16\n");
        return 2;
    }
    const bool nlm = argc == 9 && std::atoi(argv[8]) != 0;
    const bool nlmAdaptive = argc == 9 && std::atoi(argv[8]) == 2;
    const bool regress = argc == 9 && std::atoi(argv[8]) == 3;
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
        if (robustM) renderer.setSampleBuckets((U32)robustM);
        renderer.render(0.0f);

        std::vector<F32> noisy = renderer.readAccumulator();
        for (size_t p = 0; p < (size_t)W * H; ++p) {
            const F32 inv = noisy[4 * p + 3] > 0.0f ? 1.0f / noisy[4 * p + 3] : 0.0f;
            for (int k = 0; k < 3; ++k) noisy[4 * p + k] = noisy[4 * p + k] * inv;
            noisy[4 * p + 3] = 1.0f;
        }
        /* with ROBUST_M: the robust accumulator and the feature buffers the image forms of the filters take */
        std::vector<F32> robustAcc, planes[3];
        if (robustM) {
            robustAcc = renderer.robust();
            const int which[3] = {SURF_AOV_POSITION, SURF_AOV_NORMAL, SURF_AOV_ALBEDO};
            for (int k = 0; k < 3; ++k) {
                planes[k].resize((size_t)W * H * 4);
                if (surf_read_aov(renderer.handle(), which[k], planes[k].data()) != SURF_OK) {
                    std::fprintf(stderr, "render_denoised: surf_read_aov: %s\n", surf_last_error(renderer.handle()));
                    return 1;
                }
            }
            std::vector<F32> mean(robustAcc);
            for (size_t p = 0; p < (size_t)W * H; ++p) {
                const F32 inv = mean[4 * p + 3] > 0.0f ? 1.0f / mean[4 * p + 3] : 0.0f;
                for (int k = 0; k < 3; ++k) mean[4 * p + k] = mean[4 * p + k] * inv;
                mean[4 * p + 3] = 1.0f;
            }
            const std::string path = prefix + "_robust.pfm";
            if (surf_write_pfm(path.c_str(), W, H, mean.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
        if (robustM && nlm) {
            const std::vector<F32> patched = renderer.denoiseNlm();
            const std::string path = prefix + "_nlm.pfm";
            if (surf_write_pfm(path.c_str(), W, H, patched.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
        if (robustM && regress) {
            const std::vector<F32> fitted = renderer.denoiseRegress();
            const std::string path = prefix + "_regress.pfm";
            if (surf_write_pfm(path.c_str(), W, H, fitted.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        }
        std::vector<F32> clean;
        if (robustM) {
            surf_denoise_params dp;
            surf_denoise_default_params(&dp);
            clean.resize((size_t)W * H * 4);
            if (surf_denoise_image(renderer.handle(), W, H, robustAcc.data(), planes[0].data(), planes[1].data(), planes[2].data(), &dp,
                                   clean.data()) != SURF_OK) {
                std::fprintf(stderr, "render_denoised: surf_denoise_image: %s\n", surf_last_error(renderer.handle()));
                return 1;
            }
        } else {
            clean = renderer.denoise();
        }
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
            std::vector<F32> guided;
            if (robustM) {
                surf_svgf_params sp;
                surf_svgf_default_params(&sp);
                const std::vector<F32> squares = renderer.readSampleSquares();
                std::vector<F32> variance((size_t)W * H * 4);
                guided.resize((size_t)W * H * 4);
                if (surf_denoise_sampled_image(renderer.handle(), W, H, robustAcc.data(), squares.data(), planes[0].data(), planes[1].data(),
                                               planes[2].data(), &sp, guided.data(), variance.data()) != SURF_OK) {
                    std::fprintf(stderr, "render_denoised: surf_denoise_sampled_image: %s\n", surf_last_error(renderer.handle()));
                    return 1;
                }
            } else {
                guided = renderer.denoiseSampled();
            }
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
        if (robustM && nlmAdaptive) {
            renderer.clearAccumulator();
            surf_adaptive_nlm_params np;
            surf_adaptive_nlm_default_params(&np);
            np.mask.max_samples = adaptiveMax >= 2 ? (U32)adaptiveMax : 4u * (U32)spp;
            np.mask.min_samples = np.mask.min_samples < np.mask.max_samples ? np.mask.min_samples : np.mask.max_samples;
            if (np.mask.min_samples < 2) np.mask.min_samples = np.mask.max_samples = 2;
            std::vector<F32> image;
            const surf_adaptive_nlm_summary sum = renderer.renderAdaptiveNlm(np, &image);
            const std::string path = prefix + "_nlm_adaptive.pfm";
            if (surf_write_pfm(path.c_str(), W, H, image.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
            std::printf("{\"nlm_adaptive_frames\": %u, \"nlm_adaptive_rounds\": %u, \"nlm_adaptive_samples\": %llu, \"nlm_adaptive_above\": %llu}\n",
                        sum.frames, sum.rounds, (unsigned long long)sum.samples, (unsigned long long)sum.above);
        }
        std::printf("{\"width\": %u, \"height\": %u, \"spp\": %d}\n", W, H, spp);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_denoised: %s\n", e.what());
        return 1;
    }
    return 0;
}
