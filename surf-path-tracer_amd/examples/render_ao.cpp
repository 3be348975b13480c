/*
 * render_ao.cpp -- ray-traced ambient occlusion and bent normals of the indoor
 * scene through the drop-in C++ API (include/surf/surf_host.hpp): scene and
 * camera built as render_indoor.cpp builds them, then WaveFrontRenderer::readAO
 * instead of a render loop (no sample is rendered).
 *
 * usage: render_ao ASSETS_DIR WIDTH HEIGHT SAMPLES RADIUS OUT_PREFIX
 * (ASSETS_DIR first, as every example here takes it.)  SAMPLES is 1, 2, 4, 8,
 * 16, 32 or 64; RADIUS the rays' length.  Writes OUT_PREFIX_open.pfm (the
 * unoccluded share as grey) and OUT_PREFIX_bent.pfm (the bent normal's xyz),
 * colour PFM through surf_write_pfm, from the first-hit planes.
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
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT SAMPLES RADIUS OUT_PREFIX\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[6];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), samples = std::atoi(argv[4]);
    const float radius = (float)std::atof(argv[5]);
    if (w <= 0 || h <= 0) { std::fprintf(stderr, "render_ao: WIDTH and HEIGHT must be positive\n"); return 2; }
    if (samples < 1 || samples > SURF_AO_MAX_SAMPLES || (samples & (samples - 1)) != 0) {
        std::fprintf(stderr, "render_ao: SAMPLES must be a power of two in 1..%d\n", SURF_AO_MAX_SAMPLES);
        return 2;
    }
    if (!(radius > 0.0f)) { std::fprintf(stderr, "render_ao: RADIUS must be above 0\n"); return 2; }
    const U32 W = (U32)w, H = (U32)h;
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        WaveFrontRenderer renderer(&context, nullptr, RendererConfig{}, FramebufferSize{W, H}, worldCam, *indoor.scene);
        surf_ao_params q;
        surf_ao_default_params(&q);
        q.samples = (U32)samples;
        q.radius = radius;
        const std::vector<F32> open = renderer.readAO(q);
        const std::vector<U32> bits = renderer.readAOBits(q);
        std::vector<F32> grey(open.size());
        double sum = 0.0;
        size_t valid = 0;
        for (size_t p = 0; p < (size_t)W * H; ++p) {
            grey[4 * p] = grey[4 * p + 1] = grey[4 * p + 2] = open[4 * p + 3];
            grey[4 * p + 3] = 1.0f;
            if (bits[4 * p + 3]) { sum += open[4 * p + 3]; ++valid; }
        }
        const std::string openPath = prefix + "_open.pfm", bentPath = prefix + "_bent.pfm";
        if (surf_write_pfm(openPath.c_str(), W, H, grey.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", openPath.c_str()); return 1; }
        if (surf_write_pfm(bentPath.c_str(), W, H, open.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", bentPath.c_str()); return 1; }
        std::printf("{\"width\": %u, \"height\": %u, \"samples\": %d, \"radius\": %g, \"valid_pixels\": %zu, \"mean_openness\": %.6f}\n", W, H, samples,
                    (double)radius, valid, valid ? sum / (double)valid : 1.0);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_ao: %s\n", e.what());
        return 1;
    }
    return 0;
}
