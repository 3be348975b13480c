/*
 * render_lightmap.cpp -- a light map of the whole indoor scene with the library
 * alone (the light-map atlas, surf_atlas_*, include/surf_hip.h) through the
 * drop-in C++ API: scene built as render_indoor.cpp builds it, then
 *   1. grid charts over every instance (surf_atlas_grid_charts, 2 texels of
 *      margin), rasterized into one surfel per texel (buildAtlas);
 *   2. the surfels become the sensor, FRAMES one-sample frames are rendered;
 *   3. the accumulator is finished into the texture (finishAtlas) and its
 *      gutters are filled (dilateAtlas, 4 iterations).
 *
 * usage: render_lightmap ASSETS_DIR WIDTH HEIGHT FRAMES OUT_PREFIX
 * Prints the build's summary, warns when charts overlap, writes
 * OUT_PREFIX_lightmap.pfm (colour PFM through surf_write_pfm) and the same
 * picture as OUT_PREFIX_lightmap.png through the display stage
 * (surf_display_image, default parameters).
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT FRAMES OUT_PREFIX\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[5];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), frames = std::atoi(argv[4]);
    if (w <= 0 || h <= 0 || frames <= 0) { std::fprintf(stderr, "render_lightmap: WIDTH, HEIGHT and FRAMES must be positive\n"); return 2; }
    const U32 W = (U32)w, H = (U32)h, margin = 2, iterations = 4;
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        WaveFrontRenderer renderer(&context, nullptr, RendererConfig{}, FramebufferSize{W, H}, worldCam, *indoor.scene);

        const U32 n = indoor.scene->descriptor().instance_count;
        std::vector<surf_atlas_chart> charts(n);
        if (surf_atlas_grid_charts(n, nullptr, W, H, margin, charts.data()) != SURF_OK)
            throw std::runtime_error(std::string("surf_atlas_grid_charts: ") + surf_last_error(nullptr));
        const WaveFrontRenderer::AtlasPlanes atlas = renderer.buildAtlas(charts, W, H);
        const surf_atlas_summary& s = atlas.summary;
        if (s.overlapped > 0)
            std::fprintf(stderr, "render_lightmap: warning: %u texels are covered by more than one triangle: the UV layout overlaps "
                                 "(or shared edges pass through texel centres)\n", s.overlapped);

        renderer.setSurfelSensor(atlas.position, atlas.normal);
        U32 valid = 0;
        renderer.surfelSensor(&valid);
        renderer.clearAccumulator();
        for (int f = 0; f < frames; ++f) renderer.render(0.0f);
        const std::vector<F32> acc = renderer.readAccumulator();
        renderer.clearSurfelSensor();

        std::vector<uint8_t> lit;
        const std::vector<F32> finished = renderer.finishAtlas(W, H, acc, atlas.albedo, &lit);
        size_t litTexels = 0;
        for (const uint8_t v : lit) litTexels += v;
        const std::vector<F32> map = renderer.dilateAtlas(W, H, finished, lit, iterations);
        size_t filled = 0;
        for (const uint8_t v : lit) filled += v;

        const std::string pfm = prefix + "_lightmap.pfm", png = prefix + "_lightmap.png";
        if (surf_write_pfm(pfm.c_str(), W, H, map.data()) != SURF_OK) throw std::runtime_error("cannot write " + pfm);
        surf_display_params dp;
        surf_display_default_params(&dp);
        std::vector<U32> words((size_t)W * H);
        surf_display_meter_result meter;
        if (surf_display_image(renderer.handle(), W, H, map.data(), &dp, words.data(), &meter) != SURF_OK)
            throw std::runtime_error(std::string("surf_display_image: ") + surf_last_error(renderer.handle()));
        if (surf_write_png(png.c_str(), W, H, words.data()) != SURF_OK) throw std::runtime_error("cannot write " + png);
        std::printf("{\"width\": %u, \"height\": %u, \"frames\": %d, \"charts\": %u, \"triangles\": %u, \"skipped_triangles\": %u, "
                    "\"covered\": %u, \"overlapped\": %u, \"traced_texels\": %u, \"lit_texels\": %zu, \"texels_after_dilate\": %zu}\n",
                    W, H, frames, n, s.triangles, s.skipped_triangles, s.covered, s.overlapped, valid, litTexels, filled);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_lightmap: %s\n", e.what());
        return 1;
    }
    return 0;
}
