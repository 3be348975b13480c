/*
 * render_baked.cpp -- the surfel sensor (surf_set_surfel_sensor, include/surf_hip.h)
 * on the indoor scene through the drop-in C++ API: scene and camera built as
 * render_indoor.cpp builds them, then two bakes of FRAMES one-sample frames each:
 *   (a) the view: the surfels are the camera's first-hit planes, handed over on
 *       the device (copyAOVDevice into two buffers of the application,
 *       setSurfelSensorDevice; no host trip) -- every pixel's picture is the
 *       light its first hit would gather were it white and diffuse;
 *   (b) a light map: WIDTH x HEIGHT upward-facing texels on the rectangle
 *       [X0, X1] x [Z0, Z1] of the plane y = Y (the floor is y = -1), texel
 *       (x, y) at (X0 + ((x + 0.5) / WIDTH) * (X1 - X0), Y, Z0 + ((y + 0.5) / HEIGHT) * (Z1 - Z0)),
 *       every step in f32.
 *
 * usage: render_baked ASSETS_DIR WIDTH HEIGHT FRAMES X0 Z0 X1 Z1 Y OUT_PREFIX
 * (ASSETS_DIR first, as every example here takes it.)  Writes OUT_PREFIX_view.pfm
 * and OUT_PREFIX_floor.pfm -- each texel's mean rgb / w, 0 where nothing was
 * traced, colour PFM through surf_write_pfm -- and the same two pictures as
 * .png through the display stage (surf_display_image, default parameters).
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

using namespace surf;

namespace {

/* the accumulator's mean image, written as PREFIX.pfm and, through the display stage, PREFIX.png; returns the traced texels */
size_t writeBake(WaveFrontRenderer& renderer, U32 W, U32 H, const std::string& prefix) {
    const std::vector<F32> acc = renderer.readAccumulator();
    std::vector<F32> mean(acc.size(), 0.0f);
    size_t traced = 0;
    for (size_t p = 0; p < (size_t)W * H; ++p) {
        const F32 w = acc[4 * p + 3];
        mean[4 * p + 3] = 1.0f;
        if (!(w > 0.0f)) continue;
        for (int k = 0; k < 3; ++k) mean[4 * p + k] = acc[4 * p + k] / w;
        ++traced;
    }
    const std::string pfm = prefix + ".pfm", png = prefix + ".png";
    if (surf_write_pfm(pfm.c_str(), W, H, mean.data()) != SURF_OK) throw std::runtime_error("cannot write " + pfm);
    surf_display_params dp;
    surf_display_default_params(&dp);
    std::vector<U32> words((size_t)W * H);
    surf_display_meter_result meter;
    if (surf_display_image(renderer.handle(), W, H, mean.data(), &dp, words.data(), &meter) != SURF_OK)
        throw std::runtime_error(std::string("surf_display_image: ") + surf_last_error(renderer.handle()));
    if (surf_write_png(png.c_str(), W, H, words.data()) != SURF_OK) throw std::runtime_error("cannot write " + png);
    return traced;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 11) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT FRAMES X0 Z0 X1 Z1 Y OUT_PREFIX\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[10];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), frames = std::atoi(argv[4]);
    if (w <= 0 || h <= 0 || frames <= 0) { std::fprintf(stderr, "render_baked: WIDTH, HEIGHT and FRAMES must be positive\n"); return 2; }
    const F32 x0 = std::strtof(argv[5], nullptr), z0 = std::strtof(argv[6], nullptr), x1 = std::strtof(argv[7], nullptr),
              z1 = std::strtof(argv[8], nullptr), y = std::strtof(argv[9], nullptr);
    const U32 W = (U32)w, H = (U32)h;
    const size_t npx = (size_t)W * H;
    void* dPlanes[2] = {nullptr, nullptr};
    int status = 0;
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        WaveFrontRenderer renderer(&context, nullptr, RendererConfig{}, FramebufferSize{W, H}, worldCam, *indoor.scene);

        /* (a) the view baked at its own first hits, device to device */
        for (void*& d : dPlanes)
            if (hipMalloc(&d, npx * 4 * sizeof(F32)) != hipSuccess) throw std::runtime_error("hipMalloc of a feature plane failed");
        renderer.copyAOVDevice(SURF_AOV_POSITION, dPlanes[0]);
        renderer.copyAOVDevice(SURF_AOV_NORMAL, dPlanes[1]);
        renderer.setSurfelSensorDevice(dPlanes[0], dPlanes[1]);
        U32 validView = 0;
        renderer.surfelSensor(&validView);
        renderer.clearAccumulator();
        for (int f = 0; f < frames; ++f) renderer.render(0.0f);
        const size_t tracedView = writeBake(renderer, W, H, prefix + "_view");

        /* (b) the light map of the rectangle */
        std::vector<F32> pos(npx * 4, 0.0f), nrm(npx * 4, 0.0f);
        for (U32 ty = 0; ty < H; ++ty)
            for (U32 tx = 0; tx < W; ++tx) {
                const size_t p = (size_t)ty * W + tx;
                pos[4 * p] = x0 + (((F32)tx + 0.5f) / (F32)W) * (x1 - x0);
                pos[4 * p + 1] = y;
                pos[4 * p + 2] = z0 + (((F32)ty + 0.5f) / (F32)H) * (z1 - z0);
                nrm[4 * p + 1] = 1.0f;
            }
        renderer.setSurfelSensor(pos, nrm);
        renderer.clearAccumulator();
        for (int f = 0; f < frames; ++f) renderer.render(0.0f);
        const size_t tracedFloor = writeBake(renderer, W, H, prefix + "_floor");
        renderer.clearSurfelSensor();
        std::printf("{\"width\": %u, \"height\": %u, \"frames\": %d, \"view_valid_texels\": %u, \"view_traced_texels\": %zu, "
                    "\"floor_traced_texels\": %zu}\n", W, H, frames, validView, tracedView, tracedFloor);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_baked: %s\n", e.what());
        status = 1;
    }
    for (void* d : dPlanes)
        if (d) (void)hipFree(d);
    return status;
}
