/*
 * render_aov.cpp -- the first-hit feature buffers (AOVs) of the indoor scene
 * through the drop-in C++ API (include/surf/surf_host.hpp): scene and camera
 * built as render_indoor.cpp builds them, then WaveFrontRenderer::readAOV /
 * readAOVIds instead of a render loop (no sample is rendered).
 *
 * usage: render_aov ASSETS_DIR WIDTH HEIGHT PREFIX
 * Writes PREFIX_position.pfm, PREFIX_normal.pfm and PREFIX_albedo.pfm (colour
 * PFM, surf_write_pfm: the planes' RGB, alpha dropped) and PREFIX_planes.bin:
 * the four raw planes in surf_aov order (position, normal, albedo, id), each
 * WIDTH*HEIGHT records of 16 bytes, rows top to bottom.
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT PREFIX\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[4];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    if (w <= 0 || h <= 0) { std::fprintf(stderr, "render_aov: WIDTH and HEIGHT must be positive\n"); return 2; }
    const U32 W = (U32)w, H = (U32)h;
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        WaveFrontRenderer renderer(&context, nullptr, RendererConfig{}, FramebufferSize{W, H}, worldCam, *indoor.scene);

        const char* names[3] = {"position", "normal", "albedo"};
        const surf_aov planes[3] = {SURF_AOV_POSITION, SURF_AOV_NORMAL, SURF_AOV_ALBEDO};
        const std::string binPath = prefix + "_planes.bin";
        FILE* bin = std::fopen(binPath.c_str(), "wb");
        if (!bin) { std::fprintf(stderr, "cannot write %s\n", binPath.c_str()); return 1; }
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            const std::vector<F32> plane = renderer.readAOV(planes[k]);
            const std::string path = prefix + "_" + names[k] + ".pfm";
            if (surf_write_pfm(path.c_str(), W, H, plane.data()) != SURF_OK) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                std::fclose(bin);
                return 1;
            }
            ok = ok && std::fwrite(plane.data(), sizeof(F32), plane.size(), bin) == plane.size();
        }
        const std::vector<U32> ids = renderer.readAOVIds();
        ok = ok && std::fwrite(ids.data(), sizeof(U32), ids.size(), bin) == ids.size();
        if (std::fclose(bin) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", binPath.c_str()); return 1; }
        size_t hits = 0;
        for (size_t p = 0; p < (size_t)W * H; ++p) hits += ids[4 * p] != 0xffffffffu;
        std::printf("{\"width\": %u, \"height\": %u, \"hit_pixels\": %zu}\n", W, H, hits);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_aov: %s\n", e.what());
        return 1;
    }
    return 0;
}
