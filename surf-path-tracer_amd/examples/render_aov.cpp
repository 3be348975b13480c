/*
 * render_aov.cpp -- the first-hit feature buffers (AOVs) of the indoor scene
 * through the drop-in C++ API (include/surf/surf_host.hpp): scene and camera
 * built as render_indoor.cpp builds them, then WaveFrontRenderer::readAOV /
 * readAOVIds instead of a render loop (no sample is rendered).
 *
 * usage: render_aov ASSETS_DIR WIDTH HEIGHT PREFIX [MAX_LINKS [SAMPLES]]
 * Writes PREFIX_position.pfm, PREFIX_normal.pfm and PREFIX_albedo.pfm (colour
 * PFM, surf_write_pfm: the planes' RGB, alpha dropped) and PREFIX_planes.bin:
 * the four raw planes in surf_aov order (position, normal, albedo, id), each
 * WIDTH*HEIGHT records of 16 bytes, rows top to bottom.  With MAX_LINKS
 * (0..16) also the planes traced through mirrors and glass (readAOVChain /
 * readAOVChainIds), as PREFIX_chain_{position,normal,albedo}.pfm and
 * PREFIX_chain_planes.bin in the same layout.  With SAMPLES (1..64) also the
 * sampled planes of frames 0..SAMPLES-1 (readAOVSampled, instance keys), as
 * PREFIX_sampled_{position,normal,albedo}.pfm and PREFIX_matte.bin: the raw
 * matte key plane, then the raw matte count plane.
 */
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace surf;

int main(int argc, char** argv) {
    if (argc < 5 || argc > 7) {
        std::fprintf(stderr, "usage: %s ASSETS_DIR WIDTH HEIGHT PREFIX [MAX_LINKS [SAMPLES]]\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1], prefix = argv[4];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    if (w <= 0 || h <= 0) { std::fprintf(stderr, "render_aov: WIDTH and HEIGHT must be positive\n"); return 2; }
    const U32 W = (U32)w, H = (U32)h;
    const bool withChain = argc >= 6, withSampled = argc == 7;
    const int links = withChain ? std::atoi(argv[5]) : 0;
    if (links < 0 || links > SURF_AOV_CHAIN_MAX_LINKS) {
        std::fprintf(stderr, "render_aov: MAX_LINKS must be 0..%d\n", SURF_AOV_CHAIN_MAX_LINKS);
        return 2;
    }
    const U32 maxLinks = (U32)links;
    const int samples = withSampled ? std::atoi(argv[6]) : 1;
    if (samples < 1 || samples > SURF_AOVS_MAX_SAMPLES) {
        std::fprintf(stderr, "render_aov: SAMPLES must be 1..%d\n", SURF_AOVS_MAX_SAMPLES);
        return 2;
    }
    try {
        RenderContext context;            /* HIP device 0 */
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, dir);
        WaveFrontRenderer renderer(&context, nullptr, RendererConfig{}, FramebufferSize{W, H}, worldCam, *indoor.scene);

        /* one set of planes: three PFM images and the four raw planes behind each other */
        const auto writePlanes = [&](const std::string& stem, bool chain, std::vector<U32>& ids) {
            const char* names[3] = {"position", "normal", "albedo"};
            const surf_aov planes[3] = {SURF_AOV_POSITION, SURF_AOV_NORMAL, SURF_AOV_ALBEDO};
            const std::string binPath = stem + "_planes.bin";
            FILE* bin = std::fopen(binPath.c_str(), "wb");
            if (!bin) { std::fprintf(stderr, "cannot write %s\n", binPath.c_str()); return false; }
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                const std::vector<F32> plane = chain ? renderer.readAOVChain(planes[k], maxLinks) : renderer.readAOV(planes[k]);
                const std::string path = stem + "_" + names[k] + ".pfm";
                if (surf_write_pfm(path.c_str(), W, H, plane.data()) != SURF_OK) {
                    std::fprintf(stderr, "cannot write %s\n", path.c_str());
                    std::fclose(bin);
                    return false;
                }
                ok = ok && std::fwrite(plane.data(), sizeof(F32), plane.size(), bin) == plane.size();
            }
            ids = chain ? renderer.readAOVChainIds(maxLinks) : renderer.readAOVIds();
            ok = ok && std::fwrite(ids.data(), sizeof(U32), ids.size(), bin) == ids.size();
            if (std::fclose(bin) != 0 || !ok) { std::fprintf(stderr, "cannot write %s\n", binPath.c_str()); return false; }
            return true;
        };
        std::vector<U32> ids, chainIds;
        if (!writePlanes(prefix, false, ids)) return 1;
        if (withChain && !writePlanes(prefix + "_chain", true, chainIds)) return 1;
        if (withSampled) {
            surf_aov_sampled_params sp;
            surf_aov_sampled_default_params(&sp);
            sp.samples = (U32)samples;
            const char* names[3] = {"position", "normal", "albedo"};
            const surf_aovs planes[3] = {SURF_AOVS_POSITION, SURF_AOVS_NORMAL, SURF_AOVS_ALBEDO};
            for (int k = 0; k < 3; ++k) {
                const std::vector<F32> plane = renderer.readAOVSampled(planes[k], sp);
                const std::string path = prefix + "_sampled_" + names[k] + ".pfm";
                if (surf_write_pfm(path.c_str(), W, H, plane.data()) != SURF_OK) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
            }
            const std::string binPath = prefix + "_matte.bin";
            FILE* bin = std::fopen(binPath.c_str(), "wb");
            bool ok = bin != nullptr;
            for (const surf_aovs plane : {SURF_AOVS_MATTE_KEY, SURF_AOVS_MATTE_COUNT}) {
                const std::vector<U32> words = renderer.readAOVSampledIds(plane, sp);
                ok = ok && std::fwrite(words.data(), sizeof(U32), words.size(), bin) == words.size();
            }
            if (bin && std::fclose(bin) != 0) ok = false;
            if (!ok) { std::fprintf(stderr, "cannot write %s\n", binPath.c_str()); return 1; }
        }
        size_t hits = 0;
        for (size_t p = 0; p < (size_t)W * H; ++p) hits += ids[4 * p] != 0xffffffffu;
        if (withChain) {
            size_t linked = 0;
            for (size_t p = 0; p < (size_t)W * H; ++p) linked += chainIds[4 * p + 3] != 0u;
            std::printf("{\"width\": %u, \"height\": %u, \"hit_pixels\": %zu, \"max_links\": %u, \"chain_pixels\": %zu}\n", W, H, hits,
                        maxLinks, linked);
        } else
            std::printf("{\"width\": %u, \"height\": %u, \"hit_pixels\": %zu}\n", W, H, hits);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "render_aov: %s\n", e.what());
        return 1;
    }
    return 0;
}
