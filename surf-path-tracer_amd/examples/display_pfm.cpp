/*
 * display_pfm.cpp -- any colour PFM the other examples write (surf_write_pfm)
 * through the display stage on the GPU (surf_display_image, include/surf_hip.h):
 * metered exposure, optional bloom, tone curve, transfer function, dither.
 *
 * usage: display_pfm IN.pfm OUT.png [key=value ...]
 * The keys are surf_display_params' fields (exposure_mode, exposure, key,
 * min_scale, max_scale, bloom_radius, bloom_threshold, bloom_strength, curve,
 * white, transfer, dither); what is not given keeps its default
 * (surf_display_default_params).  Every pixel enters with weight 1.  Prints
 * the meter's result.
 */
#include "surf_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

/* a little-endian colour PFM (rows bottom to top) as RGBA rows top to bottom, w = 1 */
bool readPfm(const char* path, uint32_t& w, uint32_t& h, std::vector<float>& rgba) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    char magic[3] = {};
    float scale = 0.0f;
    bool ok = std::fscanf(f, "%2s %u %u %f", magic, &w, &h, &scale) == 4 && std::strcmp(magic, "PF") == 0 && scale < 0.0f && w && h &&
              (unsigned long long)w * h <= (1ull << 27) && std::fgetc(f) != EOF;
    if (ok) {
        std::vector<float> row(3 * (size_t)w);
        rgba.assign(4 * (size_t)w * h, 1.0f);
        for (uint32_t y = h; ok && y-- > 0;) {
            ok = std::fread(row.data(), sizeof(float), row.size(), f) == row.size();
            for (uint32_t x = 0; ok && x < w; ++x) std::memcpy(&rgba[4 * ((size_t)y * w + x)], &row[3 * (size_t)x], 3 * sizeof(float));
        }
    }
    std::fclose(f);
    return ok;
}

bool setField(surf_display_params& p, const std::string& key, const char* val) {
    const struct { const char* name; uint32_t* u; float* f; } fields[] = {
        {"exposure_mode", &p.exposure_mode, nullptr}, {"exposure", nullptr, &p.exposure}, {"key", nullptr, &p.key},
        {"min_scale", nullptr, &p.min_scale}, {"max_scale", nullptr, &p.max_scale}, {"bloom_radius", &p.bloom_radius, nullptr},
        {"bloom_threshold", nullptr, &p.bloom_threshold}, {"bloom_strength", nullptr, &p.bloom_strength}, {"curve", &p.curve, nullptr},
        {"white", nullptr, &p.white}, {"transfer", &p.transfer, nullptr}, {"dither", &p.dither, nullptr}};
    for (const auto& fd : fields)
        if (key == fd.name) {
            if (fd.u) *fd.u = (uint32_t)std::strtoul(val, nullptr, 10);
            else *fd.f = std::strtof(val, nullptr);
            return true;
        }
    return false;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s IN.pfm OUT.png [key=value ...]\n", argv[0]);
        return 2;
    }
    surf_display_params p;
    surf_display_default_params(&p);
    for (int k = 3; k < argc; ++k) {
        const char* eq = std::strchr(argv[k], '=');
        if (!eq || !setField(p, std::string((const char*)argv[k], eq), eq + 1)) {
            std::fprintf(stderr, "display_pfm: %s is not key=value with a field of surf_display_params\n", argv[k]);
            return 2;
        }
    }
    uint32_t w = 0, h = 0;
    std::vector<float> rgba;
    if (!readPfm(argv[1], w, h, rgba)) {
        std::fprintf(stderr, "display_pfm: %s is not a little-endian colour PFM\n", argv[1]);
        return 1;
    }
    surf_ctx* ctx = nullptr;
    int rc = surf_create(0, w, h, 0, h, &ctx);
    std::vector<uint32_t> words((size_t)w * h);
    surf_display_meter_result meter;
    if (rc == SURF_OK) rc = surf_display_image(ctx, w, h, rgba.data(), &p, words.data(), &meter);
    if (rc == SURF_OK) rc = surf_write_png(argv[2], w, h, words.data());
    if (rc != SURF_OK) {
        std::fprintf(stderr, "display_pfm: error %d: %s\n", rc, surf_last_error(ctx));
        if (ctx) surf_destroy(ctx);
        return 1;
    }
    std::printf("%u x %u: counted %u, black %u, median bin %u, scale %g -> %s\n", w, h, meter.counted, meter.black, meter.median_bin,
                (double)meter.scale, argv[2]);
    surf_destroy(ctx);
    return 0;
}
