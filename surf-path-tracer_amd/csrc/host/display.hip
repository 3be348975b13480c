/*
 * display.hip -- the display stage (surf_display*, include/surf_hip.h): from a
 * float RGBA image to RGBA8 words through a metered exposure, an optional
 * bloom, a tone curve, a transfer function and an ordered dither.  Parameter
 * checks, the host constants (the bloom's weights, the sRGB table), the
 * launches over the context's accumulator, an uploaded plane or a device
 * plane, the copies out, and the CPU twin.  The arithmetic lives in
 * device/display_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/display_kernels.h"

namespace {

static_assert(sizeof(surf_display_meter_result) == kDisplayRecordWords * sizeof(uint32_t), "the meter record is the result, word for word");

static_assert(kDisplayStripeWords >= (uint32_t)kDisplayRecordWords && kDisplayStripeWords % 4 == 0, "a copy holds the record");
/* c->dpRec in words: the meter record's copies (the first is the result) */
constexpr size_t kRecWords = (size_t)kDisplayStripes * kDisplayStripeWords;
constexpr uint32_t kMeterBlocks = 1024;      /* the meter's grid is capped: 4 blocks a CU, the rest by its stride loop */

const char* displayParamError(const surf_display_params* p) {
    if (!p) return "params is NULL";
    const auto pos = [](float v) { return std::isfinite(v) && v > 0.0f; };
    const auto nonneg = [](float v) { return std::isfinite(v) && v >= 0.0f; };
    if (p->exposure_mode > 1) return "exposure_mode is neither 0 nor 1";
    if (!pos(p->exposure)) return "exposure is not finite and > 0";
    if (!pos(p->key)) return "key is not finite and > 0";
    if (!pos(p->min_scale)) return "min_scale is not finite and > 0";
    if (!pos(p->max_scale)) return "max_scale is not finite and > 0";
    if (p->min_scale > p->max_scale) return "min_scale is above max_scale";
    if (p->bloom_radius > (uint32_t)kDisplayMaxBloom) return "bloom_radius outside 0..16";
    if (!nonneg(p->bloom_threshold)) return "bloom_threshold is not finite and >= 0";
    if (!nonneg(p->bloom_strength)) return "bloom_strength is not finite and >= 0";
    if (p->curve > 2) return "curve is none of 0, 1 and 2";
    if (!pos(p->white)) return "white is not finite and > 0";
    if (p->transfer > 2) return "transfer is none of 0, 1 and 2";
    if (p->dither > 1) return "dither is neither 0 nor 1";
    return nullptr;
}

/* the host constants of checked parameters (rule 5's weights among them; expf is the host's) */
DisplayConsts displayConsts(const surf_display_params& p) {
    DisplayConsts K{};
    K.R = (int)p.bloom_radius;
    K.curve = (int)p.curve;
    K.transfer = (int)p.transfer;
    K.dither = (int)p.dither;
    K.autoExposure = (int)p.exposure_mode;
    K.exposure = p.exposure;
    K.key = p.key;
    K.minScale = p.min_scale;
    K.maxScale = p.max_scale;
    K.threshold = p.bloom_threshold;
    K.strength = p.bloom_strength;
    K.ww = p.white * p.white;
    if (K.R > 0) {
        const float sigma = 0.5f * (float)K.R;
        float g[kDisplayMaxBloom + 1];
        for (int i = 0; i <= K.R; ++i) g[i] = expf(-(float)(i * i) / (2.0f * sigma * sigma));
        float S = g[0];
        for (int i = 1; i <= K.R; ++i) S = S + (g[i] + g[i]);
        for (int i = 0; i <= K.R; ++i) K.wn[i] = g[i] / S;
    }
    return K;
}

/* rule 7's table, computed once */
const float* srgbTable() {
    static const std::vector<float> T = [] {
        std::vector<float> t(kDisplayTable);
        for (int i = 0; i < kDisplayTable; ++i) {
            const double r = (double)i / 4095.0, l = r * r;
            t[i] = (float)(l <= 0.0031308 ? 12.92 * l : 1.055 * std::pow(l, 1.0 / 2.4) - 0.055);
        }
        return t;
    }();
    return T.data();
}

/* The stage on a device plane of a checked w x h frame: the record zeroed, the meter, the
 * scale, the blur where asked for, the pack into dst (device words); outHost: dst copied
 * there; the meter record copied to *meter.  Waits. */
int runDisplay(surf_ctx* c, uint32_t w, uint32_t h, const float4* A, const surf_display_params& p, uint32_t* dst, uint32_t* outHost,
               surf_display_meter_result* meter) {
    const size_t npx = (size_t)w * h;
    const DisplayConsts K = displayConsts(p);
    int rc = c->dpRec.grow(c, kRecWords / 4);
    if (rc) return rc;
    uint32_t* rec = reinterpret_cast<uint32_t*>(c->dpRec[0]);
    if (!c->dpTable) {                               /* the device's constant table, once per context; set only when the copy is queued */
        SURF_CHECK(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(kDisplaySrgb), srgbTable(), kDisplayTable * sizeof(float), 0, hipMemcpyHostToDevice,
                                             c->stream));
        c->dpTable = true;
    }
    if (K.R > 0 && (rc = c->dpHh.grow(c, npx))) return rc;
    StageTimer<4>& Tm = c->dpTime;
    SURF_CHECK(c, hipMemsetAsync(rec, 0, kRecWords * sizeof(uint32_t), c->stream));
    SURF_CHECK(c, Tm.mark(0, c->stream));
    const uint32_t blocks = (uint32_t)std::min<size_t>((npx + 255) / 256, kMeterBlocks);
    hipLaunchKernelGGL(k_display_meter, dim3(blocks), dim3(256), 0, c->stream, A, (uint32_t)npx, rec);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, Tm.mark(1, c->stream));
    hipLaunchKernelGGL(k_display_scale, dim3(1), dim3(64), 0, c->stream, rec, K);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, Tm.mark(2, c->stream));
    const dim3 grid = tileGrid(w, h);
    if (K.R > 0) {
        hipLaunchKernelGGL(k_display_blur_h, grid, dim3(256), 0, c->stream, A, (int)w, (int)h, (const uint32_t*)rec, c->dpHh[0], K);
        SURF_CHECK(c, hipGetLastError());
    }
    SURF_CHECK(c, Tm.mark(3, c->stream));
    if (K.R > 0)
        hipLaunchKernelGGL(k_display_blur_v_pack, grid, dim3(256), 0, c->stream, A, (const float4*)c->dpHh[0], (int)w, (int)h,
                           (const uint32_t*)rec, dst, K);
    else
        hipLaunchKernelGGL(k_display_pack, grid, dim3(256), 0, c->stream, A, (int)w, (int)h, (const uint32_t*)rec, dst, K);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, Tm.mark(4, c->stream));
    if (outHost) SURF_CHECK(c, hipMemcpyAsync(outHost, dst, npx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (meter) SURF_CHECK(c, hipMemcpyAsync(meter, rec, sizeof *meter, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    SURF_CHECK(c, Tm.collect(4));
    if (K.R == 0) Tm.ms[2] = 0.0f;                   /* no blur launch: the stage is empty */
    return SURF_OK;
}

/* the words of a form that copies to the host */
int displayWords(surf_ctx* c, size_t npx, uint32_t** dst) {
    const int rc = c->dpOut.grow(c, (npx + 3) / 4);
    *dst = reinterpret_cast<uint32_t*>(c->dpOut[0]);
    return rc;
}

}  // namespace

void surfhost::freeDisplay(surf_ctx* c) {
    c->dpRec.free();
    c->dpIn.free();
    c->dpHh.free();
    c->dpOut.free();
    c->dpTime.destroy();
}

extern "C" {

int surf_display_default_params(surf_display_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->exposure_mode = 1;
    p->exposure = 1.0f;
    p->key = 0.18f;
    p->min_scale = 1.0f / 64.0f;
    p->max_scale = 64.0f;
    p->bloom_radius = 0;
    p->bloom_threshold = 1.0f;
    p->bloom_strength = 0.1f;
    p->curve = 2;
    p->white = 4.0f;
    p->transfer = 2;
    p->dither = 1;
    return SURF_OK;
}

int surf_display(surf_ctx* c, const surf_display_params* p, uint32_t* out, surf_display_meter_result* meter) {
    if (!c || !out) return SURF_ERR_INVALID;
    const std::string who("surf_display");
    if (const char* why = displayParamError(p)) return fail(c, SURF_ERR_INVALID, who + ": " + why);
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, who + " needs a context that owns every row of the frame: the meter and the blur read the whole frame; "
                                         "assemble the shards' accumulators and call surf_display_image");
    if (c->totalSamples == 0) return fail(c, SURF_ERR_INVALID, who + ": nothing rendered since the last clear");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = drainStream(c);
    if (rc) return rc;
    uint32_t* dst = nullptr;
    if ((rc = displayWords(c, c->npx, &dst))) return rc;
    return runDisplay(c, c->width, c->height, c->acc, *p, dst, out, meter);
}

int surf_display_image(surf_ctx* c, uint32_t w, uint32_t h, const float* rgba, const surf_display_params* p, uint32_t* out,
                       surf_display_meter_result* meter) {
    if (!c) return SURF_ERR_INVALID;
    const char* why = !rgba || !out ? "NULL argument" : stillsImageError(w, h, displayParamError(p));
    if (why) return fail(c, SURF_ERR_INVALID, std::string("surf_display_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h;
    int rc = c->dpIn.grow(c, npx);
    if (rc) return rc;
    uint32_t* dst = nullptr;
    if ((rc = displayWords(c, npx, &dst))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->dpIn[0], rgba, npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return runDisplay(c, w, h, c->dpIn[0], *p, dst, out, meter);
}

int surf_display_image_device(surf_ctx* c, uint32_t w, uint32_t h, const void* src, const surf_display_params* p, void* dst,
                              surf_display_meter_result* meter) {
    if (!c) return SURF_ERR_INVALID;
    const char* why = !src || !dst ? "NULL argument" : stillsImageError(w, h, displayParamError(p));
    if (why) return fail(c, SURF_ERR_INVALID, std::string("surf_display_image_device: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    return runDisplay(c, w, h, static_cast<const float4*>(src), *p, static_cast<uint32_t*>(dst), nullptr, meter);
}

/* The CPU twin: the SURF_HD functions of device/display_kernels.h compiled for the host, on host arrays. */
int surf_display_image_host(uint32_t w, uint32_t h, const float* rgba, const surf_display_params* p, uint32_t* out,
                            surf_display_meter_result* meter) {
    const char* why = !rgba || !out ? "NULL argument" : stillsImageError(w, h, displayParamError(p));
    if (why) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_display_image_host: ") + why);
    const DisplayConsts K = displayConsts(*p);
    const size_t npx = (size_t)w * h;
    const std::vector<float4> A = hostPlane(rgba, npx);
    const int W = (int)w, H = (int)h;
    /* the meter and the scale */
    uint32_t rec[kDisplayRecordWords] = {};
    for (size_t q = 0; q < npx; ++q) ++rec[displayMeterWord(A[q])];
    uint64_t cum = 0;
    uint32_t counted = 0, m = (uint32_t)kDisplayBins;
    for (int k = 0; k < kDisplayBins; ++k) counted += rec[k];
    for (int k = 0; k < kDisplayBins && m == (uint32_t)kDisplayBins; ++k) {
        cum += rec[k];
        if (2 * cum >= (uint64_t)counted) m = (uint32_t)k;
    }
    const float scale = displayScale(K, m, counted);
    rec[kDisplayCounted] = counted;
    rec[kDisplayMedian] = m;
    rec[kDisplayScale] = f2u(scale);
    if (meter) std::memcpy(meter, rec, sizeof *meter);
    /* the bloom's two passes */
    const auto clampTo = [](int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); };
    std::vector<float4> Hh;
    if (K.R > 0) {
        std::vector<float4> B(npx);
        Hh.resize(npx);
        for (size_t q = 0; q < npx; ++q) B[q] = displayBright(A[q], scale, K.threshold);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x)
                Hh[(size_t)y * w + x] = displayBlur(K, [&](int i) { return B[(size_t)y * w + clampTo(x + i, W)]; });
    }
    const float* T = srgbTable();
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t q = (size_t)y * w + x;
            DisplayRgb v = displayExpose(displayColour(A[q]), scale);
            if (K.R > 0) v = displayAddBloom(v, K.strength, displayBlur(K, [&](int j) { return Hh[(size_t)clampTo(y + j, H) * w + x]; }));
            out[q] = displayPack(K, v, (uint32_t)x, (uint32_t)y, T);
        }
    return SURF_OK;
}

int surf_display_srgb_table(float out[4096]) {
    if (!out) return fail(nullptr, SURF_ERR_INVALID, "surf_display_srgb_table: NULL argument");
    std::memcpy(out, srgbTable(), kDisplayTable * sizeof(float));
    return SURF_OK;
}

int surf_display_bayer8(uint8_t out[64]) {
    if (!out) return fail(nullptr, SURF_ERR_INVALID, "surf_display_bayer8: NULL argument");
    for (uint32_t y = 0; y < 8; ++y)
        for (uint32_t x = 0; x < 8; ++x) out[8 * y + x] = (uint8_t)displayBayer8(x, y);
    return SURF_OK;
}

int surf_debug_display_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->dpTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
