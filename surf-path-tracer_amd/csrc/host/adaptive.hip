/*
 * adaptive.hip -- per-pixel sample masks and the adaptive loop
 * (surf_set_pixel_mask, surf_mask_from_noise, surf_adaptive_mask_image*,
 * surf_render_adaptive; include/surf_hip.h): the mask's buffers on a context,
 * parameter checks, the launches that turn (A, Q) into the byte mask and its
 * ascending list, the CPU twin, and the adaptive loop on this mask.  The rule
 * lives in device/adaptive_kernels.h; the mask's buffers, the compaction's
 * launches, the twin's dilation and the loop itself in host/mask_host.h
 * (host/error_mask.hip builds masks too); what a
 * masked stream does with the list is the sample stream's business
 * (surf_hip.hip).
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/adaptive_kernels.h"
#include "host/mask_host.h"

namespace {

const char* maskParamError(const surf_adaptive_mask_params* p) {
    if (!p) return "mask params is NULL";
    if (!(std::isfinite(p->threshold) && p->threshold > 0.0f)) return "threshold is not finite and > 0";
    if (!(std::isfinite(p->floor) && p->floor > 0.0f)) return "floor is not finite and > 0";
    if (p->min_samples < 2) return "min_samples is below 2";
    if (p->max_samples < p->min_samples) return "max_samples is below min_samples";
    if (p->dilate > (uint32_t)kAdaptiveMaxDilate) return "dilate outside 0..2";
    return nullptr;
}

AdaptiveRule ruleOf(const surf_adaptive_mask_params& p) {
    return AdaptiveRule{p.threshold, p.floor, (float)p.min_samples, (float)p.max_samples, (int)p.dilate};
}

const char* frameError(uint32_t w, uint32_t h, const float* acc, const float* squares, const uint8_t* mask, const uint32_t* count) {
    if (!acc || !squares || !mask || !count) return "NULL argument";
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return "empty frame or too many pixels";
    return nullptr;
}

/* The byte mask of device planes of a w x h frame, then its ascending list;
 * the count is read back (one synchronisation). */
int runMask(surf_ctx* c, uint32_t w, uint32_t h, const float4* A, const float4* Q, const surf_adaptive_mask_params& P, uint8_t* mask,
            uint32_t* list, uint32_t* blk, uint32_t* count) {
    hipLaunchKernelGGL(k_adaptive_flags, tileGrid(w, h), dim3(256), 0, c->stream, A, Q, mask, (int)w, (int)h, ruleOf(P));
    queueSensorValidity(c, mask);
    return compactMask(c, w * h, mask, list, blk, count);
}

}  // namespace

void surfhost::freeAdaptive(surf_ctx* c) {
    for (void* p : {(void*)c->pmMask, (void*)c->pmList, (void*)c->pmBlk, (void*)c->adImgMask, (void*)c->adImgList, (void*)c->adImgBlk})
        if (p) (void)hipFree(p);
    c->pmMask = c->adImgMask = nullptr;
    c->pmList = c->pmBlk = c->adImgList = c->adImgBlk = nullptr;
    c->adImgCap = 0;
    c->pmOn = false;
}

int surfhost::resetSensorMask(surf_ctx* c) {
    c->pmOn = false;
    c->pmActive = 0;
    if (!sensorInvalid(c)) return SURF_OK;
    if (int rc = ensureContextMask(c)) return rc;
    std::vector<uint32_t> list;
    list.reserve(c->ssValid);
    for (uint32_t p = 0; p < c->npx; ++p)
        if (c->ssValidHost[p]) list.push_back(p);
    SURF_CHECK(c, hipMemcpyAsync(c->pmMask, c->ssValidHost.data(), c->npx, hipMemcpyHostToDevice, c->stream));
    if (!list.empty())
        SURF_CHECK(c, hipMemcpyAsync(c->pmList, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    c->pmOn = true;
    c->pmActive = c->ssValid;
    return SURF_OK;
}

extern "C" {

int surf_set_pixel_mask(surf_ctx* c, const uint8_t* mask) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_set_pixel_mask: ctx is NULL");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);                     /* a stream's pixels are fixed when it opens */
    if (rc) return rc;
    if (!mask) return resetSensorMask(c);
    const uint8_t* valid = sensorInvalid(c) ? c->ssValidHost.data() : nullptr;   /* a surfel sensor's invalid texels are never active */
    std::vector<uint8_t> bytes(c->npx);
    std::vector<uint32_t> list;
    list.reserve(c->npx);
    for (uint32_t p = 0; p < c->npx; ++p) {
        bytes[p] = mask[p] && (!valid || valid[p]) ? 1 : 0;
        if (bytes[p]) list.push_back(p);
    }
    if (list.size() == c->npx) { c->pmOn = false; c->pmActive = 0; return SURF_OK; }   /* all ones: no mask */
    if ((rc = ensureContextMask(c))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->pmMask, bytes.data(), c->npx, hipMemcpyHostToDevice, c->stream));
    if (!list.empty())
        SURF_CHECK(c, hipMemcpyAsync(c->pmList, list.data(), list.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    c->pmOn = true;
    c->pmActive = (uint32_t)list.size();
    return SURF_OK;
}

int surf_get_pixel_mask(surf_ctx* c, uint8_t* out, uint32_t* count) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_get_pixel_mask: ctx is NULL");
    if (count) *count = c->pmOn ? c->pmActive : c->npx;
    if (!out) return SURF_OK;
    if (!c->pmOn) { std::memset(out, 1, c->npx); return SURF_OK; }
    SURF_CHECK(c, hipSetDevice(c->device));
    /* (the mask's writers waited for their copies and kernels: nothing of it is pending on the render stream) */
    SURF_CHECK(c, hipMemcpy(out, c->pmMask, c->npx, hipMemcpyDeviceToHost));
    return SURF_OK;
}

int surf_adaptive_default_mask_params(surf_adaptive_mask_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->threshold = 0.05f;
    p->floor = 0.01f;
    p->min_samples = 16;
    p->max_samples = 1024;
    p->dilate = 1;
    return SURF_OK;
}

int surf_mask_from_noise(surf_ctx* c, const surf_adaptive_mask_params* p, uint32_t* count) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_mask_from_noise: ctx is NULL");
    if (const char* why = maskParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_mask_from_noise: ") + why);
    if (!c->sqOn) return fail(c, SURF_ERR_INVALID, "surf_mask_from_noise: sample squares are off (surf_set_sample_squares)");
    if (p->dilate > 0 && c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_mask_from_noise: a dilation needs the neighbouring rows, this context holds a row shard; "
                                         "assemble the planes and use surf_adaptive_mask_image, or pass dilate 0");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);
    if (rc) return rc;
    if ((rc = ensureContextMask(c))) return rc;
    uint32_t n = 0;
    /* (a shard with dilate 0: its rows as a frame of their own -- the rule is then pointwise) */
    if ((rc = runMask(c, c->width, (uint32_t)c->rows.size(), c->acc, c->sq, *p, c->pmMask, c->pmList, c->pmBlk, &n))) return rc;
    c->pmOn = n != c->npx;                     /* every pixel active: no mask */
    c->pmActive = c->pmOn ? n : 0u;
    if (count) *count = n;
    return SURF_OK;
}

int surf_adaptive_mask_image(surf_ctx* c, uint32_t w, uint32_t h, const float* acc, const float* squares,
                             const surf_adaptive_mask_params* p, uint8_t* maskOut, uint32_t* listOut, uint32_t* count) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_adaptive_mask_image: ctx is NULL");
    if (const char* why = frameError(w, h, acc, squares, maskOut, count)) return fail(c, SURF_ERR_INVALID, std::string("surf_adaptive_mask_image: ") + why);
    if (const char* why = maskParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_adaptive_mask_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h;
    int rc = c->sdAQ.grow(c, npx);
    if (rc) return rc;
    if ((rc = ensureImageMask(c, npx))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->sdAQ[0], acc, npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->sdAQ[1], squares, npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    uint32_t n = 0;
    if ((rc = runMask(c, w, h, c->sdAQ[0], c->sdAQ[1], *p, c->adImgMask, c->adImgList, c->adImgBlk, &n))) return rc;
    return copyImageMask(c, npx, n, maskOut, listOut, count);
}

/* The CPU twin: adaptiveRaw and adaptiveActive compiled for the host. */
int surf_adaptive_mask_image_host(uint32_t w, uint32_t h, const float* acc, const float* squares, const surf_adaptive_mask_params* p,
                                  uint8_t* maskOut, uint32_t* listOut, uint32_t* count) {
    if (const char* why = frameError(w, h, acc, squares, maskOut, count))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_adaptive_mask_image_host: ") + why);
    if (const char* why = maskParamError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_adaptive_mask_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const AdaptiveRule R = ruleOf(*p);
    const std::vector<float4> A = hostPlane(acc, npx), Q = hostPlane(squares, npx);
    std::vector<uint8_t> raw(npx);
    for (size_t q = 0; q < npx; ++q) raw[q] = adaptiveRaw(A[q], Q[q], R) ? 1 : 0;
    *count = dilateAndList(raw.data(), (int)w, (int)h, R.dilate, [&](size_t q, bool any) { return adaptiveActive(any, A[q], R); }, maskOut, listOut);
    return SURF_OK;
}

int surf_adaptive_default_params(surf_adaptive_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    surf_adaptive_default_mask_params(&p->mask);
    p->batch = 64;                 /* a round's drain costs what about 16 full frames do (MEASUREMENTS "Adaptive sampling") */
    return SURF_OK;
}

int surf_render_adaptive(surf_ctx* c, const surf_adaptive_params* p, uint32_t* roundActive, uint32_t roundCap, surf_adaptive_summary* sum) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_render_adaptive: ctx is NULL");
    if (!p || !sum) return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: NULL argument");
    if (const char* why = maskParamError(&p->mask)) return fail(c, SURF_ERR_INVALID, std::string("surf_render_adaptive: ") + why);
    if (const char* why = roundsParamError(*p)) return fail(c, SURF_ERR_INVALID, std::string("surf_render_adaptive: ") + why);
    if (!c->sqOn) return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: sample squares are off (surf_set_sample_squares)");
    int rc = startRounds(c, "surf_render_adaptive");
    if (rc) return rc;
    if (p->mask.dilate > 0 && c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: a dilation needs the neighbouring rows, this context holds a row shard");
    if ((rc = renderRounds(c, *p, roundActive, roundCap, sum, [&](uint32_t* active) { return surf_mask_from_noise(c, &p->mask, active); })))
        return rc;
    const surf_noise_params np{p->mask.threshold, p->mask.floor};
    return surf_noise_estimate(c, &np, nullptr, &sum->noise);
}

}  // extern "C"
