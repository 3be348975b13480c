/*
 * adaptive.hip -- per-pixel sample masks and the adaptive loop
 * (surf_set_pixel_mask, surf_mask_from_noise, surf_adaptive_mask_image*,
 * surf_render_adaptive; include/surf_hip.h): the mask's buffers on a context,
 * parameter checks, the launches that turn (A, Q) into the byte mask and its
 * ascending list, the CPU twin, and the loop around surf_render.  The rule
 * lives in device/adaptive_kernels.h, the mask's buffers and the compaction's
 * launches in host/mask_host.h (host/error_mask.hip builds masks too); what a
 * masked stream does with the list is the sample stream's business
 * (surf_hip.hip).
 */
#include "host/surf_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstring>

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
    const dim3 tiles((w + kDenoiseTileW - 1) / kDenoiseTileW, (h + kDenoiseTileH - 1) / kDenoiseTileH);
    hipLaunchKernelGGL(k_adaptive_flags, tiles, dim3(256), 0, c->stream, A, Q, mask, (int)w, (int)h, ruleOf(P));
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

extern "C" {

int surf_set_pixel_mask(surf_ctx* c, const uint8_t* mask) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_set_pixel_mask: ctx is NULL");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);                     /* a stream's pixels are fixed when it opens */
    if (rc) return rc;
    if (!mask) { c->pmOn = false; c->pmActive = 0; return SURF_OK; }
    std::vector<uint8_t> bytes(c->npx);
    std::vector<uint32_t> list;
    list.reserve(c->npx);
    for (uint32_t p = 0; p < c->npx; ++p) {
        bytes[p] = mask[p] ? 1 : 0;
        if (mask[p]) list.push_back(p);
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
    SURF_CHECK(c, hipMemcpyAsync(maskOut, c->adImgMask, npx, hipMemcpyDeviceToHost, c->stream));
    if (listOut && n) SURF_CHECK(c, hipMemcpyAsync(listOut, c->adImgList, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    *count = n;
    return SURF_OK;
}

/* The CPU twin: adaptiveRaw and adaptiveActive compiled for the host. */
int surf_adaptive_mask_image_host(uint32_t w, uint32_t h, const float* acc, const float* squares, const surf_adaptive_mask_params* p,
                                  uint8_t* maskOut, uint32_t* listOut, uint32_t* count) {
    if (const char* why = frameError(w, h, acc, squares, maskOut, count))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_adaptive_mask_image_host: ") + why);
    if (const char* why = maskParamError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_adaptive_mask_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const AdaptiveRule R = ruleOf(*p);
    std::vector<float4> A(npx), Q(npx);                          /* the caller's planes need not be 16-byte aligned */
    std::memcpy(A.data(), acc, npx * sizeof(float4));
    std::memcpy(Q.data(), squares, npx * sizeof(float4));
    std::vector<uint8_t> raw(npx);
    for (size_t q = 0; q < npx; ++q) raw[q] = adaptiveRaw(A[q], Q[q], R) ? 1 : 0;
    uint32_t n = 0;
    const int d = R.dilate, W = (int)w, H = (int)h;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool any = false;
            for (int qy = std::max(0, y - d); qy <= std::min(H - 1, y + d); ++qy)
                for (int qx = std::max(0, x - d); qx <= std::min(W - 1, x + d); ++qx) any = any || raw[(size_t)qy * W + qx] != 0;
            const size_t q = (size_t)y * W + x;
            const bool on = adaptiveActive(any, A[q], R);
            maskOut[q] = on ? 1 : 0;
            if (on) { if (listOut) listOut[n] = (uint32_t)q; ++n; }
        }
    *count = n;
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
    if (p->batch == 0) return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: batch is 0");
    if ((uint64_t)p->first_sample_index + p->mask.max_samples > 0xffffffffull)
        return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: first_sample_index + max_samples exceeds 32 bits");
    if (!c->sqOn) return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: sample squares are off (surf_set_sample_squares)");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = drainStream(c);
    if (rc) return rc;
    if (c->totalSamples != 0)
        return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: the accumulator holds samples; call surf_clear_accumulator first");
    if (p->mask.dilate > 0 && c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_render_adaptive: a dilation needs the neighbouring rows, this context holds a row shard");
    std::memset(sum, 0, sizeof *sum);
    const uint64_t before = c->stats.samples;
    if ((rc = surf_set_pixel_mask(c, nullptr))) return rc;
    if ((rc = surf_render(c, p->mask.min_samples, p->first_sample_index, p->max_segments, 1))) return rc;
    uint32_t f = p->mask.min_samples, active = 0;
    for (;;) {
        if ((rc = surf_mask_from_noise(c, &p->mask, &active))) return rc;
        if (active == 0 || f == p->mask.max_samples) break;
        const uint32_t nb = std::min(p->batch, p->mask.max_samples - f);
        if (roundActive && sum->rounds < roundCap) roundActive[sum->rounds] = active;
        if ((rc = surf_render(c, nb, p->first_sample_index + f, p->max_segments, 1))) return rc;
        f += nb;
        ++sum->rounds;
    }
    sum->frames = f;
    sum->active_last = active;
    sum->samples = c->stats.samples - before;
    const surf_noise_params np{p->mask.threshold, p->mask.floor};
    return surf_noise_estimate(c, &np, nullptr, &sum->noise);
}

}  // extern "C"
