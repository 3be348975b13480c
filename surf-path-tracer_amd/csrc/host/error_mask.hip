/*
 * error_mask.hip -- the active-pixel mask from the non-local-means filter's
 * error estimate and the adaptive loop on it (surf_error_mask_image*,
 * surf_mask_from_nlm, surf_render_adaptive_nlm*; include/surf_hip.h):
 * parameter checks, the host constants, the mask launch in front of the
 * shared compaction, the CPU twin, and the adaptive loop (host/mask_host.h)
 * on the filter's context run (host/nlm.hip) and this mask.  The rule lives in
 * device/error_mask_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/error_mask_kernels.h"
#include "host/mask_host.h"

namespace {

const char* errorParamError(const surf_error_mask_params* p) {
    if (!p) return "mask params is NULL";
    if (!(std::isfinite(p->threshold) && p->threshold > 0.0f)) return "threshold is not finite and > 0";
    if (!(std::isfinite(p->floor) && p->floor > 0.0f)) return "floor is not finite and > 0";
    if (p->min_samples < 2) return "min_samples is below 2";
    if (p->max_samples < p->min_samples) return "max_samples is below min_samples";
    if (p->smooth > (uint32_t)kErrorMaxSmooth) return "smooth outside 0..3";
    if (p->dilate > (uint32_t)kErrorMaxDilate) return "dilate outside 0..2";
    return nullptr;
}

ErrorRule ruleOf(const surf_error_mask_params& p) {
    ErrorRule R;
    R.tt = p.threshold * p.threshold;
    R.ff = p.floor * p.floor;
    R.cnt = (float)((2 * p.smooth + 1) * (2 * p.smooth + 1));
    R.minSamples = (float)p.min_samples;
    R.maxSamples = (float)p.max_samples;
    R.smooth = (int)p.smooth;
    R.dilate = (int)p.dilate;
    return R;
}

const char* frameError(uint32_t w, uint32_t h, const float* out, const float* err, const float* acc, const uint8_t* mask,
                       const uint32_t* count) {
    if (!out || !err || !acc || !mask || !count) return "NULL argument";
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return "empty frame or too many pixels";
    return nullptr;
}

/* the summary's counters: the one record of c->em */
ErrorStats* emStats(surf_ctx* c) { return reinterpret_cast<ErrorStats*>(c->em[0]); }

/* The byte mask of device planes of a w x h frame, then its ascending list,
 * timed (c->emTime); the count is read back (one synchronisation).  stats:
 * the kernel also counts the summary into emStats(c), zeroed first. */
int runErrorMask(surf_ctx* c, uint32_t w, uint32_t h, const float4* out, const float4* err, const float4* A, const surf_error_mask_params& P,
                 bool stats, uint8_t* mask, uint32_t* list, uint32_t* blk, uint32_t* count) {
    const uint32_t npx = w * h;
    const ErrorRule R = ruleOf(P);
    int rc = c->em.grow(c, 1);
    if (rc) return rc;
    if (stats) SURF_CHECK(c, hipMemsetAsync(emStats(c), 0, sizeof(ErrorStats), c->stream));
    SURF_CHECK(c, c->emTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_error_mask, tileGrid(w, h), dim3(256), 0, c->stream, out, err, A, mask, (int)w, (int)h, R,
                       stats ? emStats(c) : (ErrorStats*)nullptr);
    SURF_CHECK(c, c->emTime.mark(1, c->stream));
    queueSensorValidity(c, mask);
    if ((rc = queueCompaction(c, npx, mask, list, blk))) return rc;
    SURF_CHECK(c, c->emTime.mark(2, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(count, blk + compactBlocks(npx), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    SURF_CHECK(c, c->emTime.collect(2));
    return SURF_OK;
}

/* surf_mask_from_nlm after its checks: the filter's context run, the mask from
 * its planes and the context's accumulator, set.  stats as runErrorMask's. */
int maskFromNlm(surf_ctx* c, const surf_nlm_params* np, const surf_error_mask_params* mp, const char* who, bool stats, uint32_t* count,
                const float4** out, const float4** err) {
    int rc = endStream(c);                     /* a stream's pixels are fixed when it opens */
    if (rc) return rc;
    if ((rc = nlmContextPlanes(c, np, who, out, err))) return rc;
    if ((rc = ensureContextMask(c))) return rc;
    uint32_t n = 0;
    if ((rc = runErrorMask(c, c->width, c->height, *out, *err, c->acc, *mp, stats, c->pmMask, c->pmList, c->pmBlk, &n))) return rc;
    c->pmOn = n != c->npx;                     /* every pixel active: no mask */
    c->pmActive = c->pmOn ? n : 0u;
    *count = n;
    return SURF_OK;
}

int adaptiveNlm(surf_ctx* c, const surf_adaptive_nlm_params* p, void* outImg, void* outErr, hipMemcpyKind kind, uint32_t* roundActive,
                uint32_t roundCap, surf_adaptive_nlm_summary* sum, const char* who) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, std::string(who) + ": ctx is NULL");
    if (!p || !sum) return fail(c, SURF_ERR_INVALID, std::string(who) + ": NULL argument");
    if (const char* why = errorParamError(&p->mask)) return fail(c, SURF_ERR_INVALID, std::string(who) + ": " + why);
    if (const char* why = nlmParamsError(&p->nlm)) return fail(c, SURF_ERR_INVALID, std::string(who) + ": nlm " + why);
    if (const char* why = roundsParamError(*p)) return fail(c, SURF_ERR_INVALID, std::string(who) + ": " + why);
    if (!c->bkM) return fail(c, SURF_ERR_INVALID, std::string(who) + ": sample buckets are off (surf_set_sample_buckets)");
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, std::string(who) + ": the filter and the mask need every row of the frame, this context holds a row shard");
    int rc = startRounds(c, who);
    if (rc) return rc;
    const float4 *dOut = nullptr, *dErr = nullptr;
    if ((rc = renderRounds(c, *p, roundActive, roundCap, sum,
                           [&](uint32_t* active) { return maskFromNlm(c, &p->nlm, &p->mask, who, true, active, &dOut, &dErr); })))
        return rc;
    /* the last filter run and mask are of the final state: its images and its counters */
    ErrorStats st{};
    const size_t bytes = (size_t)c->npx * sizeof(float4);
    SURF_CHECK(c, hipMemcpyAsync(&st, emStats(c), sizeof st, hipMemcpyDeviceToHost, c->stream));
    if (outImg) SURF_CHECK(c, hipMemcpyAsync(outImg, dOut, bytes, kind, c->stream));
    if (outErr) SURF_CHECK(c, hipMemcpyAsync(outErr, dErr, bytes, kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    sum->above = st.above;
    sum->max_error = st.maxKey ? errorFromKey(st.maxKey) : 0.0f;
    return SURF_OK;
}

}  // namespace

void surfhost::freeErrorMask(surf_ctx* c) {
    c->em.free();
    c->emIn.free();
    c->emTime.destroy();
}

extern "C" {

int surf_error_mask_default_params(surf_error_mask_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->threshold = 0.1f;
    p->floor = 0.01f;
    p->min_samples = 16;
    p->max_samples = 1024;
    p->smooth = 3;                 /* MEASUREMENTS "Error-driven adaptive sampling": the one radius that is ahead of uniform sampling at every threshold tried */
    p->dilate = 1;
    return SURF_OK;
}

int surf_error_mask_image(surf_ctx* c, uint32_t w, uint32_t h, const float* out, const float* err, const float* acc,
                          const surf_error_mask_params* p, uint8_t* maskOut, uint32_t* listOut, uint32_t* count) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_error_mask_image: ctx is NULL");
    if (const char* why = frameError(w, h, out, err, acc, maskOut, count)) return fail(c, SURF_ERR_INVALID, std::string("surf_error_mask_image: ") + why);
    if (const char* why = errorParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_error_mask_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->emIn.grow(c, npx);
    if (rc) return rc;
    if ((rc = ensureImageMask(c, npx))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->emIn[0], out, bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->emIn[1], err, bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->emIn[2], acc, bytes, hipMemcpyHostToDevice, c->stream));
    uint32_t n = 0;
    if ((rc = runErrorMask(c, w, h, c->emIn[0], c->emIn[1], c->emIn[2], *p, false, c->adImgMask, c->adImgList, c->adImgBlk, &n))) return rc;
    return copyImageMask(c, npx, n, maskOut, listOut, count);
}

/* The CPU twin: errorRel, errorBox, errorRaw and errorActive compiled for the host. */
int surf_error_mask_image_host(uint32_t w, uint32_t h, const float* out, const float* err, const float* acc, const surf_error_mask_params* p,
                               uint8_t* maskOut, uint32_t* listOut, uint32_t* count) {
    if (const char* why = frameError(w, h, out, err, acc, maskOut, count))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_error_mask_image_host: ") + why);
    if (const char* why = errorParamError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_error_mask_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const ErrorRule R = ruleOf(*p);
    const std::vector<float4> O = hostPlane(out, npx), E = hostPlane(err, npx), A = hostPlane(acc, npx);
    const int W = (int)w, H = (int)h;
    std::vector<float> rel(npx);
    for (size_t q = 0; q < npx; ++q) rel[q] = errorRel(O[q], E[q], R);
    std::vector<uint8_t> raw(npx);
    const auto at = [&](int x, int y) { return rel[(size_t)errorClamp(y, H) * W + errorClamp(x, W)]; };
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t q = (size_t)y * W + x;
            raw[q] = errorRaw(A[q].w, errorBox(x, y, R, at), R) ? 1 : 0;
        }
    *count = dilateAndList(raw.data(), W, H, R.dilate, [&](size_t q, bool any) { return errorActive(any, A[q].w, R); }, maskOut, listOut);
    return SURF_OK;
}

int surf_mask_from_nlm(surf_ctx* c, const surf_nlm_params* np, const surf_error_mask_params* mp, uint32_t* count) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_mask_from_nlm: ctx is NULL");
    if (const char* why = errorParamError(mp)) return fail(c, SURF_ERR_INVALID, std::string("surf_mask_from_nlm: ") + why);
    if (const char* why = nlmParamsError(np)) return fail(c, SURF_ERR_INVALID, std::string("surf_mask_from_nlm: nlm ") + why);
    if (!c->bkM) return fail(c, SURF_ERR_INVALID, "surf_mask_from_nlm: sample buckets are off (surf_set_sample_buckets)");
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_mask_from_nlm: the filter and the mask need every row of the frame, this context holds a row "
                                         "shard; assemble the planes and use surf_denoise_nlm_image and surf_error_mask_image");
    SURF_CHECK(c, hipSetDevice(c->device));
    uint32_t n = 0;
    const float4 *dOut = nullptr, *dErr = nullptr;
    if (int rc = maskFromNlm(c, np, mp, "surf_mask_from_nlm", false, &n, &dOut, &dErr)) return rc;
    if (count) *count = n;
    return SURF_OK;
}

int surf_debug_error_mask_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->emTime.read(kernel_ms, count);
    return SURF_OK;
}

int surf_adaptive_nlm_default_params(surf_adaptive_nlm_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    surf_error_mask_default_params(&p->mask);
    surf_nlm_default_params(&p->nlm);
    p->batch = 64;                 /* as surf_render_adaptive: a round's drain costs what about 16 full frames do */
    return SURF_OK;
}

int surf_render_adaptive_nlm(surf_ctx* c, const surf_adaptive_nlm_params* p, float* out, float* outErr, uint32_t* roundActive,
                             uint32_t roundCap, surf_adaptive_nlm_summary* sum) {
    return adaptiveNlm(c, p, out, outErr, hipMemcpyDeviceToHost, roundActive, roundCap, sum, "surf_render_adaptive_nlm");
}

int surf_render_adaptive_nlm_copy_device(surf_ctx* c, const surf_adaptive_nlm_params* p, void* dst, void* dstErr, uint32_t* roundActive,
                                         uint32_t roundCap, surf_adaptive_nlm_summary* sum) {
    return adaptiveNlm(c, p, dst, dstErr, hipMemcpyDeviceToDevice, roundActive, roundCap, sum, "surf_render_adaptive_nlm_copy_device");
}

}  // extern "C"
