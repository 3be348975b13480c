/*
 * mask_host.h -- internal: what the two builders of an active-pixel mask
 * (host/adaptive.hip from the noise estimate, host/error_mask.hip from the
 * non-local-means filter's error estimate) share: the mask's three buffers on a
 * context or for an image call, the launches that compact a byte mask into
 * its ascending list, the image forms' copy-out, the CPU twins' dilation, and
 * the adaptive loop around surf_render, which is handed the mask's builder.
 * Include after the kernels (device/compact_kernels.h): the launches are of
 * the including translation unit's copies.
 */
#pragma once
#include "host/surf_ctx.h"

#include <algorithm>
#include <cstring>

#include "device/compact_kernels.h"

namespace {

uint32_t compactBlocks(size_t npx) { return (uint32_t)((npx + kCompactBlock - 1) / kCompactBlock); }

/* the three buffers of a mask of npx pixels: bytes, list, block counts + total */
int allocMask(surf_ctx* c, size_t npx, uint8_t** mask, uint32_t** list, uint32_t** blk) {
    const size_t nb = compactBlocks(npx);
    if (hipMalloc((void**)mask, npx) != hipSuccess || hipMalloc((void**)list, npx * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void**)blk, (nb + 1) * sizeof(uint32_t)) != hipSuccess) {
        (void)hipGetLastError();
        for (void* p : {(void*)*mask, (void*)*list, (void*)*blk})
            if (p) (void)hipFree(p);
        *mask = nullptr; *list = nullptr; *blk = nullptr;
        return fail(c, SURF_ERR_OOM, "hipMalloc of a pixel mask of " + std::to_string(npx) + " pixels failed");
    }
    return SURF_OK;
}

int ensureContextMask(surf_ctx* c) {
    if (c->pmMask) return SURF_OK;
    return allocMask(c, c->npx, &c->pmMask, &c->pmList, &c->pmBlk);
}

/* the image forms' buffers (c->adImg*), grown when a larger frame arrives */
int ensureImageMask(surf_ctx* c, size_t npx) {
    if (npx <= c->adImgCap) return SURF_OK;
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    for (void* q : {(void*)c->adImgMask, (void*)c->adImgList, (void*)c->adImgBlk})
        if (q) (void)hipFree(q);
    c->adImgMask = nullptr; c->adImgList = nullptr; c->adImgBlk = nullptr;
    c->adImgCap = 0;
    if (int rc = allocMask(c, npx, &c->adImgMask, &c->adImgList, &c->adImgBlk)) return rc;
    c->adImgCap = npx;
    return SURF_OK;
}

/* a surfel sensor with invalid texels is set: they are never active, whatever sets or builds the context's mask */
bool sensorInvalid(const surf_ctx* c) { return c->ssOn && c->ssValid < c->npx; }

/* ... so behind the kernel that wrote the context's mask (any other mask is an image call's: left as built) and before its
 * compaction, their bytes are forced to 0 */
void queueSensorValidity(surf_ctx* c, uint8_t* mask) {
    if (mask != c->pmMask || !sensorInvalid(c)) return;
    hipLaunchKernelGGL(k_mask_and_valid, dim3(compactBlocks(c->npx)), dim3(kCompactBlock), 0, c->stream, mask, (const uint8_t*)c->ssValidDev, c->npx);
}

/* The ascending list of a byte mask of npx pixels, queued behind the kernel
 * that writes the mask: count, scan, scatter. */
int queueCompaction(surf_ctx* c, uint32_t npx, const uint8_t* mask, uint32_t* list, uint32_t* blk) {
    const uint32_t nb = compactBlocks(npx);
    hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(kCompactBlock), 0, c->stream, mask, npx, blk);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, c->stream, blk, nb);
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(kCompactBlock), 0, c->stream, mask, npx, (const uint32_t*)blk, list);
    SURF_CHECK(c, hipGetLastError());
    return SURF_OK;
}

/* ... and the count read back (one synchronisation). */
int compactMask(surf_ctx* c, uint32_t npx, const uint8_t* mask, uint32_t* list, uint32_t* blk, uint32_t* count) {
    if (int rc = queueCompaction(c, npx, mask, list, blk)) return rc;
    SURF_CHECK(c, hipMemcpyAsync(count, blk + compactBlocks(npx), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* the end of an image form: the mask of npx pixels in c->adImgMask and the n entries of its list copied out */
int copyImageMask(surf_ctx* c, size_t npx, uint32_t n, uint8_t* maskOut, uint32_t* listOut, uint32_t* count) {
    SURF_CHECK(c, hipMemcpyAsync(maskOut, c->adImgMask, npx, hipMemcpyDeviceToHost, c->stream));
    if (listOut && n) SURF_CHECK(c, hipMemcpyAsync(listOut, c->adImgList, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    *count = n;
    return SURF_OK;
}

/* The CPU twins' second pass over a W x H plane of raw flags: pixel q is on
 * where active(q, any), any: a raw flag is set within d pixels of it in the
 * frame.  Writes the byte mask and, where asked for, its list; returns the count. */
template <class Active>
uint32_t dilateAndList(const uint8_t* raw, int W, int H, int d, const Active& active, uint8_t* maskOut, uint32_t* listOut) {
    uint32_t n = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            bool any = false;
            for (int qy = std::max(0, y - d); qy <= std::min(H - 1, y + d); ++qy)
                for (int qx = std::max(0, x - d); qx <= std::min(W - 1, x + d); ++qx) any = any || raw[(size_t)qy * W + qx] != 0;
            const size_t q = (size_t)y * W + x;
            const bool on = active(q, any);
            maskOut[q] = on ? 1 : 0;
            if (on) { if (listOut) listOut[n] = (uint32_t)q; ++n; }
        }
    return n;
}

/* The adaptive loop ("render until nothing is active") for parameters P with
 * batch, max_segments, first_sample_index and mask.min/max_samples and a
 * summary S with rounds, frames, active_last and samples, in three steps: an
 * entry point puts its own refusals between them, in its order.  What is wrong
 * with the loop's parameters, or NULL ... */
template <class P>
const char* roundsParamError(const P& p) {
    if (p.batch == 0) return "batch is 0";
    if ((uint64_t)p.first_sample_index + p.mask.max_samples > 0xffffffffull) return "first_sample_index + max_samples exceeds 32 bits";
    return nullptr;
}
/* ... the stream drained and the accumulator found empty ... */
int startRounds(surf_ctx* c, const std::string& who) {
    SURF_CHECK(c, hipSetDevice(c->device));
    if (int rc = drainStream(c)) return rc;
    if (c->totalSamples != 0) return fail(c, SURF_ERR_INVALID, who + ": the accumulator holds samples; call surf_clear_accumulator first");
    return SURF_OK;
}
/* ... and the rounds: min_samples frames of every pixel, then mask(&active),
 * which builds and sets the mask, and batches under it until nothing is active
 * or max_samples frames are rendered; roundActive[r], r < roundCap: the count
 * round r rendered with.  Zeroes *sum, fills the four fields. */
template <class P, class S, class Mask>
int renderRounds(surf_ctx* c, const P& p, uint32_t* roundActive, uint32_t roundCap, S* sum, const Mask& mask) {
    std::memset(sum, 0, sizeof *sum);
    const uint64_t before = c->stats.samples;
    int rc = surf_set_pixel_mask(c, nullptr);
    if (rc) return rc;
    if ((rc = surf_render(c, p.mask.min_samples, p.first_sample_index, p.max_segments, 1))) return rc;
    uint32_t f = p.mask.min_samples, active = 0;
    for (;;) {
        if ((rc = mask(&active))) return rc;
        if (active == 0 || f == p.mask.max_samples) break;
        const uint32_t nb = std::min(p.batch, p.mask.max_samples - f);
        if (roundActive && sum->rounds < roundCap) roundActive[sum->rounds] = active;
        if ((rc = surf_render(c, nb, p.first_sample_index + f, p.max_segments, 1))) return rc;
        f += nb;
        ++sum->rounds;
    }
    sum->frames = f;
    sum->active_last = active;
    sum->samples = c->stats.samples - before;
    return SURF_OK;
}

}  // namespace
