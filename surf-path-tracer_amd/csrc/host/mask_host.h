/*
 * mask_host.h -- internal: what the two builders of an active-pixel mask
 * (host/adaptive.hip from the noise estimate, host/error_mask.hip from the
 * non-local-means filter's error estimate) share: the mask's three buffers on a
 * context or for an image call, and the launches that compact a byte mask into
 * its ascending list.  Include after the kernels (device/compact_kernels.h):
 * the launches are of the including translation unit's copies.
 */
#pragma once
#include "host/surf_ctx.h"

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

}  // namespace
