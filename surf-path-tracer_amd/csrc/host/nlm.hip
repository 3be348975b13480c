/*
 * nlm.hip -- the dual-buffer non-local-means filter for stills
 * (surf_denoise_nlm*, include/surf_hip.h): parameter checks, the host
 * constants, the halves, prepare and filter launches over the context's
 * buckets or over uploaded half planes, the choice between the staged and the
 * global filter kernel, and the CPU twin.  The arithmetic lives in
 * device/nlm_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/nlm_kernels.h"

namespace {

const char* nlmParamError(const surf_nlm_params* p) {
    if (!p) return "params is NULL";
    if (p->search_radius < 1 || p->search_radius > (uint32_t)kNlmMaxSearch) return "search_radius outside 1..10";
    if (p->patch_radius > (uint32_t)kNlmMaxPatch) return "patch_radius outside 0..3";
    if (!(std::isfinite(p->k) && p->k > 0.0f)) return "k is not finite and > 0";
    if (!(std::isfinite(p->alpha) && p->alpha >= 0.0f)) return "alpha is not finite and >= 0";
    if (!(std::isfinite(p->eps) && p->eps > 0.0f)) return "eps is not finite and > 0";
    return nullptr;
}

/* what is wrong with an image call's arguments, or NULL */
const char* nlmImageError(uint32_t w, uint32_t h, const float* half0, const float* half1, const surf_nlm_params* p, const float* out) {
    if (!half0 || !half1 || !out) return "NULL argument";
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 27)) return "empty or too large a frame";
    return nlmParamError(p);
}

NlmConsts nlmConsts(const surf_nlm_params& p) {
    NlmConsts K;
    K.r = (int)p.search_radius;
    K.f = (int)p.patch_radius;
    K.kk = p.k * p.k;
    K.alpha = p.alpha;
    K.eps = p.eps;
    K.cnt = (float)(3 * (2 * K.f + 1) * (2 * K.f + 1));
    return K;
}

/* the scratch images of c->nl */
enum { kH0, kH1, kC0, kC1, kV, kOut, kErr };

/* Prepare and filter on device half planes of a full w x h frame, timed
 * (c->nlTime stages 1 and 2; the caller marked event 0 and, after its halves
 * launch if it has one, event 1).  The results stay in c->nl[kOut] and
 * c->nl[kErr].  Waits. */
int runNlm(surf_ctx* c, uint32_t w, uint32_t h, const float4* H0, const float4* H1, const surf_nlm_params& P) {
    const NlmConsts K = nlmConsts(P);
    const dim3 grid = tileGrid(w, h);
    hipLaunchKernelGGL(k_nlm_prepare, grid, dim3(256), 0, c->stream, H0, H1, (int)w, (int)h, c->nl[kC0], c->nl[kC1], c->nl[kV]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->nlTime.mark(2, c->stream));
    const size_t lds = nlmLdsBytes(K.r, K.f);
    const bool staged = c->nlStaged && lds <= kNlmLdsMax;
    hipLaunchKernelGGL(staged ? k_nlm<true> : k_nlm<false>, grid, dim3(256), staged ? lds : 0, c->stream, (const float4*)c->nl[kC0],
                       (const float4*)c->nl[kC1], (const float4*)c->nl[kV], H0, H1, c->nl[kOut], c->nl[kErr], (int)w, (int)h, K);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->nlTime.mark(3, c->stream));
    SURF_CHECK(c, c->nlTime.collect(3));
    return SURF_OK;
}

int nlmContext(surf_ctx* c, const surf_nlm_params* p, void* out, void* outErr, hipMemcpyKind kind, const char* who) {
    if (!c || !out) return SURF_ERR_INVALID;
    const float4* dOut = nullptr;
    const float4* dErr = nullptr;
    int rc = nlmContextPlanes(c, p, who, &dOut, &dErr);
    if (rc) return rc;
    const size_t bytes = (size_t)c->npx * sizeof(float4);
    SURF_CHECK(c, hipMemcpyAsync(out, dOut, bytes, kind, c->stream));
    if (outErr) SURF_CHECK(c, hipMemcpyAsync(outErr, dErr, bytes, kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

}  // namespace

const char* surfhost::nlmParamsError(const surf_nlm_params* p) { return nlmParamError(p); }

int surfhost::nlmContextPlanes(surf_ctx* c, const surf_nlm_params* p, const char* who, const float4** out, const float4** err) {
    if (const char* why = nlmParamError(p)) return fail(c, SURF_ERR_INVALID, std::string(who) + ": " + why);
    if (!c->bkM) return fail(c, SURF_ERR_INVALID, std::string(who) + ": sample buckets are off (surf_set_sample_buckets)");
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, std::string(who) + " needs a context that owns every row of the frame: a patch reads its "
                                         "neighbours' rows; assemble the shards' bucket planes, sum their halves and call surf_denoise_nlm_image");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = drainStream(c);
    if (rc) return rc;
    if ((rc = c->nl.grow(c, c->npx))) return rc;
    SURF_CHECK(c, c->nlTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_nlm_halves, dim3((c->npx + 255) / 256), dim3(256), 0, c->stream, (const float4*)c->bk, c->bkM, c->npx, c->nl[kH0],
                       c->nl[kH1]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->nlTime.mark(1, c->stream));
    if ((rc = runNlm(c, c->width, c->height, c->nl[kH0], c->nl[kH1], *p))) return rc;
    *out = c->nl[kOut];
    *err = c->nl[kErr];
    return SURF_OK;
}

void surfhost::freeNlm(surf_ctx* c) {
    c->nl.free();
    c->nlTime.destroy();
}

extern "C" {

int surf_nlm_default_params(surf_nlm_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->search_radius = 5;
    p->patch_radius = 2;
    p->k = 0.45f;
    p->alpha = 1.0f;
    p->eps = 1e-10f;
    return SURF_OK;
}

int surf_denoise_nlm(surf_ctx* c, const surf_nlm_params* p, float* out, float* outErr) {
    return nlmContext(c, p, out, outErr, hipMemcpyDeviceToHost, "surf_denoise_nlm");
}

int surf_denoise_nlm_copy_device(surf_ctx* c, const surf_nlm_params* p, void* dst, void* dstErr) {
    return nlmContext(c, p, dst, dstErr, hipMemcpyDeviceToDevice, "surf_denoise_nlm_copy_device");
}

int surf_denoise_nlm_image(surf_ctx* c, uint32_t w, uint32_t h, const float* half0, const float* half1, const surf_nlm_params* p, float* out,
                           float* outErr) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = nlmImageError(w, h, half0, half1, p, out)) return fail(c, SURF_ERR_INVALID, std::string("surf_denoise_nlm_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->nl.grow(c, npx);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->nl[kH0], half0, bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->nl[kH1], half1, bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, c->nlTime.mark(0, c->stream));
    SURF_CHECK(c, c->nlTime.mark(1, c->stream));      /* no halves launch: stage 0 is empty */
    if ((rc = runNlm(c, w, h, c->nl[kH0], c->nl[kH1], *p))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, c->nl[kOut], bytes, hipMemcpyDeviceToHost, c->stream));
    if (outErr) SURF_CHECK(c, hipMemcpyAsync(outErr, c->nl[kErr], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* The CPU twin: nlmPrepare / nlmPixel / nlmOutput of device/nlm_kernels.h compiled for the host, on host arrays. */
int surf_denoise_nlm_image_host(uint32_t w, uint32_t h, const float* half0, const float* half1, const surf_nlm_params* p, float* out,
                                float* outErr) {
    if (const char* why = nlmImageError(w, h, half0, half1, p, out))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_nlm_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const std::vector<float4> H0 = hostPlane(half0, npx), H1 = hostPlane(half1, npx);
    std::vector<float4> C0(npx), C1(npx), V(npx);
    const NlmConsts K = nlmConsts(*p);
    const int W = (int)w, H = (int)h;
    const NlmFetchHalves halves{H0.data(), H1.data(), W};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t q = (size_t)y * w + x;
            nlmPrepare(x, y, W, H, halves, C0[q], C1[q], V[q]);
        }
    const NlmFetchPlanes fetch{C0.data(), C1.data(), V.data(), W};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t q = (size_t)y * w + x;
            const bool valid = C0[q].w != 0.0f;
            NlmSums s = nlmZero();
            if (valid) s = nlmPixel(x, y, W, H, K, fetch);
            float4 o, e;
            nlmOutput(valid, H0[q], H1[q], s, o, e);
            std::memcpy(out + 4 * q, &o, sizeof o);
            if (outErr) std::memcpy(outErr + 4 * q, &e, sizeof e);
        }
    return SURF_OK;
}

int surf_debug_nlm_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->nlTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
