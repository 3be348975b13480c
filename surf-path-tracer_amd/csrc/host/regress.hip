/*
 * regress.hip -- the first-order feature regression filter for stills
 * (surf_denoise_regress*, include/surf_hip.h): parameter checks, the host
 * constants, the halves, prepare and filter launches over the context's
 * buckets and guide planes or over uploaded planes, the choice between the
 * staged and the global filter kernel, and the CPU twin.  The arithmetic lives
 * in device/regress_kernels.h and, for what the non-local-means filter shares
 * with it, in device/nlm_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/regress_kernels.h"

namespace {

const char* regressParamError(const surf_regress_params* p) {
    if (!p) return "params is NULL";
    const surf_nlm_params weights{p->search_radius, p->patch_radius, p->k, p->alpha, p->eps, 0};     /* they mean what they mean there */
    if (const char* why = nlmParamsError(&weights)) return why;
    if (!(std::isfinite(p->ridge) && p->ridge > 0.0f)) return "ridge is not finite and > 0";
    return nullptr;
}

/* what is wrong with an image call's arguments, or NULL */
const char* regressImageError(uint32_t w, uint32_t h, const float* half0, const float* half1, const float* position, const float* normal,
                              const float* albedo, const surf_regress_params* p, const float* out) {
    if (!half0 || !half1 || !position || !normal || !albedo || !out) return "NULL argument";
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 27)) return "empty or too large a frame";
    return regressParamError(p);
}

RegressConsts regressConsts(const surf_regress_params& p) {
    RegressConsts R;
    R.n.r = (int)p.search_radius;
    R.n.f = (int)p.patch_radius;
    R.n.kk = p.k * p.k;
    R.n.alpha = p.alpha;
    R.n.eps = p.eps;
    R.n.cnt = (float)(3 * (2 * R.n.f + 1) * (2 * R.n.f + 1));
    R.ridge = p.ridge;
    return R;
}

/* the scratch images of c->rg; the last three hold the planes the image form uploads */
enum { kH0, kH1, kC0, kC1, kV, kOut, kErr, kPos, kNrm, kAlb };

/* Prepare and filter on device half planes and feature planes of a full w x h
 * frame, timed (c->rgTime stages 1 and 2; the caller marked event 0 and, after
 * its halves launch if it has one, event 1).  The results stay in c->rg[kOut]
 * and c->rg[kErr].  Waits. */
int runRegress(surf_ctx* c, uint32_t w, uint32_t h, const float4* H0, const float4* H1, const float4* pos, const float4* nrm,
               const float4* alb, const surf_regress_params& P) {
    const RegressConsts R = regressConsts(P);
    const dim3 grid = tileGrid(w, h);
    hipLaunchKernelGGL(k_nlm_prepare, grid, dim3(256), 0, c->stream, H0, H1, (int)w, (int)h, c->rg[kC0], c->rg[kC1], c->rg[kV]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->rgTime.mark(2, c->stream));
    const size_t lds = regressLdsBytes(R.n.r, R.n.f);
    const bool staged = c->rgStaged && lds <= kRegressLdsMax;
    if (staged && !c->rgLdsSet) {             /* announce that launches will ask for more than 64 KiB of dynamic LDS */
        SURF_CHECK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_regress<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)kRegressLdsMax));
        c->rgLdsSet = true;
    }
    hipLaunchKernelGGL(staged ? k_regress<true> : k_regress<false>, grid, dim3(256), staged ? lds : 0, c->stream, (const float4*)c->rg[kC0],
                       (const float4*)c->rg[kC1], (const float4*)c->rg[kV], H0, H1, pos, nrm, alb, c->rg[kOut], c->rg[kErr], (int)w, (int)h,
                       R);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->rgTime.mark(3, c->stream));
    SURF_CHECK(c, c->rgTime.collect(3));
    return SURF_OK;
}

int regressContext(surf_ctx* c, const surf_regress_params* p, void* out, void* outErr, hipMemcpyKind kind, const char* who) {
    if (!c || !out) return SURF_ERR_INVALID;
    if (const char* why = regressParamError(p)) return fail(c, SURF_ERR_INVALID, std::string(who) + ": " + why);
    if (!c->bkM) return fail(c, SURF_ERR_INVALID, std::string(who) + ": sample buckets are off (surf_set_sample_buckets)");
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, std::string(who) + " needs a context that owns every row of the frame: a patch reads its "
                                         "neighbours' rows; assemble the shards' bucket planes and feature planes, sum the halves and "
                                         "call surf_denoise_regress_image");
    SURF_CHECK(c, hipSetDevice(c->device));
    void* const* g = nullptr;     /* the first-hit planes, or the chain's (surf_set_filter_guides) */
    int rc = guidePlanes(c, &g);
    if (rc) return rc;
    if ((rc = drainStream(c))) return rc;
    if ((rc = c->rg.grow(c, c->npx))) return rc;
    SURF_CHECK(c, c->rgTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_nlm_halves, dim3((c->npx + 255) / 256), dim3(256), 0, c->stream, (const float4*)c->bk, c->bkM, c->npx, c->rg[kH0],
                       c->rg[kH1]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->rgTime.mark(1, c->stream));
    if ((rc = runRegress(c, c->width, c->height, c->rg[kH0], c->rg[kH1], static_cast<const float4*>(g[SURF_AOV_POSITION]),
                         static_cast<const float4*>(g[SURF_AOV_NORMAL]), static_cast<const float4*>(g[SURF_AOV_ALBEDO]), *p)))
        return rc;
    const size_t bytes = (size_t)c->npx * sizeof(float4);
    SURF_CHECK(c, hipMemcpyAsync(out, c->rg[kOut], bytes, kind, c->stream));
    if (outErr) SURF_CHECK(c, hipMemcpyAsync(outErr, c->rg[kErr], bytes, kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

}  // namespace

void surfhost::freeRegress(surf_ctx* c) {
    c->rg.free();
    c->rgTime.destroy();
}

extern "C" {

int surf_regress_default_params(surf_regress_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->search_radius = 5;
    p->patch_radius = 2;
    p->k = 0.7f;
    p->alpha = 1.0f;
    p->eps = 1e-10f;
    p->ridge = 0.1f;
    return SURF_OK;
}

int surf_denoise_regress(surf_ctx* c, const surf_regress_params* p, float* out, float* outErr) {
    return regressContext(c, p, out, outErr, hipMemcpyDeviceToHost, "surf_denoise_regress");
}

int surf_denoise_regress_copy_device(surf_ctx* c, const surf_regress_params* p, void* dst, void* dstErr) {
    return regressContext(c, p, dst, dstErr, hipMemcpyDeviceToDevice, "surf_denoise_regress_copy_device");
}

int surf_denoise_regress_image(surf_ctx* c, uint32_t w, uint32_t h, const float* half0, const float* half1, const float* position,
                               const float* normal, const float* albedo, const surf_regress_params* p, float* out, float* outErr) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = regressImageError(w, h, half0, half1, position, normal, albedo, p, out))
        return fail(c, SURF_ERR_INVALID, std::string("surf_denoise_regress_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->rg.grow(c, npx);
    if (rc) return rc;
    const float* src[5] = {half0, half1, position, normal, albedo};
    const int dst[5] = {kH0, kH1, kPos, kNrm, kAlb};
    for (int k = 0; k < 5; ++k) SURF_CHECK(c, hipMemcpyAsync(c->rg[dst[k]], src[k], bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, c->rgTime.mark(0, c->stream));
    SURF_CHECK(c, c->rgTime.mark(1, c->stream));      /* no halves launch: stage 0 is empty */
    if ((rc = runRegress(c, w, h, c->rg[kH0], c->rg[kH1], c->rg[kPos], c->rg[kNrm], c->rg[kAlb], *p))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, c->rg[kOut], bytes, hipMemcpyDeviceToHost, c->stream));
    if (outErr) SURF_CHECK(c, hipMemcpyAsync(outErr, c->rg[kErr], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* The CPU twin: nlmPrepare of device/nlm_kernels.h, regressPixel of device/regress_kernels.h and nlmOutput compiled
 * for the host, on host arrays. */
int surf_denoise_regress_image_host(uint32_t w, uint32_t h, const float* half0, const float* half1, const float* position,
                                    const float* normal, const float* albedo, const surf_regress_params* p, float* out, float* outErr) {
    if (const char* why = regressImageError(w, h, half0, half1, position, normal, albedo, p, out))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_regress_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const std::vector<float4> H0 = hostPlane(half0, npx), H1 = hostPlane(half1, npx);
    const std::vector<float4> Ps = hostPlane(position, npx), Ns = hostPlane(normal, npx), Al = hostPlane(albedo, npx);
    std::vector<float4> C0(npx), C1(npx), V(npx);
    const RegressConsts R = regressConsts(*p);
    const int W = (int)w, H = (int)h;
    const NlmFetchHalves halves{H0.data(), H1.data(), W};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t q = (size_t)y * w + x;
            nlmPrepare(x, y, W, H, halves, C0[q], C1[q], V[q]);
        }
    const RegressFetchPlanes fetch{NlmFetchPlanes{C0.data(), C1.data(), V.data(), W}, Ps.data(), Ns.data(), Al.data()};
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t q = (size_t)y * w + x;
            const bool valid = C0[q].w != 0.0f;
            NlmSums s = nlmZero();
            if (valid) s = regressPixel(x, y, W, H, R, fetch);
            float4 o, e;
            nlmOutput(valid, H0[q], H1[q], s, o, e);
            std::memcpy(out + 4 * q, &o, sizeof o);
            if (outErr) std::memcpy(outErr + 4 * q, &e, sizeof e);
        }
    return SURF_OK;
}

int surf_debug_regress_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->rgTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
