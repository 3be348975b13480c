/*
 * regress.hip -- the first-order feature regression filter for stills
 * (surf_denoise_regress*, include/surf_hip.h): parameter checks, the host
 * constants, the guide planes of the context form and the uploaded feature
 * planes of the image form, and this filter's launch with the choice between
 * the staged and the global kernel, handed to the stills filters' driver and
 * its CPU twin (host/nlm.hip).  The arithmetic lives in
 * device/regress_kernels.h and, for what the non-local-means filter shares
 * with it, in device/nlm_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/regress_kernels.h"

namespace {

/* the weights' parameters mean what they mean to the non-local-means filter */
surf_nlm_params weightsOf(const surf_regress_params& p) { return surf_nlm_params{p.search_radius, p.patch_radius, p.k, p.alpha, p.eps, 0}; }

const char* regressParamError(const surf_regress_params* p) {
    if (!p) return "params is NULL";
    const surf_nlm_params weights = weightsOf(*p);
    if (const char* why = nlmParamsError(&weights)) return why;
    if (!(std::isfinite(p->ridge) && p->ridge > 0.0f)) return "ridge is not finite and > 0";
    return nullptr;
}

RegressConsts regressConsts(const surf_regress_params& p) { return RegressConsts{nlmConsts(weightsOf(p)), p.ridge}; }

/* the planes of c->rgIn, which the image form uploads */
enum { kPos, kNrm, kAlb };

/* This filter's call of the driver.  *pos, *nrm, *alb: the three feature
 * planes on the device, which call.ready puts in place. */
int runRegress(surf_ctx* c, StillsCall call, const surf_regress_params* p, const float4* const* pos, const float4* const* nrm,
               const float4* const* alb) {
    call.paramsWhy = regressParamError(p);
    call.shardAdvice = "assemble the shards' bucket planes and feature planes, sum the halves and call surf_denoise_regress_image";
    call.planesWhat = "the regression filter's planes";
    return runStills(c, call, c->rgTime, [&](const StillsStep& st) -> int {
        const RegressConsts R = regressConsts(*p);
        const size_t lds = regressLdsBytes(R.n.r, R.n.f);
        const bool staged = c->rgStaged && lds <= kRegressLdsMax;
        if (staged && !c->rgLdsSet) {             /* announce that launches will ask for more than 64 KiB of dynamic LDS */
            SURF_CHECK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_regress<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)kRegressLdsMax));
            c->rgLdsSet = true;
        }
        hipLaunchKernelGGL(staged ? k_regress<true> : k_regress<false>, st.grid, dim3(256), staged ? lds : 0, c->stream, st.C0, st.C1, st.V, st.H0,
                           st.H1, *pos, *nrm, *alb, st.out, st.err, st.W, st.H, R);
        return SURF_OK;
    });
}

int regressContext(surf_ctx* c, const surf_regress_params* p, void* out, void* outErr, hipMemcpyKind kind, const char* who) {
    if (!c || !out) return SURF_ERR_INVALID;
    const float4 *pos = nullptr, *nrm = nullptr, *alb = nullptr;
    StillsCall call{who, 0, 0, nullptr, nullptr, out, outErr, kind};
    call.ready = [&]() -> int {
        void* const* g = nullptr;     /* the first-hit planes, the chain's or the sampled ones (surf_set_filter_guides*) */
        if (int rc = guidePlanes(c, &g)) return rc;
        pos = static_cast<const float4*>(g[SURF_AOV_POSITION]);
        nrm = static_cast<const float4*>(g[SURF_AOV_NORMAL]);
        alb = static_cast<const float4*>(g[SURF_AOV_ALBEDO]);
        return SURF_OK;
    };
    return runRegress(c, call, p, &pos, &nrm, &alb);
}

}  // namespace

void surfhost::freeRegress(surf_ctx* c) {
    c->rgIn.free();
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
    if (!half0 || !half1 || !position || !normal || !albedo || !out) return fail(c, SURF_ERR_INVALID, "surf_denoise_regress_image: NULL argument");
    const float4 *pos = nullptr, *nrm = nullptr, *alb = nullptr;
    StillsCall call{"surf_denoise_regress_image", w, h, half0, half1, out, outErr, hipMemcpyDeviceToHost};
    call.ready = [&]() -> int {
        const size_t npx = (size_t)w * h;
        if (int rc = c->rgIn.grow(c, npx)) return rc;
        const float* src[3] = {position, normal, albedo};
        for (int k = 0; k < 3; ++k) SURF_CHECK(c, hipMemcpyAsync(c->rgIn[k], src[k], npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        pos = c->rgIn[kPos];
        nrm = c->rgIn[kNrm];
        alb = c->rgIn[kAlb];
        return SURF_OK;
    };
    return runRegress(c, call, p, &pos, &nrm, &alb);
}

/* The CPU twin: nlmPrepare of device/nlm_kernels.h, regressPixel of device/regress_kernels.h and nlmOutput compiled
 * for the host, on host arrays. */
int surf_denoise_regress_image_host(uint32_t w, uint32_t h, const float* half0, const float* half1, const float* position,
                                    const float* normal, const float* albedo, const surf_regress_params* p, float* out, float* outErr) {
    const char* why = !half0 || !half1 || !position || !normal || !albedo || !out ? "NULL argument" : stillsImageError(w, h, regressParamError(p));
    if (why) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_regress_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const std::vector<float4> Ps = hostPlane(position, npx), Ns = hostPlane(normal, npx), Al = hostPlane(albedo, npx);
    const RegressConsts R = regressConsts(*p);
    const RegressFetchFeat feat{Ps.data(), Ns.data(), Al.data(), (int)w};
    stillsTwin(w, h, half0, half1,
               [&](int x, int y, const NlmFetchPlanes& fetch) { return regressPixel(x, y, (int)w, (int)h, R, fetch, feat); }, out, outErr);
    return SURF_OK;
}

int surf_debug_regress_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->rgTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
