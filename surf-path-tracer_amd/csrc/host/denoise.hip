/*
 * denoise.hip -- the fixed-sigma a-trous denoiser (surf_denoise*,
 * include/surf_hip.h): parameter checks, the per-iteration constants, the
 * prepare and a-trous launches, the CPU twin, and the growth of every
 * filter's image groups.  The arithmetic lives in device/denoise_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

const char* surfhost::denoiseParamsError(const surf_denoise_params* p) {
    if (!p) return "params is NULL";
    if (p->iterations < 1 || p->iterations > (uint32_t)kDenoiseMaxIterations) return "iterations outside 1..6";
    for (float s : {p->sigma_color, p->sigma_normal, p->sigma_plane})
        if (!(std::isfinite(s) && s > 0.0f)) return "a sigma is not finite and > 0";
    return nullptr;
}

int surfhost::growImages(surf_ctx* c, float4** planes, int count, size_t& cap, size_t npx, const char* what) {
    if (npx <= cap) return SURF_OK;
    for (int k = 0; k < count; ++k) {
        if (planes[k]) (void)hipFree(planes[k]);
        planes[k] = nullptr;
    }
    cap = 0;
    for (int k = 0; k < count; ++k)
        if (hipMalloc(reinterpret_cast<void**>(&planes[k]), npx * sizeof(float4)) != hipSuccess || !planes[k]) {
            planes[k] = nullptr;
            (void)hipGetLastError();
            return fail(c, SURF_ERR_OOM, std::string("hipMalloc of ") + what + " (" + std::to_string(npx * sizeof(float4)) + " bytes an image) failed");
        }
    cap = npx;
    return SURF_OK;
}

namespace {

/* the per-iteration constants, computed in f32 on the host as the header states */
struct DenoiseConsts { float kc, kn, kp; };
DenoiseConsts denoiseConsts(const surf_denoise_params& p, uint32_t i) {
    const float sc = p.sigma_color * ldexpf(1.0f, -(int)i);
    DenoiseConsts k;
    k.kc = 1.0f / (sc * sc);
    k.kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    k.kp = 1.0f / (p.sigma_plane * p.sigma_plane);
    return k;
}

}  // namespace

/* Prepare + n a-trous launches on the context's stream. */
int surfhost::denoisePlanes(surf_ctx* c, uint32_t w, uint32_t h, const float4* acc, const float4* pos, const float4* nrm, const float4* alb,
                            const surf_denoise_params& P, const float4** result) {
    const size_t npx = (size_t)w * h;
    int rc = c->dn.grow(c, npx);
    if (rc) return rc;
    const float4* gN = c->dn[2];
    const float4* gP = c->dn[3];
    const uint32_t demod = P.demodulate ? 1u : 0u;
    SURF_CHECK(c, c->dnTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_denoise_prepare, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, acc, pos, nrm, alb, demod,
                       (uint32_t)npx, c->dn[0], c->dn[2], c->dn[3]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->dnTime.mark(1, c->stream));
    return runAtrous(c, w, h, P.iterations, c->dnTime, 1, [&](const AtrousStep& st) {
        const DenoiseConsts k = denoiseConsts(P, st.i);
        hipLaunchKernelGGL(st.staged ? k_atrous<true> : k_atrous<false>, st.grid, dim3(256), st.lds, c->stream, st.in, gN, gP, alb, st.out,
                           (int)w, (int)h, st.s, k.kc, k.kn, k.kp, demod, st.last);
    }, result);
}

namespace {

/* surf_denoise / surf_denoise_copy_device: the context's own accumulator and
 * cached feature planes, the result copied to the host or to a device buffer */
int denoiseContext(surf_ctx* c, const surf_denoise_params* p, void* dst, hipMemcpyKind kind) {
    if (!c || !dst) return SURF_ERR_INVALID;
    if (const char* why = denoiseParamsError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_denoise: ") + why);
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_denoise needs a context that owns every row of the frame: a spatial filter reads its "
                                         "neighbours' rows; assemble the shards' accumulators and feature planes and call surf_denoise_image");
    void* const* g = nullptr;     /* the first-hit planes, the chain's or the sampled ones (surf_set_filter_guides*) */
    int rc = guidePlanes(c, &g);
    if (rc) return rc;
    if ((rc = drainStream(c))) return rc;
    const float4* res = nullptr;
    rc = denoisePlanes(c, c->width, c->height, c->acc, static_cast<const float4*>(g[SURF_AOV_POSITION]),
                       static_cast<const float4*>(g[SURF_AOV_NORMAL]), static_cast<const float4*>(g[SURF_AOV_ALBEDO]), *p, &res);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(dst, res, (size_t)c->npx * sizeof(float4), kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

}  // namespace

void surfhost::freeDenoise(surf_ctx* c) {
    c->dn.free();
    c->dnIn.free();
    c->dnTime.destroy();
}

extern "C" {

int surf_denoise_default_params(surf_denoise_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->iterations = 5;
    p->sigma_color = 1.0f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 0.1f;
    p->demodulate = 1;
    return SURF_OK;
}

int surf_denoise(surf_ctx* c, const surf_denoise_params* p, float* out) {
    return denoiseContext(c, p, out, hipMemcpyDeviceToHost);
}

int surf_denoise_copy_device(surf_ctx* c, const surf_denoise_params* p, void* dst) {
    return denoiseContext(c, p, dst, hipMemcpyDeviceToDevice);
}

int surf_denoise_image(surf_ctx* c, uint32_t w, uint32_t h, const float* acc, const float* position, const float* normal,
                       const float* albedo, const surf_denoise_params* p, float* out) {
    if (!c || !acc || !position || !normal || !albedo || !out) return SURF_ERR_INVALID;
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return fail(c, SURF_ERR_INVALID, "surf_denoise_image: empty or too large a frame");
    if (const char* why = denoiseParamsError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_denoise_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h;
    int rc = c->dnIn.grow(c, npx);
    if (rc) return rc;
    const float* src[4] = {acc, position, normal, albedo};
    for (int k = 0; k < 4; ++k)
        SURF_CHECK(c, hipMemcpyAsync(c->dnIn[k], src[k], npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    const float4* res = nullptr;
    if ((rc = denoisePlanes(c, w, h, c->dnIn[0], c->dnIn[1], c->dnIn[2], c->dnIn[3], *p, &res))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, res, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* The CPU twin: denoisePrepare / denoisePixel / denoiseStore of
 * device/denoise_kernels.h compiled for the host, on host arrays. */
int surf_denoise_image_host(uint32_t w, uint32_t h, const float* acc, const float* position, const float* normal,
                            const float* albedo, const surf_denoise_params* p, float* out) {
    if (!acc || !position || !normal || !albedo || !out) return fail(nullptr, SURF_ERR_INVALID, "surf_denoise_image_host: NULL argument");
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return fail(nullptr, SURF_ERR_INVALID, "surf_denoise_image_host: empty or too large a frame");
    if (const char* why = denoiseParamsError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const std::vector<float4> A = hostPlane(acc, npx), Ps = hostPlane(position, npx), Ns = hostPlane(normal, npx), Al = hostPlane(albedo, npx);
    const uint32_t demod = p->demodulate ? 1u : 0u;
    std::vector<float4> lvl[2], gN(npx), gP(npx);
    lvl[0].resize(npx);
    lvl[1].resize(npx);
    for (size_t q = 0; q < npx; ++q) denoisePrepare(A[q], Ps[q], Ns[q], Al[q], demod, lvl[0][q], gN[q], gP[q]);
    for (uint32_t i = 0; i < p->iterations; ++i) {
        const int s = 1 << i;
        const DenoiseConsts k = denoiseConsts(*p, i);
        const bool last = i + 1 == p->iterations;
        const std::vector<float4>& I = lvl[i & 1];
        std::vector<float4>& O = lvl[(i & 1) ^ 1];
        const DenoiseFetchPlanes fetch{I.data(), gN.data(), gP.data(), (int)w};
        for (int y = 0; y < (int)h; ++y)
            for (int x = 0; x < (int)w; ++x) {
                const size_t q = (size_t)y * w + x;
                const bool valid = gN[q].w != 0.0f;
                V3 f = mk3(0.0f, 0.0f, 0.0f);
                if (valid) f = denoisePixel(x, y, (int)w, (int)h, s, k.kc, k.kn, k.kp, I[q], gN[q], gP[q], fetch);
                O[q] = denoiseStore(valid, I[q], f, last, Al[q], demod);
            }
    }
    std::memcpy(out, lvl[p->iterations & 1].data(), npx * sizeof(float4));
    return SURF_OK;
}

int surf_debug_denoise_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->dnTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
