/*
 * nlm.hip -- the dual-buffer non-local-means filter for stills
 * (surf_denoise_nlm*, include/surf_hip.h) and the driver it shares with the
 * other stills filter on the sample buckets' halves (host/regress.hip):
 * parameter checks, the host constants, runStills -- the checks, the halves
 * and prepare launches over the context's buckets or over uploaded half
 * planes, the handed filter launch, the copies out -- and its CPU twin, and
 * this filter's launch with the choice between the staged and the global
 * kernel.  The arithmetic lives in device/nlm_kernels.h.
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

/* The driver's two kernels -- here, not in the header both stills filters include: one object holds them. */

/* The halves of n pixels from M bucket planes n records apart: half 0 the even
 * planes added in ascending order to 0, half 1 the odd ones. */
__global__ __launch_bounds__(256) void k_nlm_halves(const float4* __restrict__ bk, uint32_t M, uint32_t n, float4* __restrict__ H0,
                                                    float4* __restrict__ H1) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float4 s[2] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
    for (uint32_t j = 0; j < M; j += 2) {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const float4 b = bk[(size_t)(j + h) * n + p];
            s[h] = make_float4(s[h].x + b.x, s[h].y + b.y, s[h].z + b.z, s[h].w + b.w);
        }
    }
    H0[p] = s[0];
    H1[p] = s[1];
}

/* Prepare: one thread per pixel of the 32 x 8 tiles; the nine neighbours' half
 * records come from global memory (the 3 x 3 windows of a tile overlap in L1). */
__global__ __launch_bounds__(256) void k_nlm_prepare(const float4* __restrict__ H0, const float4* __restrict__ H1, int W, int H,
                                                     float4* __restrict__ C0, float4* __restrict__ C1, float4* __restrict__ V) {
    const TilePixel px = tilePixel(W, H);
    if (!px.inside) return;
    const NlmFetchHalves fetch{H0, H1, W};
    float4 c0, c1, v;
    nlmPrepare(px.x, px.y, W, H, fetch, c0, c1, v);
    C0[px.p] = c0;
    C1[px.p] = c1;
    V[px.p] = v;
}

/* the scratch images of c->nl */
enum { kH0, kH1, kC0, kC1, kV, kOut, kErr };

/* this filter's call of the driver: the launch of k_nlm, staged where the layout fits */
int runNlm(surf_ctx* c, StillsCall call, const surf_nlm_params* p, const float4** dOut = nullptr, const float4** dErr = nullptr) {
    call.paramsWhy = nlmParamError(p);
    call.shardAdvice = "assemble the shards' bucket planes, sum their halves and call surf_denoise_nlm_image";
    call.planesWhat = c->nl.what;
    return runStills(c, call, c->nlTime, [&](const StillsStep& st) -> int {
        const NlmConsts K = nlmConsts(*p);
        const size_t lds = nlmLdsBytes(K.r, K.f);
        const bool staged = c->nlStaged && lds <= kNlmLdsMax;
        hipLaunchKernelGGL(staged ? k_nlm<true> : k_nlm<false>, st.grid, dim3(256), staged ? lds : 0, c->stream, st.C0, st.C1, st.V, st.H0, st.H1,
                           st.out, st.err, st.W, st.H, K);
        return SURF_OK;
    }, dOut, dErr);
}

int nlmContext(surf_ctx* c, const surf_nlm_params* p, void* out, void* outErr, hipMemcpyKind kind, const char* who) {
    if (!c || !out) return SURF_ERR_INVALID;
    return runNlm(c, StillsCall{who, 0, 0, nullptr, nullptr, out, outErr, kind}, p);
}

}  // namespace

const char* surfhost::nlmParamsError(const surf_nlm_params* p) { return nlmParamError(p); }

NlmConsts surfhost::nlmConsts(const surf_nlm_params& p) {
    NlmConsts K;
    K.r = (int)p.search_radius;
    K.f = (int)p.patch_radius;
    K.kk = p.k * p.k;
    K.alpha = p.alpha;
    K.eps = p.eps;
    K.cnt = (float)(3 * (2 * K.f + 1) * (2 * K.f + 1));
    return K;
}

const char* surfhost::stillsImageError(uint32_t w, uint32_t h, const char* paramsWhy) {
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 27)) return "empty or too large a frame";
    return paramsWhy;
}

int surfhost::runStills(surf_ctx* c, const StillsCall& call, StageTimer<3>& T, const std::function<int(const StillsStep&)>& launch,
                        const float4** dOut, const float4** dErr) {
    const bool image = call.half0 != nullptr;
    const std::string who(call.who);
    if (image) {
        if (const char* why = stillsImageError(call.w, call.h, call.paramsWhy)) return fail(c, SURF_ERR_INVALID, who + ": " + why);
    } else {
        if (call.paramsWhy) return fail(c, SURF_ERR_INVALID, who + ": " + call.paramsWhy);
        if (!c->bkM) return fail(c, SURF_ERR_INVALID, who + ": sample buckets are off (surf_set_sample_buckets)");
        if (c->rows.size() != c->height)
            return fail(c, SURF_ERR_INVALID, who + " needs a context that owns every row of the frame: a patch reads its neighbours' rows; " +
                                             call.shardAdvice);
    }
    SURF_CHECK(c, hipSetDevice(c->device));
    const uint32_t w = image ? call.w : c->width, h = image ? call.h : c->height;
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = SURF_OK;
    if (image) {
        if ((rc = growImages(c, c->nl.p, 7, c->nl.cap, npx, call.planesWhat))) return rc;
        SURF_CHECK(c, hipMemcpyAsync(c->nl[kH0], call.half0, bytes, hipMemcpyHostToDevice, c->stream));
        SURF_CHECK(c, hipMemcpyAsync(c->nl[kH1], call.half1, bytes, hipMemcpyHostToDevice, c->stream));
        if (call.ready && (rc = call.ready())) return rc;
        SURF_CHECK(c, T.mark(0, c->stream));           /* no halves launch: stage 0 is empty */
    } else {
        if (call.ready && (rc = call.ready())) return rc;
        if ((rc = drainStream(c))) return rc;
        if ((rc = growImages(c, c->nl.p, 7, c->nl.cap, npx, call.planesWhat))) return rc;
        SURF_CHECK(c, T.mark(0, c->stream));
        hipLaunchKernelGGL(k_nlm_halves, dim3((c->npx + 255) / 256), dim3(256), 0, c->stream, (const float4*)c->bk, c->bkM, c->npx, c->nl[kH0],
                           c->nl[kH1]);
        SURF_CHECK(c, hipGetLastError());
    }
    SURF_CHECK(c, T.mark(1, c->stream));
    const StillsStep st{tileGrid(w, h), c->nl[kC0], c->nl[kC1], c->nl[kV], c->nl[kH0], c->nl[kH1], c->nl[kOut], c->nl[kErr], (int)w, (int)h};
    hipLaunchKernelGGL(k_nlm_prepare, st.grid, dim3(256), 0, c->stream, st.H0, st.H1, st.W, st.H, c->nl[kC0], c->nl[kC1], c->nl[kV]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, T.mark(2, c->stream));
    if ((rc = launch(st))) return rc;
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, T.mark(3, c->stream));
    SURF_CHECK(c, T.collect(3));
    if (dOut) *dOut = st.out;
    if (dErr) *dErr = st.err;
    if (call.out) {
        SURF_CHECK(c, hipMemcpyAsync(call.out, st.out, bytes, call.kind, c->stream));
        if (call.outErr) SURF_CHECK(c, hipMemcpyAsync(call.outErr, st.err, bytes, call.kind, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
    }
    return SURF_OK;
}

void surfhost::stillsTwin(uint32_t w, uint32_t h, const float* half0, const float* half1,
                          const std::function<NlmSums(int, int, const NlmFetchPlanes&)>& pixel, float* out, float* outErr) {
    const size_t npx = (size_t)w * h;
    const std::vector<float4> H0 = hostPlane(half0, npx), H1 = hostPlane(half1, npx);
    std::vector<float4> C0(npx), C1(npx), V(npx);
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
            if (valid) s = pixel(x, y, fetch);
            float4 o, e;
            nlmOutput(valid, H0[q], H1[q], s, o, e);
            std::memcpy(out + 4 * q, &o, sizeof o);
            if (outErr) std::memcpy(outErr + 4 * q, &e, sizeof e);
        }
}

int surfhost::nlmContextPlanes(surf_ctx* c, const surf_nlm_params* p, const char* who, const float4** out, const float4** err) {
    return runNlm(c, StillsCall{who}, p, out, err);
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
    if (!half0 || !half1 || !out) return fail(c, SURF_ERR_INVALID, "surf_denoise_nlm_image: NULL argument");
    return runNlm(c, StillsCall{"surf_denoise_nlm_image", w, h, half0, half1, out, outErr, hipMemcpyDeviceToHost}, p);
}

/* The CPU twin: nlmPrepare / nlmPixel / nlmOutput of device/nlm_kernels.h compiled for the host, on host arrays. */
int surf_denoise_nlm_image_host(uint32_t w, uint32_t h, const float* half0, const float* half1, const surf_nlm_params* p, float* out,
                                float* outErr) {
    const char* why = !half0 || !half1 || !out ? "NULL argument" : stillsImageError(w, h, nlmParamError(p));
    if (why) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_nlm_image_host: ") + why);
    const NlmConsts K = nlmConsts(*p);
    stillsTwin(w, h, half0, half1, [&](int x, int y, const NlmFetchPlanes& fetch) { return nlmPixel(x, y, (int)w, (int)h, K, fetch); }, out, outErr);
    return SURF_OK;
}

int surf_debug_nlm_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->nlTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
