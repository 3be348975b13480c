/*
 * robust.hip -- the robust estimate of a still from its sample buckets
 * (surf_robust*, include/surf_hip.h): parameter checks, the one launch of
 * k_robust over the context's own planes or over uploaded ones, the trim
 * image and the summary it leaves, and the CPU twin.  The arithmetic lives in
 * device/robust_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/robust_kernels.h"

namespace {

const char* robustParamError(const surf_robust_params* p) {
    if (!p) return "robust params is NULL";
    if (!(std::isfinite(p->trim_scale) && p->trim_scale >= 0.0f)) return "trim_scale is not finite and >= 0";
    return nullptr;
}

bool bucketCount(uint32_t M) { return M == 2 || M == 4 || M == 8 || M == 16; }

/* what is wrong with an image call's arguments, or NULL */
const char* robustImageError(uint32_t npx, uint32_t M, const float* acc, const float* buckets, const surf_robust_params* p, const float* out) {
    if (!acc || !buckets || !out) return "NULL argument";
    if (npx == 0 || npx > (1u << 27)) return "no pixels or too many";
    if (!bucketCount(M)) return "M is none of 2, 4, 8 and 16";
    return robustParamError(p);
}

auto robustKernel(uint32_t M) { return M == 2 ? k_robust<2> : M == 4 ? k_robust<4> : M == 8 ? k_robust<8> : k_robust<16>; }

/* the records the striped counters take at the head of c->rbTrim */
constexpr size_t kCountBytes = (size_t)kRobustStripes * kRobustStripeWords * sizeof(unsigned long long);
constexpr size_t kCountRecords = kCountBytes / sizeof(float4);

/* k_robust over device planes of npx pixels, timed (c->rbTime); the output
 * stays in c->rbOut[0], the trim image (wantTrim) and the counters in
 * c->rbTrim: the counters' stripes first, then npx bytes.  Does not wait. */
int launchRobust(surf_ctx* c, uint32_t npx, uint32_t M, const float4* A, const float4* B, const surf_robust_params& P, bool wantTrim) {
    int rc = c->rbOut.grow(c, npx);
    if (rc) return rc;
    if ((rc = c->rbTrim.grow(c, kCountRecords + ((size_t)npx + 15) / 16))) return rc;
    unsigned long long* dCount = reinterpret_cast<unsigned long long*>(c->rbTrim[0]);
    uint8_t* dTrim = wantTrim ? reinterpret_cast<uint8_t*>(c->rbTrim[0] + kCountRecords) : nullptr;
    SURF_CHECK(c, hipMemsetAsync(dCount, 0, kCountBytes, c->stream));
    SURF_CHECK(c, c->rbTime.mark(0, c->stream));
    hipLaunchKernelGGL(robustKernel(M), dim3((npx + 255) / 256), dim3(256), 0, c->stream, A, B, npx, P.trim_scale, c->rbOut[0], dTrim, dCount);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->rbTime.mark(1, c->stream));
    return SURF_OK;
}

/* the results of the launch to the caller: the image (kind says where dst lives), the trim image and the summary; waits */
int collectRobust(surf_ctx* c, uint32_t npx, void* dst, hipMemcpyKind kind, uint8_t* outTrim, surf_robust_summary* sum) {
    unsigned long long count[kRobustStripes * kRobustStripeWords] = {};
    SURF_CHECK(c, hipMemcpyAsync(dst, c->rbOut[0], (size_t)npx * sizeof(float4), kind, c->stream));
    if (outTrim) SURF_CHECK(c, hipMemcpyAsync(outTrim, c->rbTrim[0] + kCountRecords, npx, hipMemcpyDeviceToHost, c->stream));
    if (sum) SURF_CHECK(c, hipMemcpyAsync(count, c->rbTrim[0], sizeof count, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    SURF_CHECK(c, c->rbTime.collect(1));
    if (sum) {
        sum->pixels = npx;
        sum->trimmed = 0;
        for (uint32_t k = 0; k < kRobustStripes; ++k) sum->trimmed += count[k * kRobustStripeWords];
    }
    return SURF_OK;
}

int robustContext(surf_ctx* c, const surf_robust_params* p, void* dst, hipMemcpyKind kind, uint8_t* outTrim, surf_robust_summary* sum,
                  const char* who) {
    if (!c || !dst) return SURF_ERR_INVALID;
    if (const char* why = robustParamError(p)) return fail(c, SURF_ERR_INVALID, std::string(who) + ": " + why);
    if (!c->bkM) return fail(c, SURF_ERR_INVALID, std::string(who) + ": sample buckets are off (surf_set_sample_buckets)");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = drainStream(c);
    if (rc) return rc;
    if ((rc = launchRobust(c, c->npx, c->bkM, c->acc, c->bk, *p, outTrim != nullptr))) return rc;
    return collectRobust(c, c->npx, dst, kind, outTrim, sum);
}

template <uint32_t M>
void robustHost(uint32_t npx, const float* acc, const float* buckets, float trimScale, float* out, uint8_t* outTrim, uint64_t* trimmed) {
    for (size_t q = 0; q < npx; ++q) {
        float4 A, B[M];                                          /* the caller's planes need not be 16-byte aligned */
        std::memcpy(&A, acc + 4 * q, sizeof A);
        for (uint32_t j = 0; j < M; ++j) std::memcpy(&B[j], buckets + 4 * ((size_t)j * npx + q), sizeof A);
        uint32_t cut = 0;
        const float4 r = robustPixel<M>(A, B, trimScale, &cut);
        std::memcpy(out + 4 * q, &r, sizeof r);
        if (outTrim) outTrim[q] = (uint8_t)cut;
        if (cut) ++*trimmed;
    }
}

}  // namespace

void surfhost::freeRobust(surf_ctx* c) {
    c->rbOut.free();
    c->rbTrim.free();
    c->rbIn.free();
    c->rbTime.destroy();
}

extern "C" {

int surf_robust_default_params(surf_robust_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->trim_scale = 1.0f;
    return SURF_OK;
}

int surf_robust_accumulator(surf_ctx* c, const surf_robust_params* p, float* outAcc, uint8_t* outTrim, surf_robust_summary* sum) {
    return robustContext(c, p, outAcc, hipMemcpyDeviceToHost, outTrim, sum, "surf_robust_accumulator");
}

int surf_robust_copy_device(surf_ctx* c, const surf_robust_params* p, void* dst) {
    return robustContext(c, p, dst, hipMemcpyDeviceToDevice, nullptr, nullptr, "surf_robust_copy_device");
}

int surf_robust_image(surf_ctx* c, uint32_t npx, uint32_t M, const float* acc, const float* buckets, const surf_robust_params* p,
                      float* outAcc, uint8_t* outTrim, surf_robust_summary* sum) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = robustImageError(npx, M, acc, buckets, p, outAcc)) return fail(c, SURF_ERR_INVALID, std::string("surf_robust_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = c->rbIn.grow(c, (size_t)npx * (M + 1));
    if (rc) return rc;
    float4* dA = c->rbIn[0];
    float4* dB = c->rbIn[0] + npx;
    SURF_CHECK(c, hipMemcpyAsync(dA, acc, (size_t)npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(dB, buckets, (size_t)npx * M * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    if ((rc = launchRobust(c, npx, M, dA, dB, *p, outTrim != nullptr))) return rc;
    return collectRobust(c, npx, outAcc, hipMemcpyDeviceToHost, outTrim, sum);
}

/* The CPU twin: robustPixel compiled for the host. */
int surf_robust_image_host(uint32_t npx, uint32_t M, const float* acc, const float* buckets, const surf_robust_params* p, float* outAcc,
                           uint8_t* outTrim, surf_robust_summary* sum) {
    if (const char* why = robustImageError(npx, M, acc, buckets, p, outAcc))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_robust_image_host: ") + why);
    uint64_t trimmed = 0;
    const float ts = p->trim_scale;
    if (M == 2) robustHost<2>(npx, acc, buckets, ts, outAcc, outTrim, &trimmed);
    else if (M == 4) robustHost<4>(npx, acc, buckets, ts, outAcc, outTrim, &trimmed);
    else if (M == 8) robustHost<8>(npx, acc, buckets, ts, outAcc, outTrim, &trimmed);
    else robustHost<16>(npx, acc, buckets, ts, outAcc, outTrim, &trimmed);
    if (sum) {
        sum->pixels = npx;
        sum->trimmed = trimmed;
    }
    return SURF_OK;
}

int surf_debug_robust_time(surf_ctx* c, float* kernel_ms) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->rbTime.read(kernel_ms, 1);
    return SURF_OK;
}

}  // extern "C"
