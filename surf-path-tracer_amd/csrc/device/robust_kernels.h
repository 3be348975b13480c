/*
 * robust_kernels.h -- what the sample buckets (the M planes
 * k_accumulate_buckets keeps beside the accumulator) are read for
 * (surf_robust_*, include/surf_hip.h gives the arithmetic): the median-of-means
 * estimate of a pixel with a Gini-adaptive trim -- a pixel without outliers
 * keeps its mean, a pixel with outliers drops its extreme bucket means
 * (Buisine et al. 2021).  No reference counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states.  robustPixel below is the only place it is written; the
 * kernel and the host twin call it on the same values.
 */
#pragma once
#include "surf_math.h"
#include "temporal_kernels.h"       /* svgfLum */
#include "types.h"

namespace surfdev {

/* One pixel: A its accumulator record, B its M bucket records in bucket order.
 * Returns the output record, *trim the bucket means dropped at either end.
 * Every loop has a compile-time trip count and every array a compile-time
 * index once unrolled: the buckets are ordered by counting ranks (M^2
 * compares) and taken by rank (M^2 selects), so the device keeps all of it in
 * registers. */
template <uint32_t M>
SURF_HD float4 robustPixel(float4 A, const float4 (&B)[M], float trimScale, uint32_t* trim) {
    static_assert(M == 2 || M == 4 || M == 8 || M == 16, "bucket counts the interface allows");
    *trim = 0u;
    bool ok = true;
    float mx[M], my[M], mz[M], l[M];
#pragma unroll
    for (uint32_t j = 0; j < M; ++j) {
        const float n = B[j].w;
        if (!(n > 0.0f)) ok = false;
        mx[j] = B[j].x / n;
        my[j] = B[j].y / n;
        mz[j] = B[j].z / n;
        l[j] = svgfLum(mx[j], my[j], mz[j]);
        if (!(l[j] - l[j] == 0.0f)) ok = false;               /* not finite */
    }
    if (!ok) return A;
    /* rank[j]: how many buckets precede j in the order by (l, index) */
    uint32_t rank[M];
#pragma unroll
    for (uint32_t j = 0; j < M; ++j) {
        uint32_t r = 0u;
#pragma unroll
        for (uint32_t i = 0; i < M; ++i)
            if (i != j && (l[i] < l[j] || (l[i] == l[j] && i < j))) ++r;
        rank[j] = r;
    }
    /* the means in that order */
    float sx[M], sy[M], sz[M], sl[M];
#pragma unroll
    for (uint32_t i = 0; i < M; ++i) {
        float x = 0.0f, y = 0.0f, z = 0.0f, v = 0.0f;
#pragma unroll
        for (uint32_t j = 0; j < M; ++j)
            if (rank[j] == i) { x = mx[j]; y = my[j]; z = mz[j]; v = l[j]; }
        sx[i] = x; sy[i] = y; sz[i] = z; sl[i] = v;
    }
    float T = 0.0f, Gn = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < M; ++i) {
        T = T + sl[i];
        Gn = Gn + (float)(2 * (int)(i + 1u) - (int)M - 1) * sl[i];
    }
    if (!(T > 0.0f)) return A;
    const float G = Gn / ((float)M * T);
    const float f = floorf((G * trimScale) * ((float)M * 0.5f));
    constexpr uint32_t cap = (M - 1u) / 2u;
    uint32_t c = 0u;
    if (f >= 1.0f) c = f >= (float)cap ? cap : (uint32_t)f;     /* a value below 1 or a NaN gives 0 */
    if (c == 0u) return A;
    float ex = 0.0f, ey = 0.0f, ez = 0.0f;
#pragma unroll
    for (uint32_t i = 0; i < M; ++i)
        if (i >= c && i < M - c) { ex = ex + sx[i]; ey = ey + sy[i]; ez = ez + sz[i]; }
    const float d = (float)(M - 2u * c);
    ex = ex / d; ey = ey / d; ez = ez / d;
    *trim = c;
    return make_float4(ex * A.w, ey * A.w, ez * A.w, A.w);
}

/* what k_robust counts the trimmed pixels into: kRobustStripes 64-bit counters,
 * one per 128-byte line, zeroed before the launch and summed by the host.  A
 * block adds to stripe blockIdx.x % kRobustStripes: with every wave adding to
 * one address the kernel took 0.13 - 0.2 ms at 1280 x 720, against 0.02 - 0.07
 * (MEASUREMENTS "Robust estimate"). */
constexpr uint32_t kRobustStripes = 32;
constexpr uint32_t kRobustStripeWords = 16;      /* 64-bit words from one stripe's counter to the next */

#if defined(__HIPCC__) || defined(__HIP__)

/* The robust estimate of n pixels: one thread per pixel, consecutive lanes
 * consecutive records of every plane; (M + 1) 16-byte loads, one 16-byte
 * store and, with a trim image, one byte.  bk: the M bucket planes, n records
 * apart.  The trimmed pixels are counted as k_noise counts: every lane of a
 * wave takes part (a lane past n adds nothing), a ballot and popcount, then
 * lane 0 issues one 64-bit integer add to its block's stripe -- exact whatever
 * order the waves arrive in. */
template <uint32_t M>
static __global__ __launch_bounds__(256) void k_robust(const float4* __restrict__ A, const float4* __restrict__ bk, uint32_t n,
                                                       float trimScale, float4* __restrict__ out, uint8_t* __restrict__ trim,
                                                       unsigned long long* __restrict__ trimmed) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool cut = false;
    if (p < n) {
        float4 B[M];
#pragma unroll
        for (uint32_t j = 0; j < M; ++j) B[j] = bk[(size_t)j * n + p];
        uint32_t c = 0u;
        out[p] = robustPixel<M>(A[p], B, trimScale, &c);
        if (trim) trim[p] = (uint8_t)c;
        cut = c > 0u;
    }
    const unsigned long long votes = __ballot(cut);
    if ((threadIdx.x & 63u) == 0u && votes)
        atomicAdd(trimmed + (blockIdx.x % kRobustStripes) * kRobustStripeWords, (unsigned long long)__popcll(votes));
}

#endif  /* HIP */

}  // namespace surfdev
