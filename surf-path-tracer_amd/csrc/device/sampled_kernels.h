/*
 * sampled_kernels.h -- what the per-sample second moments (the squares plane
 * k_accumulate<true> keeps beside the accumulator) are read for
 * (surf_denoise_sampled*, surf_noise_*, include/surf_hip.h gives the
 * arithmetic): level 0 of the sample-variance-guided filter -- the variance
 * of the pixel mean in the image's w, in front of the variance-guided
 * a-trous iterations of svgf_kernels.h, which run unchanged -- and the noise
 * estimate, the relative standard error of a pixel's mean luminance with its
 * summary.  No reference counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states.  sampledLevel0 and noiseError below are the only place
 * it is written; the kernels and the host twins call them on the same values.
 */
#pragma once
#include "denoise_kernels.h"
#include "surf_math.h"
#include "svgf_kernels.h"           /* svgfLevel0 */
#include "temporal_kernels.h"       /* svgfLum */
#include "types.h"

namespace surfdev {

/* what a pixel with fewer than two samples reports as its error */
constexpr float kNoiseNoEstimate = 1e30f;

/* Level 0 of a pixel: (c / den, v), v the unbiased sample variance of the
 * mean of the demodulated luminance, the channels' deviations taken as fully
 * correlated; v = 0 for an invalid pixel and below two samples. */
SURF_HD float4 sampledLevel0(float4 A, float4 Q, float4 alb, uint32_t demodulate) {
    const float n = A.w;
    const float inv = A.w > 0.0f ? 1.0f / A.w : 0.0f;
    const V3 c = mk3(A.x * inv, A.y * inv, A.z * inv);
    float v = 0.0f;
    if (alb.w != 0.0f && n >= 2.0f) {
        const V3 den = denoiseDen(alb, demodulate);
        float tx = Q.x * inv - c.x * c.x, ty = Q.y * inv - c.y * c.y, tz = Q.z * inv - c.z * c.z;
        tx = tx > 0.0f ? tx : 0.0f;                      /* a NaN becomes 0 */
        ty = ty > 0.0f ? ty : 0.0f;
        tz = tz > 0.0f ? tz : 0.0f;
        const float sd = svgfLum(sqrtf(tx) / den.x, sqrtf(ty) / den.y, sqrtf(tz) / den.z);
        v = (sd * sd) / (n - 1.0f);
    }
    return svgfLevel0(make_float4(c.x, c.y, c.z, 0.0f), alb, demodulate, v);
}

/* The relative standard error of a pixel's mean luminance. */
SURF_HD float noiseError(float4 A, float4 Q, float floor) {
    const float n = A.w;
    if (!(n >= 2.0f)) return kNoiseNoEstimate;
    const float inv = 1.0f / n;
    const float lb = svgfLum(A.x * inv, A.y * inv, A.z * inv);
    float t = Q.w * inv - lb * lb;
    t = t > 0.0f ? t : 0.0f;
    return sqrtf(t / (n - 1.0f)) / (lb + floor);
}

/* What a pixel's error adds to the summary: whether it counts as above the
 * threshold (a NaN does), and the running maximum, which starts at 0 and
 * which a NaN or a negative error leaves alone. */
SURF_HD bool noiseAbove(float e, float threshold) { return !(e <= threshold); }
SURF_HD float noiseMax(float mx, float e) { return e > mx ? e : mx; }

#if defined(__HIPCC__) || defined(__HIP__)

/* Level 0 of the sample-variance-guided filter: 256 threads on a 32 x 8 pixel
 * tile, the grid covering partial tiles (the iterations' grid).  Pointwise:
 * three 16-byte loads (accumulator, squares, albedo), consecutive lanes
 * consecutive records, one 16-byte and one 4-byte store -- 48 B in, 20 B out
 * per pixel.  The guides are packed by k_svgf_guides, as for surf_svgf_*. */
static __global__ __launch_bounds__(256) void k_sampled_level0(const float4* __restrict__ A, const float4* __restrict__ Q,
                                                               const float4* __restrict__ alb, float4* __restrict__ I0,
                                                               float* __restrict__ var0, int W, int H, uint32_t demodulate) {
    const int x = (int)blockIdx.x * kDenoiseTileW + (int)(threadIdx.x & (kDenoiseTileW - 1));
    const int y = (int)blockIdx.y * kDenoiseTileH + (int)(threadIdx.x / kDenoiseTileW);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 i0 = sampledLevel0(A[p], Q[p], alb[p], demodulate);
    I0[p] = i0;
    var0[p] = i0.w;
}

/* what k_noise reduces into: zeroed before the launch */
struct NoiseSums {
    unsigned long long above;
    uint32_t maxBits;            /* the bits of the largest error, a non-negative float: their order is the floats' */
    uint32_t _pad;
};

/* The noise estimate of n pixels: the error image where err is not NULL, and
 * the summary.  Every lane of a wave takes part in the reduction (a lane past
 * n adds nothing): the count by ballot and popcount, the maximum by six
 * lane shuffles (xor 32 .. 1); then lane 0 of the wave issues one 64-bit
 * integer add and one 32-bit unsigned max, both exact and independent of the
 * order the waves arrive in.  32 B in per pixel, 4 B out with an image. */
static __global__ __launch_bounds__(256) void k_noise(const float4* __restrict__ A, const float4* __restrict__ Q, uint32_t n,
                                                      float threshold, float floor, float* __restrict__ err,
                                                      NoiseSums* __restrict__ sums) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    bool above = false;
    float mx = 0.0f;
    if (p < n) {
        const float e = noiseError(A[p], Q[p], floor);
        if (err) err[p] = e;
        above = noiseAbove(e, threshold);
        mx = noiseMax(0.0f, e);
    }
    const unsigned long long votes = __ballot(above);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = noiseMax(mx, __shfl_xor(mx, d));
    if ((threadIdx.x & 63u) == 0u) {
        if (votes) atomicAdd(&sums->above, (unsigned long long)__popcll(votes));
        if (mx > 0.0f) atomicMax(&sums->maxBits, __float_as_uint(mx));
    }
}

#endif  /* HIP */

}  // namespace surfdev
