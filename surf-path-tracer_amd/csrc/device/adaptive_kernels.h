/*
 * adaptive_kernels.h -- the active-pixel mask from the noise estimate
 * (surf_mask_from_noise, surf_adaptive_mask_image; include/surf_hip.h gives
 * the arithmetic): the per-pixel rule and the flags kernel that dilates it.
 * The order-preserving compaction of the byte mask into the ascending list a
 * masked stream issues from is compact_kernels.h's.  No reference counterpart.
 *
 * adaptiveRaw and adaptiveActive below are the only place the rule is
 * written; the kernel and the host twin call them on the same values.
 */
#pragma once
#include "compact_kernels.h"        /* the byte mask's compaction into the ascending list */
#include "denoise_kernels.h"        /* the 32 x 8 tile */
#include "sampled_kernels.h"        /* noiseError */
#include "types.h"

namespace surfdev {

constexpr int kAdaptiveMaxDilate = 2;
/* the tile and its widest halo: 36 x 12 flags, 432 B of static LDS */
constexpr int kAdaptiveTileW = kDenoiseTileW + 2 * kAdaptiveMaxDilate, kAdaptiveTileH = kDenoiseTileH + 2 * kAdaptiveMaxDilate;

/* the parameters as the kernel takes them */
struct AdaptiveRule {
    float threshold, floor, minSamples, maxSamples;
    int dilate;
};

/* A pixel that wants more samples on its own account: too few of them, or an
 * error that is not known to be at most the threshold (a NaN counts). */
SURF_HD bool adaptiveRaw(float4 A, float4 Q, const AdaptiveRule& R) {
    return !(A.w >= R.minSamples) || !(noiseError(A, Q, R.floor) <= R.threshold);
}
/* ... and whether it gets them: a raw pixel within `dilate`, and room below the cap. */
SURF_HD bool adaptiveActive(bool anyRaw, float4 A, const AdaptiveRule& R) { return anyRaw && A.w < R.maxSamples; }

#if defined(__HIPCC__) || defined(__HIP__)

/* The byte mask of a W x H frame: 256 threads on a 32 x 8 pixel tile, the grid
 * covering partial tiles.  The threads fill the (32 + 2d) x (8 + 2d) raw flags
 * of the tile and its halo of d = dilate in turn (two rounds at most), each
 * from the texel's accumulator and squares records; a texel outside the frame
 * holds 0 and is never loaded.  After the one barrier a pixel ORs the
 * (2d + 1)^2 bytes around it -- a row of 32 lanes reads 32 consecutive bytes,
 * 8 words, conflict-free -- and writes its byte. */
static __global__ __launch_bounds__(256) void k_adaptive_flags(const float4* __restrict__ A, const float4* __restrict__ Q,
                                                               uint8_t* __restrict__ mask, int W, int H, AdaptiveRule R) {
    __shared__ uint8_t raw[kAdaptiveTileW * kAdaptiveTileH];
    const int d = R.dilate;
    const int tw = kDenoiseTileW + 2 * d, th = kDenoiseTileH + 2 * d;
    const int bx = (int)blockIdx.x * kDenoiseTileW, by = (int)blockIdx.y * kDenoiseTileH;
    const int x0 = bx - d, y0 = by - d;
    for (int t = (int)threadIdx.x; t < tw * th; t += 256) {
        const int ly = t / tw, lx = t - ly * tw;
        const int gx = x0 + lx, gy = y0 + ly;
        uint8_t f = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            f = adaptiveRaw(A[g], Q[g], R) ? 1 : 0;
        }
        raw[ly * kAdaptiveTileW + lx] = f;
    }
    __syncthreads();
    const int tx = (int)(threadIdx.x & (kDenoiseTileW - 1)), ty = (int)(threadIdx.x / kDenoiseTileW);
    const int x = bx + tx, y = by + ty;
    if (x >= W || y >= H) return;
    uint32_t any = 0;
    for (int dy = 0; dy <= 2 * d; ++dy)
        for (int dx = 0; dx <= 2 * d; ++dx) any |= raw[(ty + dy) * kAdaptiveTileW + (tx + dx)];
    const size_t p = (size_t)y * W + x;
    mask[p] = adaptiveActive(any != 0u, A[p], R) ? 1 : 0;
}

#endif  /* HIP */

}  // namespace surfdev
