/*
 * adaptive_kernels.h -- the active-pixel mask from the noise estimate
 * (surf_mask_from_noise, surf_adaptive_mask_image; include/surf_hip.h gives
 * the arithmetic): the per-pixel rule, the flags kernel that dilates it, and
 * the order-preserving compaction of the byte mask into the ascending list a
 * masked stream issues from.  No reference counterpart.
 *
 * adaptiveRaw and adaptiveActive below are the only place the rule is
 * written; the kernel and the host twin call them on the same values.
 */
#pragma once
#include "denoise_kernels.h"        /* the 32 x 8 tile */
#include "sampled_kernels.h"        /* noiseError */
#include "types.h"

namespace surfdev {

constexpr int kAdaptiveMaxDilate = 2;
/* the tile and its widest halo: 36 x 12 flags, 432 B of static LDS */
constexpr int kAdaptiveTileW = kDenoiseTileW + 2 * kAdaptiveMaxDilate, kAdaptiveTileH = kDenoiseTileH + 2 * kAdaptiveMaxDilate;
constexpr uint32_t kCompactBlock = 256;      /* pixels per block of the compaction */

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

/* Compaction, step 1: blk[b] = the nonzero bytes among pixels [256 b, 256 b + 256). */
static __global__ __launch_bounds__(kCompactBlock) void k_compact_count(const uint8_t* __restrict__ mask, uint32_t n,
                                                                        uint32_t* __restrict__ blk) {
    __shared__ uint32_t wv[kCompactBlock / 64];
    const uint32_t p = blockIdx.x * kCompactBlock + threadIdx.x;
    const bool on = p < n && mask[p] != 0;
    const unsigned long long votes = __ballot(on);
    if ((threadIdx.x & 63u) == 0u) wv[threadIdx.x >> 6] = (uint32_t)__popcll(votes);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = (wv[0] + wv[1]) + (wv[2] + wv[3]);
}

/* Step 2, one block of 1024 threads: the block counts become their exclusive
 * prefix sums, blk[nb] the total.  Each thread takes a run of consecutive
 * counts; the 1024 run sums are scanned in LDS (k_binscan's pattern). */
static __global__ __launch_bounds__(1024) void k_compact_scan(uint32_t* __restrict__ blk, uint32_t nb) {
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (nb + 1023u) / 1024u;
    const uint32_t a = t * per < nb ? t * per : nb, b = a + per < nb ? a + per : nb;
    uint32_t sum = 0;
    for (uint32_t k = a; k < b; ++k) sum += blk[k];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
        const uint32_t v = t >= off ? part[t - off] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - sum;
    for (uint32_t k = a; k < b; ++k) { const uint32_t c = blk[k]; blk[k] = run; run += c; }
    if (t == 1023u) blk[nb] = part[1023];
}

/* Step 3: pixel p's index goes to list[blk[b] + active pixels of the block's
 * earlier waves + active lanes below it in its wave]. */
static __global__ __launch_bounds__(kCompactBlock) void k_compact_scatter(const uint8_t* __restrict__ mask, uint32_t n,
                                                                          const uint32_t* __restrict__ blk, uint32_t* __restrict__ list) {
    __shared__ uint32_t wv[kCompactBlock / 64];
    const uint32_t p = blockIdx.x * kCompactBlock + threadIdx.x;
    const bool on = p < n && mask[p] != 0;
    const unsigned long long votes = __ballot(on);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == 0u) wv[w] = (uint32_t)__popcll(votes);
    __syncthreads();
    if (!on) return;
    uint32_t base = blk[blockIdx.x];
    for (uint32_t k = 0; k < w; ++k) base += wv[k];
    list[base + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull))] = p;
}

#endif  /* HIP */

}  // namespace surfdev
