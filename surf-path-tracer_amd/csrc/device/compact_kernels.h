/*
 * compact_kernels.h -- the order-preserving compaction of a byte mask into the
 * ascending list of its nonzero pixels (include/surf_hip.h, "per-pixel sample
 * masks"): count, scan, scatter; no atomic, so the list does not depend on the
 * order the blocks arrive in.  Shared by the mask from the noise estimate
 * (adaptive_kernels.h) and the mask from the non-local-means filter's error
 * estimate (error_mask_kernels.h).  No reference counterpart.
 */
#pragma once
#include "types.h"

namespace surfdev {

constexpr uint32_t kCompactBlock = 256;      /* pixels per block of the compaction */

#if defined(__HIPCC__) || defined(__HIP__)

/* Before the compaction of a context's mask under a surfel sensor: mask[p] = 0
 * where the texel is invalid (valid[p] == 0); every other byte is left as built. */
static __global__ __launch_bounds__(kCompactBlock) void k_mask_and_valid(uint8_t* __restrict__ mask, const uint8_t* __restrict__ valid,
                                                                         uint32_t n) {
    const uint32_t p = blockIdx.x * kCompactBlock + threadIdx.x;
    if (p < n && valid[p] == 0) mask[p] = 0;
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
