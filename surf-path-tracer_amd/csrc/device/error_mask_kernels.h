/*
 * error_mask_kernels.h -- the active-pixel mask from the non-local-means
 * filter's error estimate (surf_error_mask_image, surf_mask_from_nlm;
 * include/surf_hip.h gives the arithmetic): the relative error of a pixel, its
 * box mean, the raw flag, and the one kernel that stages, sums, flags and
 * dilates on a tile.  The compaction of the byte mask is compact_kernels.h's.  No
 * reference counterpart.
 *
 * errorRel, errorBox, errorRaw and errorActive below are the only place the
 * rule is written; the kernel and the host twin call them on the same values.
 */
#pragma once
#include "compact_kernels.h"
#include "denoise_kernels.h"        /* the 32 x 8 tile */
#include "types.h"

namespace surfdev {

constexpr int kErrorMaxSmooth = 3, kErrorMaxDilate = 2;
constexpr int kErrorMaxHalo = kErrorMaxSmooth + kErrorMaxDilate;
/* the LDS of a tile: the relative errors of the tile and its halo of smooth +
 * dilate (42 x 18 floats), the row sums of the tile and its halo of dilate
 * across, smooth + dilate down (36 x 18 floats), the raw flags of the tile and
 * its halo of dilate (36 x 12 bytes): 6048 B */
constexpr int kErrorRelW = kDenoiseTileW + 2 * kErrorMaxHalo, kErrorRelH = kDenoiseTileH + 2 * kErrorMaxHalo;
constexpr int kErrorRawW = kDenoiseTileW + 2 * kErrorMaxDilate, kErrorRawH = kDenoiseTileH + 2 * kErrorMaxDilate;

/* the parameters as the kernel takes them: tt = threshold * threshold,
 * ff = floor * floor, cnt = (float)((2 smooth + 1)^2), all taken on the host */
struct ErrorRule {
    float tt, ff, cnt, minSamples, maxSamples;
    int smooth, dilate;
};

/* what the kernel adds up for the loop's summary: integer adds and an integer
 * max, whatever order the blocks arrive in */
struct ErrorStats {
    uint32_t above;       /* pixels with A.w >= min_samples and !(S <= tt) */
    uint32_t maxKey;      /* the largest errorKey(S) of a non-NaN S; 0: there is none */
};

SURF_HD int errorClamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

/* the relative squared error of a pixel: the filter's estimate over the filtered colour's square */
SURF_HD float errorRel(float4 o, float4 e, const ErrorRule& R) {
    const float num = (e.x + e.y) + e.z;
    const float den = (((o.x * o.x) + (o.y * o.y)) + (o.z * o.z)) + R.ff;
    return num / den;
}

/* S at (x, y): rel(ux, uy) is the relative error at an unclamped texel -- the
 * value at the texel clamped to the frame.  Rows first, then the column of
 * row sums. */
template <class Rel>
SURF_HD float errorBox(int x, int y, const ErrorRule& R, const Rel& rel) {
    if (R.smooth == 0) return rel(x, y);
    float S = 0.0f;
    for (int j = -R.smooth; j <= R.smooth; ++j) {
        float row = 0.0f;
        for (int i = -R.smooth; i <= R.smooth; ++i) row = row + rel(x + i, y + j);
        S = S + row;
    }
    return S / R.cnt;
}

/* A pixel that wants more samples on its own account: too few of them, or a
 * smoothed error that is not known to be at most the threshold's square (a NaN counts). */
SURF_HD bool errorLoud(float S, const ErrorRule& R) { return !(S <= R.tt); }
SURF_HD bool errorRaw(float w, float S, const ErrorRule& R) { return !(w >= R.minSamples) || errorLoud(S, R); }
/* ... and whether it gets them: a raw pixel within `dilate`, and room below the cap. */
SURF_HD bool errorActive(bool anyRaw, float w, const ErrorRule& R) { return anyRaw && w < R.maxSamples; }

/* an unsigned key that orders non-NaN floats as the floats are ordered (-0 below +0), never 0 */
SURF_HD uint32_t errorKey(float S) {
    uint32_t b;
    __builtin_memcpy(&b, &S, sizeof b);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
SURF_HD float errorFromKey(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    float S;
    __builtin_memcpy(&S, &b, sizeof S);
    return S;
}

#if defined(__HIPCC__) || defined(__HIP__)

/* The byte mask of a W x H frame: 256 threads on a 32 x 8 pixel tile, the grid
 * covering partial tiles.  With s = smooth, d = dilate:
 *   1. the relative errors of the tile and its halo of s + d go to LDS, each
 *      texel clamped to the frame, from the texel's out and err records (the
 *      halo's records are read again by the neighbouring tiles, out of L2: a
 *      pointwise pre-pass that wrote rel to a plane first measured slower,
 *      MEASUREMENTS "Error-driven adaptive sampling");
 *   2. barrier; the row sums of the (32 + 2d) x (8 + 2s + 2d) texels that the
 *      raw flags' columns read;
 *   3. barrier; the raw flag of each texel of the tile and its halo of d that
 *      lies in the frame (0 outside it): the column of 2s + 1 row sums over
 *      cnt, against tt, and the texel's own sample count.  A texel of the tile
 *      itself also votes for the summary where one is asked for;
 *   4. barrier; a pixel ORs the (2d + 1)^2 bytes around it and writes its byte.
 * With s = 0 step 2 copies and step 3 takes the value as it is (S is rel).
 * Every LDS index is below the static sizes for s <= 3, d <= 2; every global
 * read is at a texel clamped to the frame.  Rows of 32 lanes read consecutive
 * words or bytes of LDS. */
static __global__ __launch_bounds__(256) void k_error_mask(const float4* __restrict__ out, const float4* __restrict__ err,
                                                           const float4* __restrict__ A, uint8_t* __restrict__ mask, int W, int H,
                                                           ErrorRule R, ErrorStats* __restrict__ stats) {
    __shared__ float rel[kErrorRelW * kErrorRelH];
    __shared__ float rows[kErrorRawW * kErrorRelH];
    __shared__ uint8_t raw[kErrorRawW * kErrorRawH];
    __shared__ uint32_t vote[2];
    const int s = R.smooth, d = R.dilate, hs = s + d;
    const int bx = (int)blockIdx.x * kDenoiseTileW, by = (int)blockIdx.y * kDenoiseTileH;
    if (threadIdx.x < 2) vote[threadIdx.x] = 0u;
    /* 1. rel, LDS texel (lx, ly) = frame texel clamp(bx - hs + lx, by - hs + ly) */
    const int rw = kDenoiseTileW + 2 * hs, rh = kDenoiseTileH + 2 * hs;
    for (int t = (int)threadIdx.x; t < rw * rh; t += 256) {
        const int ly = t / rw, lx = t - ly * rw;
        const size_t g = (size_t)errorClamp(by - hs + ly, H) * W + errorClamp(bx - hs + lx, W);
        rel[ly * kErrorRelW + lx] = errorRel(out[g], err[g], R);
    }
    __syncthreads();
    /* 2. row sums, LDS texel (lx, ly) = frame texel (bx - d + lx, by - hs + ly), unclamped */
    const int fw = kDenoiseTileW + 2 * d;
    for (int t = (int)threadIdx.x; t < fw * rh; t += 256) {
        const int ly = t / fw, lx = t - ly * fw;
        float row = 0.0f;
        if (s == 0) row = rel[ly * kErrorRelW + lx];
        else
            for (int i = 0; i <= 2 * s; ++i) row = row + rel[ly * kErrorRelW + lx + i];
        rows[ly * kErrorRawW + lx] = row;
    }
    __syncthreads();
    /* 3. raw flags, LDS texel (lx, ly) = frame texel (bx - d + lx, by - d + ly) */
    const int fh = kDenoiseTileH + 2 * d;
    for (int t = (int)threadIdx.x; t < fw * fh; t += 256) {
        const int ly = t / fw, lx = t - ly * fw;
        const int gx = bx - d + lx, gy = by - d + ly;
        uint8_t f = 0;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            float S;
            if (s == 0) S = rows[ly * kErrorRawW + lx];
            else {
                S = 0.0f;
                for (int j = 0; j <= 2 * s; ++j) S = S + rows[(ly + j) * kErrorRawW + lx];
                S = S / R.cnt;
            }
            const float w = A[(size_t)gy * W + gx].w;
            f = errorRaw(w, S, R) ? 1 : 0;
            if (stats && lx >= d && lx < d + kDenoiseTileW && ly >= d && ly < d + kDenoiseTileH) {
                if (w >= R.minSamples && errorLoud(S, R)) atomicAdd(&vote[0], 1u);
                if (S == S) atomicMax(&vote[1], errorKey(S));
            }
        }
        raw[ly * kErrorRawW + lx] = f;
    }
    __syncthreads();
    if (stats && threadIdx.x == 0) {
        if (vote[0]) atomicAdd(&stats->above, vote[0]);
        if (vote[1]) atomicMax(&stats->maxKey, vote[1]);
    }
    /* 4. dilate */
    const int tx = (int)(threadIdx.x & (kDenoiseTileW - 1)), ty = (int)(threadIdx.x / kDenoiseTileW);
    const int x = bx + tx, y = by + ty;
    if (x >= W || y >= H) return;
    uint32_t any = 0;
    for (int dy = 0; dy <= 2 * d; ++dy)
        for (int dx = 0; dx <= 2 * d; ++dx) any |= raw[(ty + dy) * kErrorRawW + (tx + dx)];
    const size_t p = (size_t)y * W + x;
    mask[p] = errorActive(any != 0u, A[p].w, R) ? 1 : 0;
}

#endif  /* HIP */

}  // namespace surfdev
