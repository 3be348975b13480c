/*
 * svgf_kernels.h -- the variance-guided filter (surf_svgf*, include/surf_hip.h
 * gives the arithmetic): the piece of SVGF (Schied et al. 2017) that joins the
 * temporal accumulation to the a-trous filter.  The luminance moments ride
 * k_temporal<true> (temporal_kernels.h); here are the per-pixel variance
 * estimate and the a-trous level whose colour edge-stopping width is that
 * variance; and the filter's two optional stages (surf_svgf_ext): the firefly
 * clamp in front of the accumulation (k_firefly) and the feedback of the
 * first filtered iteration into the history (a switch on k_atrous_var).  No
 * reference counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states.  svgfVariancePixel and denoisePixelVar below are the only
 * place it is written; the staged kernels, the global-memory kernels and the
 * host twin (surf_svgf_image_host) differ only in the Fetch object that hands
 * them their taps, as denoisePixel's callers do.
 */
#pragma once
#include "denoise_kernels.h"
#include "surf_math.h"
#include "temporal_kernels.h"       /* svgfLum */
#include "types.h"

namespace surfdev {

constexpr int kSvgfVarRadius = 3;                                   /* the 7 x 7 spatial estimate */
constexpr int kSvgfVarTileW = kDenoiseTileW + 2 * kSvgfVarRadius;   /* 38 */
constexpr int kSvgfVarTileH = kDenoiseTileH + 2 * kSvgfVarRadius;   /* 14 */
/* the staged variance kernel's LDS: normal, position and moments of the tile
 * and its halo of 3 -- 3 x 16 B x 38 x 14 = 25 536 B */
constexpr size_t kSvgfVarLdsBytes = (size_t)3 * sizeof(float4) * kSvgfVarTileW * kSvgfVarTileH;

/* per call, computed in f32 on the host as the header states */
struct SvgfConsts {
    float kn, kp;                /* 1 / sigma_normal^2, 1 / sigma_plane^2, as the denoiser's */
    float sigmaLum, varEps;
    float spatialBelow;          /* (float)spatial_below */
};

/* The variance of a VALID pixel (x, y) whose moments are Mp = (mu1', mu2', m', 0):
 * temporal where the moments' history is long enough, else the guide-weighted
 * 7 x 7 spatial estimate, boosted.  fetch.n / .p / .m (qx, qy) return the
 * guide normal (w = validity), the guide position and the moments of an
 * in-frame texel; position of a skipped tap is never fetched. */
template <class Fetch>
SURF_HD float svgfVariancePixel(int x, int y, int W, int H, const SvgfConsts& K, float4 Mp, float4 Np, float4 Pp, const Fetch& fetch) {
    if (Mp.z >= K.spatialBelow) {
        const float v = Mp.y - Mp.x * Mp.x;
        return v > 0.0f ? v : 0.0f;
    }
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int dy = -kSvgfVarRadius; dy <= kSvgfVarRadius; ++dy) {
        const int qy = y + dy;
#pragma unroll
        for (int dx = -kSvgfVarRadius; dx <= kSvgfVarRadius; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float4 Nq = fetch.n(qx, qy);
            if (Nq.w == 0.0f) continue;
            const float4 Mq = fetch.m(qx, qy);
            if (Mq.z == 0.0f) continue;
            const float4 Pq = fetch.p(qx, qy);
            const float nx = Nq.x - Np.x, ny = Nq.y - Np.y, nz = Nq.z - Np.z;
            const float dn = (nx * nx + ny * ny) + nz * nz;
            const float px = Pq.x - Pp.x, py = Pq.y - Pp.y, pz = Pq.z - Pp.z;
            const float pl = (px * Np.x + py * Np.y) + pz * Np.z;
            const float dp = pl * pl;
            float e = dn * K.kn + dp * K.kp;
            e = e < 100.0f ? e : 100.0f;
            const float wq = gExpf(-e);
            sw = sw + wq;
            s1 = s1 + wq * Mq.x;
            s2 = s2 + wq * Mq.y;
        }
    }
    if (!(sw > 0.0f)) return 0.0f;
    const float a1 = s1 / sw, a2 = s2 / sw;
    float v = a2 - a1 * a1;
    v = v > 0.0f ? v : 0.0f;
    const float boost = K.spatialBelow / (Mp.z > 1.0f ? Mp.z : 1.0f);
    return v * boost;
}

/* Level 0 of the filtered image: (r / den, v), r the temporal blend; an
 * invalid pixel has den = 1 and v = 0, i.e. (c, 0). */
SURF_HD float4 svgfLevel0(float4 r, float4 alb, uint32_t demodulate, float v) {
    const V3 den = denoiseDen(alb, demodulate);
    return make_float4(r.x / den.x, r.y / den.y, r.z / den.z, alb.w != 0.0f ? v : 0.0f);
}

/* One variance-guided a-trous level at a VALID pixel: denoisePixel with the
 * colour term replaced by the luminance difference over the 3 x 3
 * prefiltered standard deviation, the variance (the image's w) filtered
 * along with the weights squared.  The same Fetch objects as denoisePixel. */
template <class Fetch>
SURF_HD float4 denoisePixelVar(int x, int y, int W, int H, int s, const SvgfConsts& K, float4 Ip, float4 Np, float4 Pp, const Fetch& fetch) {
    const float g[3] = {0.25f, 0.5f, 0.25f};                  /* g (x) g = {1/16, 1/8, 1/16; 1/8, 1/4, 1/8; ...}, exact products */
    float gs = 0.0f, gw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            if (fetch.n(qx, qy).w == 0.0f) continue;
            const float gk = g[dy + 1] * g[dx + 1];
            gs = gs + gk * fetch.i(qx, qy).w;
            gw = gw + gk;
        }
    }
    const float gv = gs / gw;                                  /* the centre tap makes gw > 0 */
    const float kl = 1.0f / (K.sigmaLum * sqrtf(gv) + K.varEps);
    const float lp = svgfLum(Ip.x, Ip.y, Ip.z);
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sumW = 0.0f, sumV = 0.0f;
    V3 sum = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * s;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s;
            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float4 Nq = fetch.n(qx, qy);
            if (Nq.w == 0.0f) continue;
            const float4 Iq = fetch.i(qx, qy);
            const float4 Pq = fetch.p(qx, qy);
            const float dl = fabsf(svgfLum(Iq.x, Iq.y, Iq.z) - lp);
            const float nx = Nq.x - Np.x, ny = Nq.y - Np.y, nz = Nq.z - Np.z;
            const float dn = (nx * nx + ny * ny) + nz * nz;
            const float px = Pq.x - Pp.x, py = Pq.y - Pp.y, pz = Pq.z - Pp.z;
            const float pl = (px * Np.x + py * Np.y) + pz * Np.z;
            const float dp = pl * pl;
            float e = (dl * kl + dn * K.kn) + dp * K.kp;
            e = e < 100.0f ? e : 100.0f;                 /* NaN -> 100 */
            const float w = (h[dy + 2] * h[dx + 2]) * gExpf(-e);
            sumW = sumW + w;
            sum.x = sum.x + w * Iq.x;
            sum.y = sum.y + w * Iq.y;
            sum.z = sum.z + w * Iq.z;
            sumV = sumV + (w * w) * Iq.w;
        }
    }
    return make_float4(sum.x / sumW, sum.y / sumW, sum.z / sumW, sumV / (sumW * sumW));
}

/* The image an iteration writes: the next level (rgb, variance) -- an invalid
 * pixel's level copied through -- and on the last iteration the remodulated
 * output (I_n * den, 1).  var: the variance leaving the filter (0 where invalid). */
SURF_HD float4 svgfStore(bool valid, float4 Ip, float4 filtered, bool last, float4 alb, uint32_t demodulate, float& var) {
    const float4 v = valid ? filtered : Ip;
    var = valid ? v.w : 0.0f;
    if (!last) return v;
    if (!valid) return make_float4(v.x, v.y, v.z, 1.0f);
    const V3 den = denoiseDen(alb, demodulate);
    return make_float4(v.x * den.x, v.y * den.y, v.z * den.z, 1.0f);
}

/* Filtered-history feedback: the history record of a VALID pixel after
 * iteration 0 -- the level that iteration wrote, remodulated, with the history
 * length n1 the temporal accumulation gave the pixel. */
SURF_HD float4 svgfFeedback(float4 filtered, float4 alb, uint32_t demodulate, float n1) {
    const V3 den = denoiseDen(alb, demodulate);
    return make_float4(filtered.x * den.x, filtered.y * den.y, filtered.z * den.z, n1);
}

/* ---- stage 0, the firefly clamp (surf_svgf_ext.firefly_scale, surf_firefly_image) ----
 * A pixel's luminance of c / den is clamped to firefly_scale times the largest
 * among its usable 3 x 3 neighbours; the accumulator the later stages read
 * becomes A' = (c', 1).  fireflyLum and fireflyPixel are the only place this
 * arithmetic is written; k_firefly and the host twin differ in the Fetch. */
constexpr int kFireflyTileW = kDenoiseTileW + 2, kFireflyTileH = kDenoiseTileH + 2;      /* 34 x 10: the tile and its halo of 1 */
constexpr int kFireflyHalo = kFireflyTileW * kFireflyTileH - kDenoiseTileW * kDenoiseTileH;   /* 84 texels */
/* k_firefly's LDS: one float per texel, 1 360 B, static */
constexpr size_t kFireflyLdsBytes = sizeof(float) * kFireflyTileW * kFireflyTileH;
/* what a tap reads of a pixel that is not usable (invalid, or without a sample) */
constexpr float kFireflyNoTap = -1.0f;

/* c and l = lum(c / den) of a pixel, and, returned, what a neighbour's tap
 * reads of it: kFireflyNoTap where it is not usable, else l with everything
 * that cannot raise a maximum that starts at 0 -- l <= 0, a NaN -- stored as
 * 0: the tap counts and leaves mx alone, exactly as the comparison would. */
SURF_HD float fireflyLum(float4 A, float4 alb, uint32_t demodulate, V3& c, float& l) {
    const float inv = A.w > 0.0f ? 1.0f / A.w : 0.0f;
    c = mk3(A.x * inv, A.y * inv, A.z * inv);
    const V3 den = denoiseDen(alb, demodulate);
    l = svgfLum(c.x / den.x, c.y / den.y, c.z / den.z);
    if (!(alb.w != 0.0f && A.w > 0.0f)) return kFireflyNoTap;
    return l > 0.0f ? l : 0.0f;
}

/* A' of pixel (x, y): c, l and tap are fireflyLum's of this pixel; fetch.l
 * (qx, qy) returns fireflyLum's value of an in-frame neighbour. */
template <class Fetch>
SURF_HD float4 fireflyPixel(int x, int y, int W, int H, float scale, float4 A, V3 c, float l, float tap, const Fetch& fetch) {
    if (!(A.w > 0.0f)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float mx = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = x + dx;
            if ((dx == 0 && dy == 0) || qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
            const float lq = fetch.l(qx, qy);
            if (lq < 0.0f) continue;
            cnt = cnt + 1;
            mx = lq > mx ? lq : mx;
        }
    }
    const float lim = scale * mx;
    if (tap >= 0.0f && cnt > 0 && l > lim) {                 /* a NaN l fails and stays */
        const float f = lim / l;
        c = mk3(c.x * f, c.y * f, c.z * f);
    }
    return make_float4(c.x, c.y, c.z, 1.0f);
}

/* taps of the clamp from a full-frame plane of fireflyLum's values (the host twin) */
struct FireflyFetchPlane {
    const float* L;
    int W;
    SURF_HD float l(int qx, int qy) const { return L[(size_t)qy * W + qx]; }
};

/* taps of the variance estimate from full-frame planes in memory */
struct SvgfFetchPlanes {
    const float4* N;
    const float4* P;
    const float4* M;
    int W;
    SURF_HD float4 n(int qx, int qy) const { return N[(size_t)qy * W + qx]; }
    SURF_HD float4 p(int qx, int qy) const { return P[(size_t)qy * W + qx]; }
    SURF_HD float4 m(int qx, int qy) const { return M[(size_t)qy * W + qx]; }
};

#if defined(__HIPCC__) || defined(__HIP__)

/* ... and from the staged tile: three planes of kSvgfVarTileW x kSvgfVarTileH
 * texels whose texel (0, 0) is frame pixel (x0, y0) */
struct SvgfFetchTile {
    const float4* N;
    const float4* P;
    const float4* M;
    int x0, y0;
    __device__ __forceinline__ float4 n(int qx, int qy) const { return N[(qy - y0) * kSvgfVarTileW + (qx - x0)]; }
    __device__ __forceinline__ float4 p(int qx, int qy) const { return P[(qy - y0) * kSvgfVarTileW + (qx - x0)]; }
    __device__ __forceinline__ float4 m(int qx, int qy) const { return M[(qy - y0) * kSvgfVarTileW + (qx - x0)]; }
};

/* ... and of the clamp from the staged tile of kFireflyTileW x kFireflyTileH
 * floats whose texel (0, 0) is frame pixel (x0, y0) */
struct FireflyFetchTile {
    const float* L;
    int x0, y0;
    __device__ __forceinline__ float l(int qx, int qy) const { return L[(qy - y0) * kFireflyTileW + (qx - x0)]; }
};

/* The firefly clamp: 256 threads on a 32 x 8 pixel tile, the grid covering
 * partial tiles.  Every thread loads its pixel's accumulator and albedo (two
 * 16-byte loads, consecutive lanes consecutive records) and stores
 * fireflyLum's tap value in a 34 x 10 tile of floats in static LDS
 * (kFireflyLdsBytes); the first 84 threads also fill one texel each of the
 * halo of 1 -- top row, bottom row, left and right column.  Every texel
 * outside the frame holds kFireflyNoTap and is never loaded from memory.
 * After the one barrier the 8 taps come from LDS: a row of 32 lanes reads 32
 * consecutive floats, conflict-free.  48 B of memory traffic per pixel.  One
 * variant: at 1.4 KB there is no LDS to trade against. */
static __global__ __launch_bounds__(256) void k_firefly(const float4* __restrict__ A, const float4* __restrict__ alb,
                                                 float4* __restrict__ out, int W, int H, float scale, uint32_t demodulate) {
    __shared__ float ffTile[kFireflyTileW * kFireflyTileH];
    const int tx = (int)(threadIdx.x & (kDenoiseTileW - 1)), ty = (int)(threadIdx.x / kDenoiseTileW);
    const int bx = (int)blockIdx.x * kDenoiseTileW, by = (int)blockIdx.y * kDenoiseTileH;
    const int x = bx + tx, y = by + ty;
    const int x0 = bx - 1, y0 = by - 1;
    const bool inside = x < W && y < H;
    const size_t p = (size_t)y * W + x;
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    V3 c = mk3(0.0f, 0.0f, 0.0f);
    float l = 0.0f, tap = kFireflyNoTap;
    if (inside) {
        a = A[p];
        tap = fireflyLum(a, alb[p], demodulate, c, l);
    }
    ffTile[(ty + 1) * kFireflyTileW + (tx + 1)] = tap;
    if (threadIdx.x < (unsigned)kFireflyHalo) {
        const int t = (int)threadIdx.x;
        int lx, ly;
        if (t < 2 * kFireflyTileW) {                          /* the top row, then the bottom row */
            ly = t < kFireflyTileW ? 0 : kFireflyTileH - 1;
            lx = t < kFireflyTileW ? t : t - kFireflyTileW;
        } else {                                              /* the left column, then the right one */
            const int u = t - 2 * kFireflyTileW;
            lx = u < kDenoiseTileH ? 0 : kFireflyTileW - 1;
            ly = 1 + (u < kDenoiseTileH ? u : u - kDenoiseTileH);
        }
        const int gx = x0 + lx, gy = y0 + ly;
        float ht = kFireflyNoTap;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            V3 hc;
            float hl;
            ht = fireflyLum(A[g], alb[g], demodulate, hc, hl);
        }
        ffTile[ly * kFireflyTileW + lx] = ht;
    }
    __syncthreads();
    if (!inside) return;
    const FireflyFetchTile fetch{ffTile, x0, y0};
    out[p] = fireflyPixel(x, y, W, H, scale, a, c, l, tap, fetch);
}

/* Elementwise: the packed guides of n pixels, as denoisePrepare packs them. */
static __global__ __launch_bounds__(256) void k_svgf_guides(const float4* __restrict__ pos, const float4* __restrict__ nrm,
                                                     const float4* __restrict__ alb, uint32_t n, float4* __restrict__ gN,
                                                     float4* __restrict__ gP) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const float4 a = alb[p], nr = nrm[p], ps = pos[p];
    gN[p] = make_float4(nr.x, nr.y, nr.z, a.w != 0.0f ? 1.0f : 0.0f);
    gP[p] = make_float4(ps.x, ps.y, ps.z, 0.0f);
}

/* The variance estimate and level 0: 256 threads on a 32 x 8 pixel tile, the
 * grid covering partial tiles.  STAGED: the block first copies the in-frame
 * part of the tile and its halo of 3 -- 38 x 14 texels of normal, position
 * and moments -- into dynamic LDS (kSvgfVarLdsBytes) and takes centre and
 * taps from there; out-of-frame texels are left unwritten, svgfVariancePixel
 * never fetches them.  Rows of 32 lanes read consecutive 16-byte texels, as
 * k_atrous's tile: conflict-free.  Not STAGED: from global memory.  Both call
 * svgfVariancePixel on the same values: identical bits.  A tile whose pixels
 * all have a long history takes no tap at all; the staged copy is made
 * before that is known.  (The prologue and the staging loop are tilePixel's
 * and stageTile3's of denoise_kernels.h written out: through the helpers the
 * kernel compiled to five instructions fewer and one of its ten timed figures
 * came out over the parent's margin, MEASUREMENTS "Filters' home".) */
template <bool STAGED>
__global__ __launch_bounds__(256) void k_svgf_variance(const float4* __restrict__ R, const float4* __restrict__ alb,
                                                       const float4* __restrict__ gN, const float4* __restrict__ gP,
                                                       const float4* __restrict__ M, float4* __restrict__ I0,
                                                       float* __restrict__ var0, int W, int H, SvgfConsts K, uint32_t demodulate) {
    extern __shared__ float4 svTile[];
    const int tx = (int)(threadIdx.x & (kDenoiseTileW - 1)), ty = (int)(threadIdx.x / kDenoiseTileW);
    const int bx = (int)blockIdx.x * kDenoiseTileW, by = (int)blockIdx.y * kDenoiseTileH;
    const int x = bx + tx, y = by + ty;
    const bool inside = x < W && y < H;
    const size_t p = (size_t)y * W + x;
    float v = 0.0f;
    if (STAGED) {
        constexpr int tw = kSvgfVarTileW, th = kSvgfVarTileH;
        const int x0 = bx - kSvgfVarRadius, y0 = by - kSvgfVarRadius;
        float4* tN = svTile;
        float4* tP = svTile + tw * th;
        float4* tM = svTile + 2 * tw * th;
        for (int t = (int)threadIdx.x; t < tw * th; t += 256) {
            const int ly = t / tw, lx = t - ly * tw;
            const int gx = x0 + lx, gy = y0 + ly;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gy * W + gx;
                tN[t] = gN[g];
                tP[t] = gP[g];
                tM[t] = M[g];
            }
        }
        __syncthreads();
        if (!inside) return;
        const SvgfFetchTile fetch{tN, tP, tM, x0, y0};
        const float4 Np = fetch.n(x, y);
        if (Np.w != 0.0f) v = svgfVariancePixel(x, y, W, H, K, fetch.m(x, y), Np, fetch.p(x, y), fetch);
    } else {
        if (!inside) return;
        const SvgfFetchPlanes fetch{gN, gP, M, W};
        const float4 Np = gN[p];
        if (Np.w != 0.0f) v = svgfVariancePixel(x, y, W, H, K, M[p], Np, gP[p], fetch);
    }
    const float4 i0 = svgfLevel0(R[p], alb[p], demodulate, v);
    I0[p] = i0;
    var0[p] = i0.w;
}

/* One variance-guided a-trous iteration at step s: k_atrous with
 * denoisePixelVar -- the same tile, the same staged layout (the image's w
 * now carries the variance; the 3 x 3 prefilter's taps lie inside the 2*s >= 2
 * halo), the same bits staged or not.  `last` fuses the remodulation and
 * writes the variance leaving the filter to var1.
 * FEEDBACK (surf_svgf_ext.feedback, iteration 0 only): the level this launch
 * writes, remodulated, replaces the colour of a valid pixel's history --
 * hist(p) = (I_1.rgb * den, n'), n' as k_temporal left it; an invalid pixel's
 * record is not touched.  One more 16-byte load (alb, unless `last` reads it
 * anyway), a 4-byte load and a 16-byte store per valid pixel; the other
 * instantiations never touch hist. */
template <bool STAGED, bool FEEDBACK>
__global__ __launch_bounds__(256) void k_atrous_var(const float4* __restrict__ I, const float4* __restrict__ gN,
                                                    const float4* __restrict__ gP, const float4* __restrict__ alb,
                                                    float4* __restrict__ out, float* __restrict__ var1, int W, int H, int s,
                                                    SvgfConsts K, uint32_t demodulate, int last, float4* __restrict__ hist) {
    extern __shared__ float4 dnTile[];
    const TilePixel px = tilePixel(W, H);
    const int x = px.x, y = px.y;
    const size_t p = px.p;
    float4 Ip, Np, Pp;
    float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (STAGED) {
        const int tw = kDenoiseTileW + 4 * s, th = kDenoiseTileH + 4 * s, x0 = px.bx - 2 * s, y0 = px.by - 2 * s;
        float4* tN = dnTile;
        float4* tI = dnTile + tw * th;
        float4* tP = dnTile + 2 * tw * th;
        stageTile3(tN, tI, tP, gN, I, gP, x0, y0, tw, th, W, H);
        if (!px.inside) return;
        const DenoiseFetchTile fetch{tN, tI, tP, x0, y0, tw};
        Np = fetch.n(x, y);
        Ip = fetch.i(x, y);
        Pp = fetch.p(x, y);
        if (Np.w != 0.0f) f = denoisePixelVar(x, y, W, H, s, K, Ip, Np, Pp, fetch);
    } else {
        if (!px.inside) return;
        const DenoiseFetchPlanes fetch{I, gN, gP, W};
        Np = gN[p];
        Ip = I[p];
        Pp = gP[p];
        if (Np.w != 0.0f) f = denoisePixelVar(x, y, W, H, s, K, Ip, Np, Pp, fetch);
    }
    const float4 a = last ? alb[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float var;
    out[p] = svgfStore(Np.w != 0.0f, Ip, f, last != 0, a, demodulate, var);
    if (last) var1[p] = var;
    if (FEEDBACK && Np.w != 0.0f) hist[p] = svgfFeedback(f, last ? a : alb[p], demodulate, hist[p].w);
}

#endif  /* HIP */

}  // namespace surfdev
