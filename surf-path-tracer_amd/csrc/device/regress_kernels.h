/*
 * regress_kernels.h -- the first-order feature regression filter for stills
 * (surf_denoise_regress*, include/surf_hip.h gives the arithmetic): a weighted
 * local regression of each half image's colour on the feature planes (normal,
 * albedo, relative depth, 1), the weights the non-local-means filter's
 * cross-half patch weights (Moon et al. 2014; Bitterli et al. 2016 in the
 * non-collaborative form), evaluated at the centre pixel.  No reference
 * counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states.  Prepare, the distance images, the patch sums and the
 * weights are nlm_kernels.h's functions.  What is added is written once, in
 * the SURF_HD functions below: regressPack (the feature record of a pixel),
 * regressPhi (a tap's features against the centre), regressTap / regressTap0
 * (the normal equations' sums of order one and order zero), regressSolve (the
 * ridge, the elimination, the fallback).  The walk over the taps is
 * nlm_kernels.h's too, in both its forms: RegressTaps is the consumer that
 * says which taps the regression takes and adds them to the normal
 * equations, from feature planes in memory (regressPixel: the global kernel
 * and the host twin) or from the staged kernel's LDS copy of them: identical
 * bits.
 */
#pragma once
#include "nlm_kernels.h"

namespace surfdev {

/* what the host computes once per call */
struct RegressConsts {
    NlmConsts n;
    float ridge;
};

constexpr int kRegressDim = 8;                    /* seven features and the constant, which goes last */
constexpr int kRegressTri = kRegressDim * (kRegressDim + 1) / 2;
/* the packed upper triangle: entry (i, j), i <= j */
SURF_HD constexpr int regressIdx(int i, int j) { return i * kRegressDim - i * (i - 1) / 2 + (j - i); }

/* The staged kernel's dynamic LDS, stated once for the host and the device:
 * the non-local-means layout's two float4 record planes of the tile with its
 * halo of r + f, then the feature records of the tile with its halo of r as
 * two float4 planes -- (N, albedo.x), (albedo.y, albedo.z, position.w, hit):
 * 32 bytes a texel -- then the float2 plane of the records and the distance
 * image as in nlmLdsBytes.  43.9 + 24.2 KB at the defaults. */
SURF_HD size_t regressFeatTexels(int r) { return (size_t)nlmTileW(r) * nlmTileH(r); }
SURF_HD size_t regressLdsBytes(int r, int f) { return nlmLdsBytes(r, f) + 2 * sizeof(float4) * regressFeatTexels(r); }
/* The staged variant is taken while its layout fits the 160 KiB of a compute
 * unit; above, the global one.  The kernel's registers (129..256 a lane) leave
 * room for two waves a SIMD, that is for two of its 256-thread workgroups, and
 * up to 80 KiB -- the defaults, (6, 2), (7, 1) -- two are resident; from (6, 3),
 * 84,416 B, one is.  One staged workgroup a compute unit still measured 3.3 times faster
 * than the global kernel at (7, 3) and at (10, 3), the largest layout the
 * parameter ranges allow (129,728 B): at these ranges nothing is past the bound
 * (MEASUREMENTS "First-order regression"). */
constexpr size_t kRegressLdsMax = 160 * 1024;

/* the feature record of a pixel from the three planes as surf_read_aov defines them */
SURF_HD void regressPack(float4 pos, float4 nrm, float4 alb, float4& F0, float4& F1) {
    F0 = make_float4(nrm.x, nrm.y, nrm.z, alb.x);
    F1 = make_float4(alb.y, alb.z, pos.w, alb.w != 0.0f ? 1.0f : 0.0f);
}

/* the features of tap q against the centre p; whether the seven differences are all finite */
SURF_HD bool regressPhi(float4 P0, float4 P1, float4 Q0, float4 Q1, float* phi) {
    phi[0] = Q0.x - P0.x;
    phi[1] = Q0.y - P0.y;
    phi[2] = Q0.z - P0.z;
    phi[3] = Q0.w - P0.w;
    phi[4] = Q1.x - P1.x;
    phi[5] = Q1.y - P1.y;
    phi[6] = (Q1.z - P1.z) / P1.z;
    phi[7] = 1.0f;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 7; ++i) ok = ok && nlmFinite(phi[i]);
    return ok;
}

/* the normal equations of one half of one pixel: A's upper triangle, b's three colour channels a row */
struct RegressAcc {
    float A[kRegressTri];
    float b[3 * kRegressDim];
};
SURF_HD void regressZero(RegressAcc& a) {
#pragma unroll
    for (int i = 0; i < kRegressTri; ++i) a.A[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < 3 * kRegressDim; ++i) a.b[i] = 0.0f;
}

/* one accepted tap of a hit centre, both halves: the products phi_i * phi_j are shared */
SURF_HD void regressTap(RegressAcc& a0, RegressAcc& a1, float w0, float w1, const float* phi, float4 Cq0, float4 Cq1) {
#pragma unroll
    for (int i = 0; i < kRegressDim; ++i) {
#pragma unroll
        for (int j = i; j < kRegressDim; ++j) {
            const float pp = phi[i] * phi[j];
            a0.A[regressIdx(i, j)] = a0.A[regressIdx(i, j)] + w0 * pp;
            a1.A[regressIdx(i, j)] = a1.A[regressIdx(i, j)] + w1 * pp;
        }
        const float u0 = w0 * phi[i], u1 = w1 * phi[i];
        a0.b[3 * i + 0] = a0.b[3 * i + 0] + u0 * Cq0.x;
        a0.b[3 * i + 1] = a0.b[3 * i + 1] + u0 * Cq0.y;
        a0.b[3 * i + 2] = a0.b[3 * i + 2] + u0 * Cq0.z;
        a1.b[3 * i + 0] = a1.b[3 * i + 0] + u1 * Cq1.x;
        a1.b[3 * i + 1] = a1.b[3 * i + 1] + u1 * Cq1.y;
        a1.b[3 * i + 2] = a1.b[3 * i + 2] + u1 * Cq1.z;
    }
}
/* one accepted tap of a miss centre: order zero, the last row alone -- nlmTap's sums */
SURF_HD void regressTap0(RegressAcc& a0, RegressAcc& a1, float w0, float w1, float4 Cq0, float4 Cq1) {
    constexpr int d = regressIdx(7, 7);
    a0.A[d] = a0.A[d] + w0;
    a1.A[d] = a1.A[d] + w1;
    a0.b[21] = a0.b[21] + w0 * Cq0.x;
    a0.b[22] = a0.b[22] + w0 * Cq0.y;
    a0.b[23] = a0.b[23] + w0 * Cq0.z;
    a1.b[21] = a1.b[21] + w1 * Cq1.x;
    a1.b[22] = a1.b[22] + w1 * Cq1.y;
    a1.b[23] = a1.b[23] + w1 * Cq1.z;
}

/* The prediction at the centre from one half's sums (which it overwrites).
 * order1: the ridge, then the elimination k = 0..6 -- the pivot d_k = A_kk,
 * l_i = A_ki / d_k for the rows i below, A_ij = A_ij - l_i * A_kj and
 * b_ic = b_ic - l_i * b_kc -- and beta = b_7 / A_77 of what is left; order
 * zero where a pivot or beta is not usable, and for a miss centre. */
SURF_HD V3 regressSolve(RegressAcc& a, float ridge, bool order1) {
    constexpr int last = regressIdx(7, 7);
    const float sw = a.A[last];
    const V3 zero = mk3(a.b[21] / sw, a.b[22] / sw, a.b[23] / sw);
    if (!order1) return zero;
#pragma unroll
    for (int j = 0; j < 7; ++j) a.A[regressIdx(j, j)] = a.A[regressIdx(j, j)] + ridge * sw;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float d = a.A[regressIdx(k, k)];
        ok = ok && nlmFinite(d) && d > 0.0f;
#pragma unroll
        for (int i = k + 1; i < kRegressDim; ++i) {
            const float l = a.A[regressIdx(k, i)] / d;
#pragma unroll
            for (int j = i; j < kRegressDim; ++j) a.A[regressIdx(i, j)] = a.A[regressIdx(i, j)] - l * a.A[regressIdx(k, j)];
#pragma unroll
            for (int c = 0; c < 3; ++c) a.b[3 * i + c] = a.b[3 * i + c] - l * a.b[3 * k + c];
        }
    }
    const float d7 = a.A[last];
    ok = ok && nlmFinite(d7) && d7 > 0.0f;
    const V3 beta = mk3(a.b[21] / d7, a.b[22] / d7, a.b[23] / d7);
    ok = ok && nlmFinite(beta.x) && nlmFinite(beta.y) && nlmFinite(beta.z);
    return ok ? beta : zero;
}

/* the two predictions as the sums nlmOutput divides: o_h = beta_h / 1.0f */
SURF_HD NlmSums regressSums(RegressAcc& a0, RegressAcc& a1, float ridge, bool order1) {
    NlmSums s;
    s.w0 = s.w1 = 1.0f;
    s.s0 = regressSolve(a0, ridge, order1);
    s.s1 = regressSolve(a1, ridge, order1);
    return s;
}

/* the three feature planes in memory (device global memory, host arrays) */
struct RegressFetchFeat {
    const float4 *P, *N, *A;
    int W;
    SURF_HD void feat(int x, int y, float4& F0, float4& F1) const {
        const size_t i = (size_t)y * W + x;
        regressPack(P[i], N[i], A[i], F0, F1);
    }
};

/* The regression as a consumer of nlm_kernels.h's walks (NlmTaps states the
 * interface), the feature records from feat: begin() zeroes the two halves'
 * sums and keeps the centre's feature record; a hit centre takes the taps
 * that are hits with finite features, at order one, a miss centre every tap,
 * at order zero. */
template <class Feat>
struct RegressTaps {
    Feat feat;
    RegressAcc a0, a1;
    float4 P0, P1;
    bool hit;
    float phi[kRegressDim];
    SURF_HD void begin(int x, int y, bool inside) {
        regressZero(a0);
        regressZero(a1);
        P0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        P1 = P0;
        if (inside) feat.feat(x, y, P0, P1);
        hit = P1.w != 0.0f;
    }
    SURF_HD bool take(int qx, int qy) {
        if (!hit) return true;
        float4 Q0, Q1;
        feat.feat(qx, qy, Q0, Q1);
        return Q1.w != 0.0f && regressPhi(P0, P1, Q0, Q1, phi);
    }
    SURF_HD void add(float w0, float w1, float4 Cq0, float4 Cq1) {
        if (hit) regressTap(a0, a1, w0, w1, phi, Cq0, Cq1);
        else regressTap0(a0, a1, w0, w1, Cq0, Cq1);
    }
    SURF_HD NlmSums sums(float ridge) { return regressSums(a0, a1, ridge, hit); }
};

/* the predictions of a colour-VALID pixel (x, y): the global kernel's and the host twin's pixel function */
template <class Fetch, class Feat>
SURF_HD NlmSums regressPixel(int x, int y, int W, int H, const RegressConsts& R, const Fetch& fetch, const Feat& feat) {
    RegressTaps<Feat> taps{feat};
    taps.begin(x, y, true);
    nlmWalk(x, y, W, H, R.n, fetch, taps);
    return taps.sums(R.ridge);
}

#if defined(__HIPCC__) || defined(__HIP__)

/* the feature records of the tile at (x0 + r, y0 + r) with its halo of r in LDS */
struct RegressLdsFeat {
    const float4 *F0, *F1;
    int w, x0, y0;
    __device__ __forceinline__ void feat(int x, int y, float4& Q0, float4& Q1) const {
        const int i = (y - y0) * w + (x - x0);
        Q0 = F0[i];
        Q1 = F1[i];
    }
};

/* ... and the staged walk's consumer: the feature records of the in-frame
 * part of the tile with its halo of r staged beside the walk's planes
 * (regressLdsBytes).  A tap reads its two feature records from there,
 * consecutive lanes consecutive 16-byte texels of a plane's row; the centre's
 * feature record stays in registers. */
struct RegressStagedTaps : RegressTaps<RegressLdsFeat> {
    const float4 *P, *N, *A;
    __device__ __forceinline__ static size_t ldsFloat4s(const NlmConsts& K) { return 2 * regressFeatTexels(K.r); }
    __device__ __forceinline__ void stage(float4* lds, int bx, int by, int W, int H, const NlmConsts& K) {
        const int fw = nlmTileW(K.r), fx0 = bx - K.r, fy0 = by - K.r, ftexels = (int)regressFeatTexels(K.r);
        float4* tF0 = lds;
        float4* tF1 = tF0 + ftexels;
        for (int t = (int)threadIdx.x; t < ftexels; t += 256) {
            const int ly = t / fw, lx = t - ly * fw;
            const int gx = fx0 + lx, gy = fy0 + ly;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gy * W + gx;
                float4 F0, F1;
                regressPack(P[g], N[g], A[g], F0, F1);
                tF0[t] = F0;
                tF1[t] = F1;
            }
        }
        feat = RegressLdsFeat{tF0, tF1, fw, fx0, fy0};
    }
};

/* The filter: 256 threads on a 32 x 8 pixel tile, both halves in one launch
 * (the taps, the features and their products are shared by the two).
 * STAGED: nlmWalkStaged with the feature records staged beside its planes.
 * Not STAGED: regressPixel on global memory.
 * At most two waves a SIMD: the 120 sums of a pixel's two halves stay in registers. */
template <bool STAGED>
__global__ __launch_bounds__(256, 2) void k_regress(const float4* __restrict__ C0, const float4* __restrict__ C1, const float4* __restrict__ V,
                                                    const float4* __restrict__ H0, const float4* __restrict__ H1,
                                                    const float4* __restrict__ P, const float4* __restrict__ N,
                                                    const float4* __restrict__ A, float4* __restrict__ out, float4* __restrict__ err,
                                                    int W, int H, RegressConsts R) {
    extern __shared__ float4 regressTile[];
    const TilePixel px = tilePixel(W, H);
    NlmSums s = nlmZero();
    bool valid = false;
    if (STAGED) {
        RegressStagedTaps taps;
        taps.P = P, taps.N = N, taps.A = A;
        valid = nlmWalkStaged(regressTile, px, C0, C1, V, W, H, R.n, taps);
        if (!px.inside) return;
        if (valid) s = taps.sums(R.ridge);
    } else {
        if (!px.inside) return;
        valid = C0[px.p].w != 0.0f;
        if (valid) s = regressPixel(px.x, px.y, W, H, R, NlmFetchPlanes{C0, C1, V, W}, RegressFetchFeat{P, N, A, W});
    }
    float4 o, e;
    nlmOutput(valid, H0[px.p], H1[px.p], s, o, e);
    out[px.p] = o;
    err[px.p] = e;
}

#endif  /* HIP */

}  // namespace surfdev
