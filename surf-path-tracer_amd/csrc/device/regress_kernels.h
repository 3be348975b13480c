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
 * ridge, the elimination, the fallback).  regressPixel strings them together
 * for a pixel whose every value comes from a Fetch object: the global kernel
 * and the host twin call it.  The staged kernel calls the same pieces around
 * its LDS copy of the tile: identical bits.
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

/* the prepared records and the three feature planes in memory (device global memory, host arrays) */
struct RegressFetchPlanes {
    NlmFetchPlanes nlm;
    const float4* P;
    const float4* N;
    const float4* A;
    SURF_HD float4 c(int g, int x, int y) const { return nlm.c(g, x, y); }
    SURF_HD float4 v(int x, int y) const { return nlm.v(x, y); }
    SURF_HD void feat(int x, int y, float4& F0, float4& F1) const {
        const size_t i = (size_t)y * nlm.W + x;
        regressPack(P[i], N[i], A[i], F0, F1);
    }
};

/* The predictions of a colour-VALID pixel (x, y), every value from fetch at
 * in-frame texels: the taps dy outer and dx inner, each tap's two patch
 * distances computed texel by texel as nlmPixel computes them. */
template <class Fetch>
SURF_HD NlmSums regressPixel(int x, int y, int W, int H, const RegressConsts& R, const Fetch& fetch) {
    const NlmConsts& K = R.n;
    RegressAcc a0, a1;
    regressZero(a0);
    regressZero(a1);
    float4 P0, P1;
    fetch.feat(x, y, P0, P1);
    const bool hit = P1.w != 0.0f;
    for (int dy = -K.r; dy <= K.r; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -K.r; dx <= K.r; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const float4 Cq0 = fetch.c(0, qx, qy);
            if (Cq0.w == 0.0f) continue;
            float phi[kRegressDim];
            if (hit) {
                float4 Q0, Q1;
                fetch.feat(qx, qy, Q0, Q1);
                if (Q1.w == 0.0f) continue;
                if (!regressPhi(P0, P1, Q0, Q1, phi)) continue;
            }
            const float4 Cq1 = fetch.c(1, qx, qy);
            const bool centre = dx == 0 && dy == 0;
            float D0 = 0.0f, D1 = 0.0f;
            if (!centre)
                nlmPatch(x, y, K.f, K.cnt, [&](int sx, int sy) {
                    const int ax = nlmClamp(sx, W), ay = nlmClamp(sy, H), bx = nlmClamp(sx + dx, W), by = nlmClamp(sy + dy, H);
                    const float4 Va = fetch.v(ax, ay), Vb = fetch.v(bx, by);
                    return make_float2(nlmDistance(fetch.c(0, ax, ay), fetch.c(0, bx, by), Va, Vb, K),
                                       nlmDistance(fetch.c(1, ax, ay), fetch.c(1, bx, by), Va, Vb, K));
                }, D0, D1);
            const float w0 = centre ? 1.0f : nlmWeight(D1);
            const float w1 = centre ? 1.0f : nlmWeight(D0);
            if (hit) regressTap(a0, a1, w0, w1, phi, Cq0, Cq1);
            else regressTap0(a0, a1, w0, w1, Cq0, Cq1);
        }
    }
    return regressSums(a0, a1, R.ridge, hit);
}

#if defined(__HIPCC__) || defined(__HIP__)

/* The filter: 256 threads on a 32 x 8 pixel tile, both halves in one launch
 * (the taps, the features and their products are shared by the two).
 * STAGED: as k_nlm<true> -- the prepared records of the tile with its halo of
 * r + f and each search offset's distance image in dynamic LDS -- and beside
 * them the feature records of the in-frame part of the tile with its halo of
 * r (regressLdsBytes).  A tap reads its two colour records and its two
 * feature records from there, consecutive lanes consecutive 16-byte texels of
 * a plane's row; the centre's feature record stays in registers.
 * Not STAGED: regressPixel on global memory.
 * At most two waves a SIMD: the 120 sums of a pixel's two halves stay in registers. */
template <bool STAGED>
__global__ __launch_bounds__(256, 2) void k_regress(const float4* __restrict__ C0, const float4* __restrict__ C1, const float4* __restrict__ V,
                                                    const float4* __restrict__ H0, const float4* __restrict__ H1,
                                                    const float4* __restrict__ P, const float4* __restrict__ N,
                                                    const float4* __restrict__ A, float4* __restrict__ out, float4* __restrict__ err,
                                                    int W, int H, RegressConsts R) {
    extern __shared__ float4 regressTile[];
    const NlmConsts& K = R.n;
    const TilePixel px = tilePixel(W, H);
    const int x = px.x, y = px.y;
    NlmSums s = nlmZero();
    bool valid = false;
    if (STAGED) {
        const int halo = K.r + K.f;
        const int tw = nlmTileW(halo), th = nlmTileH(halo), x0 = px.bx - halo, y0 = px.by - halo;
        const int fw = nlmTileW(K.r), fx0 = px.bx - K.r, fy0 = px.by - K.r, ftexels = (int)regressFeatTexels(K.r);
        const int dw = nlmTileW(K.f), dn = (int)nlmDistTexels(K.f), dx0 = px.bx - K.f, dy0 = px.by - K.f;
        const int texels = tw * th;
        float4* t0 = regressTile;
        float4* t1 = t0 + texels;
        float4* tF0 = t1 + texels;
        float4* tF1 = tF0 + ftexels;
        float2* tV = reinterpret_cast<float2*>(tF1 + ftexels);
        float2* tD = tV + texels;
        for (int t = (int)threadIdx.x; t < texels; t += 256) {
            const int ly = t / tw, lx = t - ly * tw;
            const int gx = x0 + lx, gy = y0 + ly;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t g = (size_t)gy * W + gx;
                const float4 vv = V[g];
                t0[t] = C0[g];
                t1[t] = C1[g];
                tV[t] = make_float2(vv.x, vv.y);
            }
        }
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
        __syncthreads();
        const auto var = [&](int i) { return make_float4(t1[i].w, tV[i].x, tV[i].y, 0.0f); };
        const auto at = [&](int qx, int qy) { return (qy - y0) * tw + (qx - x0); };
        const auto fat = [&](int qx, int qy) { return (qy - fy0) * fw + (qx - fx0); };
        /* the distance texels this thread computes for every offset, clamped to the frame */
        int ai[kNlmDistPerThread], sx[kNlmDistPerThread], sy[kNlmDistPerThread];
#pragma unroll
        for (int k = 0; k < kNlmDistPerThread; ++k) {
            const int t = (int)threadIdx.x + 256 * k;
            const int ly = t / dw, lx = t - ly * dw;
            sx[k] = dx0 + lx;
            sy[k] = dy0 + ly;
            ai[k] = t < dn ? at(nlmClamp(sx[k], W), nlmClamp(sy[k], H)) : -1;
        }
        valid = px.inside && t0[at(x, y)].w != 0.0f;
        float4 P0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), P1 = P0;
        if (px.inside) {
            P0 = tF0[fat(x, y)];
            P1 = tF1[fat(x, y)];
        }
        const bool hit = P1.w != 0.0f;
        RegressAcc a0, a1;
        regressZero(a0);
        regressZero(a1);
        for (int dy = -K.r; dy <= K.r; ++dy) {
            for (int dx = -K.r; dx <= K.r; ++dx) {
                const bool centre = dx == 0 && dy == 0;
                if (!centre) {
#pragma unroll
                    for (int k = 0; k < kNlmDistPerThread; ++k) {
                        if (ai[k] < 0) continue;
                        const int bi = at(nlmClamp(sx[k] + dx, W), nlmClamp(sy[k] + dy, H));
                        const float4 Va = var(ai[k]), Vb = var(bi);
                        tD[(int)threadIdx.x + 256 * k] =
                            make_float2(nlmDistance(t0[ai[k]], t0[bi], Va, Vb, K), nlmDistance(t1[ai[k]], t1[bi], Va, Vb, K));
                    }
                    __syncthreads();
                }
                const int qx = x + dx, qy = y + dy;
                if (valid && qx >= 0 && qx < W && qy >= 0 && qy < H) {
                    const int qi = at(qx, qy);
                    const float4 Cq0 = t0[qi];
                    bool take = Cq0.w != 0.0f;
                    float phi[kRegressDim];
                    if (take && hit) {
                        const int fi = fat(qx, qy);
                        const float4 Q1 = tF1[fi];
                        take = Q1.w != 0.0f && regressPhi(P0, P1, tF0[fi], Q1, phi);
                    }
                    if (take) {
                        float D0 = 0.0f, D1 = 0.0f;
                        if (!centre) nlmPatch(x, y, K.f, K.cnt, [&](int ux, int uy) { return tD[(uy - dy0) * dw + (ux - dx0)]; }, D0, D1);
                        const float w0 = centre ? 1.0f : nlmWeight(D1);
                        const float w1 = centre ? 1.0f : nlmWeight(D0);
                        if (hit) regressTap(a0, a1, w0, w1, phi, Cq0, t1[qi]);
                        else regressTap0(a0, a1, w0, w1, Cq0, t1[qi]);
                    }
                }
                if (!centre) __syncthreads();
            }
        }
        if (!px.inside) return;
        if (valid) s = regressSums(a0, a1, R.ridge, hit);
    } else {
        if (!px.inside) return;
        valid = C0[px.p].w != 0.0f;
        const RegressFetchPlanes fetch{NlmFetchPlanes{C0, C1, V, W}, P, N, A};
        if (valid) s = regressPixel(x, y, W, H, R, fetch);
    }
    float4 o, e;
    nlmOutput(valid, H0[px.p], H1[px.p], s, o, e);
    out[px.p] = o;
    err[px.p] = e;
}

#endif  /* HIP */

}  // namespace surfdev
