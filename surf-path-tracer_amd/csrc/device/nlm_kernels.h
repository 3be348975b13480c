/*
 * nlm_kernels.h -- the dual-buffer non-local-means filter for stills
 * (surf_denoise_nlm*, include/surf_hip.h gives the arithmetic): the two half
 * images of the sample buckets are filtered with patch weights taken from the
 * other half (Rousselle, Knaus, Zwicker 2012), so the weights and the values
 * they average are independent and no feature plane is read.  No reference
 * counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states.  It is written once, in the SURF_HD functions below:
 * nlmPrepare (the half means, their validity, the variance estimate),
 * nlmDistance (one texel of a search offset's distance image), nlmPatch (the
 * row sums, then their sum), nlmWeight, nlmTap (the weighted sums) and
 * nlmOutput.
 *
 * The walk over a pixel's taps -- which taps exist, each tap's two patch
 * distances and its two cross-half weights -- is written once in each of two
 * forms, for this filter and for whatever else weights the halves this way
 * (device/regress_kernels.h): nlmWalk, every value from a Fetch object, which
 * the global kernels and the host twins call, and nlmWalkStaged, the same
 * pieces around an LDS copy of the tile and of the distance image: identical
 * bits.  What a tap is added to is the walk's template argument, a consumer
 * (NlmTaps states the interface); the walks know nothing of their consumers.
 */
#pragma once
#include "denoise_kernels.h"    /* the 32 x 8 tile: tilePixel */
#include "surf_math.h"
#include "types.h"

namespace surfdev {

constexpr int kNlmMaxSearch = 10, kNlmMaxPatch = 3;

/* what the host computes once per call */
struct NlmConsts {
    int r, f;
    float kk, alpha, eps, cnt;
};

/* The staged kernel's dynamic LDS, stated once for the host and the device:
 * the prepared records of the tile with its halo of r + f as two float4 planes
 * and one float2 plane -- (c0, validity), (c1, V.x), (V.y, V.z): 40 bytes a
 * texel -- then the distance image of one search offset, a float2 (weights'
 * half 0, half 1) per texel of the tile with its halo of f.  40.5 + 3.5 KB at
 * the defaults, 58.2 + 4.3 KB at r + f = 10 with f = 3; from r + f = 11
 * (64.8 KB of records) it does not fit kNlmLdsMax. */
SURF_HD int nlmTileW(int halo) { return kDenoiseTileW + 2 * halo; }
SURF_HD int nlmTileH(int halo) { return kDenoiseTileH + 2 * halo; }
SURF_HD size_t nlmPlaneTexels(int r, int f) { return (size_t)nlmTileW(r + f) * nlmTileH(r + f); }
SURF_HD size_t nlmDistTexels(int f) { return (size_t)nlmTileW(f) * nlmTileH(f); }
SURF_HD size_t nlmLdsBytes(int r, int f) { return (2 * sizeof(float4) + sizeof(float2)) * nlmPlaneTexels(r, f) + sizeof(float2) * nlmDistTexels(f); }
/* the staged variant is taken while its LDS leaves room for two workgroups on
 * a compute unit (160 KiB) beside whatever else runs there; above, the global one */
constexpr size_t kNlmLdsMax = 64 * 1024;
/* distance texels a thread of the 256-thread block computes per offset: ceil(38 * 14 / 256) at f = 3 */
constexpr int kNlmDistPerThread = 3;

SURF_HD int nlmClamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }
SURF_HD bool nlmFinite(float x) { return x - x == 0.0f; }

/* the half means of a pixel and whether it is valid; an invalid pixel has c0 = c1 = 0 */
struct NlmMeans {
    V3 c0, c1;
    bool valid;
};
SURF_HD NlmMeans nlmMeans(float4 h0, float4 h1) {
    NlmMeans m;
    m.c0 = mk3(0.0f, 0.0f, 0.0f);
    m.c1 = mk3(0.0f, 0.0f, 0.0f);
    m.valid = false;
    const float n0 = h0.w, n1 = h1.w;
    if (n0 > 0.0f && n1 > 0.0f) {
        const V3 a = mk3(h0.x / n0, h0.y / n0, h0.z / n0);
        const V3 b = mk3(h1.x / n1, h1.y / n1, h1.z / n1);
        if (nlmFinite(a.x) && nlmFinite(a.y) && nlmFinite(a.z) && nlmFinite(b.x) && nlmFinite(b.y) && nlmFinite(b.z)) {
            m.c0 = a;
            m.c1 = b;
            m.valid = true;
        }
    }
    return m;
}

/* the half planes in memory (device global memory, host arrays) */
struct NlmFetchHalves {
    const float4* H0;
    const float4* H1;
    int W;
    SURF_HD float4 h0(int x, int y) const { return H0[(size_t)y * W + x]; }
    SURF_HD float4 h1(int x, int y) const { return H1[(size_t)y * W + x]; }
};

/* Prepare: the packed records of pixel (x, y) -- C0 = (c0, valid ? 1 : 0),
 * C1 = (c1, V.x), VV = (V.y, V.z, 0, 0), V the 3 x 3 box mean of the halves'
 * squared difference: ten values in 40 of the 48 bytes */
template <class Fetch>
SURF_HD void nlmPrepare(int x, int y, int W, int H, const Fetch& fetch, float4& C0, float4& C1, float4& VV) {
    const NlmMeans m = nlmMeans(fetch.h0(x, y), fetch.h1(x, y));
    V3 s = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = nlmClamp(y + dy, H);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = nlmClamp(x + dx, W);
            const NlmMeans q = nlmMeans(fetch.h0(qx, qy), fetch.h1(qx, qy));
            const float ex = q.c0.x - q.c1.x, ey = q.c0.y - q.c1.y, ez = q.c0.z - q.c1.z;
            s.x = s.x + 0.5f * (ex * ex);
            s.y = s.y + 0.5f * (ey * ey);
            s.z = s.z + 0.5f * (ez * ez);
        }
    }
    C0 = make_float4(m.c0.x, m.c0.y, m.c0.z, m.valid ? 1.0f : 0.0f);
    C1 = make_float4(m.c1.x, m.c1.y, m.c1.z, s.x / 9.0f);
    VV = make_float4(s.y / 9.0f, s.z / 9.0f, 0.0f, 0.0f);
}

SURF_HD float nlmDistance1(float ca, float cb, float va, float vb, const NlmConsts& K) {
    const float d = ca - cb;
    const float vm = vb < va ? vb : va;
    const float num = d * d - K.alpha * (va + vm);
    const float den = K.eps + K.kk * (va + vb);
    return num / den;
}
/* one texel of a distance image: Ca, Cb the weights' half at a and b (.xyz), Va, Vb the variance estimates there */
SURF_HD float nlmDistance(float4 Ca, float4 Cb, float4 Va, float4 Vb, const NlmConsts& K) {
    const float dx = nlmDistance1(Ca.x, Cb.x, Va.x, Vb.x, K);
    const float dy = nlmDistance1(Ca.y, Cb.y, Va.y, Vb.y, K);
    const float dz = nlmDistance1(Ca.z, Cb.z, Va.z, Vb.z, K);
    return (dx + dy) + dz;
}

/* The patch distances of pixel (x, y) in both halves: dist(sx, sy) is the two
 * distance images (.x half 0, .y half 1) at an unclamped texel.  Rows first,
 * then the column of row sums. */
template <class Dist>
SURF_HD void nlmPatch(int x, int y, int f, float cnt, const Dist& dist, float& D0, float& D1) {
    float S0 = 0.0f, S1 = 0.0f;
    for (int j = -f; j <= f; ++j) {
        float R0 = 0.0f, R1 = 0.0f;
        for (int i = -f; i <= f; ++i) {
            const float2 d = dist(x + i, y + j);
            R0 = R0 + d.x;
            R1 = R1 + d.y;
        }
        S0 = S0 + R0;
        S1 = S1 + R1;
    }
    D0 = S0 / cnt;
    D1 = S1 / cnt;
}

SURF_HD float nlmWeight(float D) {
    float e = D < 100.0f ? D : 100.0f;              /* NaN -> 100 */
    e = e > 0.0f ? e : 0.0f;
    return gExpf(-e);
}

/* the weighted sums of the two halves of one pixel */
struct NlmSums {
    float w0, w1;
    V3 s0, s1;
};
SURF_HD NlmSums nlmZero() {
    NlmSums s;
    s.w0 = s.w1 = 0.0f;
    s.s0 = mk3(0.0f, 0.0f, 0.0f);
    s.s1 = mk3(0.0f, 0.0f, 0.0f);
    return s;
}
/* one taken tap: its two weights and the two halves' colours there */
SURF_HD void nlmTap(NlmSums& s, float w0, float w1, float4 Cq0, float4 Cq1) {
    s.w0 = s.w0 + w0;
    s.s0.x = s.s0.x + w0 * Cq0.x;
    s.s0.y = s.s0.y + w0 * Cq0.y;
    s.s0.z = s.s0.z + w0 * Cq0.z;
    s.w1 = s.w1 + w1;
    s.s1.x = s.s1.x + w1 * Cq1.x;
    s.s1.y = s.s1.y + w1 * Cq1.y;
    s.s1.z = s.s1.z + w1 * Cq1.z;
}

/* A consumer of the walks below says three things.  take(qx, qy): whether the
 * tap at an in-frame pixel whose colour is valid is taken at all -- asked
 * before the patch sum.  add(w0, w1, Cq0, Cq1): what a taken tap is added to.
 * And, for the staged walk alone, what it keeps in LDS beside the walk's own
 * planes: ldsFloat4s(K) records, which stage(lds, bx, by, W, H, K) fills for
 * the tile at (bx, by) before the walk's first barrier and begin(x, y, inside)
 * may read after it.  This one is the
 * non-local-means filter's: every tap, into the weighted sums, nothing staged. */
struct NlmTaps {
    NlmSums s = nlmZero();
    SURF_HD bool take(int, int) { return true; }
    SURF_HD void add(float w0, float w1, float4 Cq0, float4 Cq1) { nlmTap(s, w0, w1, Cq0, Cq1); }
    SURF_HD static size_t ldsFloat4s(const NlmConsts&) { return 0; }
    SURF_HD void stage(float4*, int, int, int, int, const NlmConsts&) {}
    SURF_HD void begin(int, int, bool) {}
};

/* the output records of a pixel: valid with the sums of its taps, else the plain mean */
SURF_HD void nlmOutput(bool valid, float4 h0, float4 h1, const NlmSums& s, float4& out, float4& err) {
    if (valid) {
        const V3 o0 = mk3(s.s0.x / s.w0, s.s0.y / s.w0, s.s0.z / s.w0);
        const V3 o1 = mk3(s.s1.x / s.w1, s.s1.y / s.w1, s.s1.z / s.w1);
        const float n0 = h0.w, n1 = h1.w, n = n0 + n1;
        out = make_float4(((o0.x * n0) + (o1.x * n1)) / n, ((o0.y * n0) + (o1.y * n1)) / n, ((o0.z * n0) + (o1.z * n1)) / n, 1.0f);
        const float ex = o0.x - o1.x, ey = o0.y - o1.y, ez = o0.z - o1.z;
        err = make_float4(0.25f * (ex * ex), 0.25f * (ey * ey), 0.25f * (ez * ez), 0.0f);
    } else {
        const float n = h0.w + h1.w;
        const float inv = n > 0.0f ? 1.0f / n : 0.0f;
        out = make_float4((h0.x + h1.x) * inv, (h0.y + h1.y) * inv, (h0.z + h1.z) * inv, 1.0f);
        err = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

/* the prepared records in memory (device global memory, host arrays); g selects the half, whose colour is .xyz */
struct NlmFetchPlanes {
    const float4* C0;
    const float4* C1;
    const float4* VV;
    int W;
    SURF_HD float4 c(int g, int x, int y) const { return (g ? C1 : C0)[(size_t)y * W + x]; }
    SURF_HD float4 v(int x, int y) const {
        const size_t i = (size_t)y * W + x;
        return make_float4(C1[i].w, VV[i].x, VV[i].y, 0.0f);
    }
};

/* The taps of a VALID pixel (x, y), every value from fetch.c / fetch.v at
 * in-frame texels: the taps dy outer and dx inner, each taken tap's two patch
 * distances computed texel by texel; half 0 takes the weight of the distance
 * in half 1 (D1) and the other way round, the centre tap weight 1 -- written
 * as one branch on the centre, not as two selects after the patch sum: the
 * same values, and the form in which the compiler keeps the centre's jump past
 * the exponentials (MEASUREMENTS "One stills walk"). */
template <class Fetch, class Taps>
SURF_HD void nlmWalk(int x, int y, int W, int H, const NlmConsts& K, const Fetch& fetch, Taps& taps) {
    for (int dy = -K.r; dy <= K.r; ++dy) {
        const int qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int dx = -K.r; dx <= K.r; ++dx) {
            const int qx = x + dx;
            if (qx < 0 || qx >= W) continue;
            const float4 Cq0 = fetch.c(0, qx, qy);
            if (Cq0.w == 0.0f) continue;
            if (!taps.take(qx, qy)) continue;
            const float4 Cq1 = fetch.c(1, qx, qy);
            const bool centre = dx == 0 && dy == 0;
            float w0 = 1.0f, w1 = 1.0f;
            if (!centre) {
                float D0, D1;
                nlmPatch(x, y, K.f, K.cnt, [&](int sx, int sy) {
                    const int ax = nlmClamp(sx, W), ay = nlmClamp(sy, H), bx = nlmClamp(sx + dx, W), by = nlmClamp(sy + dy, H);
                    const float4 Va = fetch.v(ax, ay), Vb = fetch.v(bx, by);
                    return make_float2(nlmDistance(fetch.c(0, ax, ay), fetch.c(0, bx, by), Va, Vb, K),
                                       nlmDistance(fetch.c(1, ax, ay), fetch.c(1, bx, by), Va, Vb, K));
                }, D0, D1);
                w0 = nlmWeight(D1);
                w1 = nlmWeight(D0);
            }
            taps.add(w0, w1, Cq0, Cq1);
        }
    }
}

/* the sums of a VALID pixel: the global kernel's and the host twin's pixel function */
template <class Fetch>
SURF_HD NlmSums nlmPixel(int x, int y, int W, int H, const NlmConsts& K, const Fetch& fetch) {
    NlmTaps taps;
    nlmWalk(x, y, W, H, K, fetch, taps);
    return taps.s;
}

#if defined(__HIPCC__) || defined(__HIP__)

/* The staged walk of a 256-thread block on its 32 x 8 pixel tile.  The block
 * copies the in-frame part of the tile with its halo of r + f -- the ten values
 * of a prepared record, 40 bytes -- into dynamic LDS (nlmLdsBytes; what the
 * consumer stages lies between the two float4 planes and the float2 plane).
 * Then, for every search offset but the centre, the block computes the
 * offset's distance image once per texel of the tile with its halo of f (both
 * halves, one float2) into LDS, meets at a barrier, and every valid pixel
 * whose tap is taken sums its patch from there: rows first, then the row
 * sums, as nlmPatch states -- the values and the order of nlmWalk.  A second
 * barrier ends the offset.  Every LDS read is at a texel clamped to the frame,
 * which lies in the staged part: the tile holds a frame pixel, so clamping a
 * texel of the tile's halo to the frame leaves it inside the halo.  Consecutive
 * lanes read consecutive 16-byte or 8-byte texels of a plane's row.  Every
 * thread of the block calls it, pixels outside the frame included (they take
 * no tap); returns whether the pixel is inside and valid. */
template <class Taps>
__device__ __forceinline__ bool nlmWalkStaged(float4* lds, const TilePixel& px, const float4* __restrict__ C0, const float4* __restrict__ C1,
                                              const float4* __restrict__ V, int W, int H, const NlmConsts& K, Taps& taps) {
    const int x = px.x, y = px.y;
    const int halo = K.r + K.f;
    const int tw = nlmTileW(halo), th = nlmTileH(halo), x0 = px.bx - halo, y0 = px.by - halo;
    const int dw = nlmTileW(K.f), dn = (int)nlmDistTexels(K.f), dx0 = px.bx - K.f, dy0 = px.by - K.f;
    const int texels = tw * th;
    float4* t0 = lds;
    float4* t1 = t0 + texels;
    float4* tTaps = t1 + texels;
    float2* tV = reinterpret_cast<float2*>(tTaps + Taps::ldsFloat4s(K));
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
    taps.stage(tTaps, px.bx, px.by, W, H, K);
    __syncthreads();
    taps.begin(x, y, px.inside);
    const auto var = [&](int i) { return make_float4(t1[i].w, tV[i].x, tV[i].y, 0.0f); };
    const auto at = [&](int qx, int qy) { return (qy - y0) * tw + (qx - x0); };
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
    const bool valid = px.inside && t0[at(x, y)].w != 0.0f;
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
                if (Cq0.w != 0.0f && taps.take(qx, qy)) {
                    float D0 = 0.0f, D1 = 0.0f;
                    if (!centre) nlmPatch(x, y, K.f, K.cnt, [&](int ux, int uy) { return tD[(uy - dy0) * dw + (ux - dx0)]; }, D0, D1);
                    const float w0 = centre ? 1.0f : nlmWeight(D1);
                    const float w1 = centre ? 1.0f : nlmWeight(D0);
                    taps.add(w0, w1, Cq0, t1[qi]);
                }
            }
            if (!centre) __syncthreads();
        }
    }
    return valid;
}

/* The filter: 256 threads on a 32 x 8 pixel tile, both halves in one launch
 * (the taps, their validity and the variance records are shared by the two).
 * STAGED: nlmWalkStaged.  Not STAGED: nlmWalk on global memory. */
template <bool STAGED>
__global__ __launch_bounds__(256) void k_nlm(const float4* __restrict__ C0, const float4* __restrict__ C1, const float4* __restrict__ V,
                                             const float4* __restrict__ H0, const float4* __restrict__ H1, float4* __restrict__ out,
                                             float4* __restrict__ err, int W, int H, NlmConsts K) {
    extern __shared__ float4 nlmTile[];
    const TilePixel px = tilePixel(W, H);
    NlmTaps taps;
    bool valid = false;
    if (STAGED) {
        valid = nlmWalkStaged(nlmTile, px, C0, C1, V, W, H, K, taps);
        if (!px.inside) return;
    } else {
        if (!px.inside) return;
        valid = C0[px.p].w != 0.0f;
        if (valid) nlmWalk(px.x, px.y, W, H, K, NlmFetchPlanes{C0, C1, V, W}, taps);
    }
    float4 o, e;
    nlmOutput(valid, H0[px.p], H1[px.p], taps.s, o, e);
    out[px.p] = o;
    err[px.p] = e;
}

#endif  /* HIP */

}  // namespace surfdev
