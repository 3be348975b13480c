/*
 * temporal_kernels.h -- temporal accumulation with reprojection, the temporal
 * half of SVGF (Schied et al. 2017): last frame's blended radiance is
 * reprojected onto this frame's pixels through the first-hit feature buffers
 * and blended with this frame's samples (surf_temporal*, include/surf_hip.h
 * gives the arithmetic).  No reference counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states, so the host twin (surf_temporal_image_host) and a numpy
 * restatement reproduce the device images bit for bit.  temporalPixel below
 * is the only place that arithmetic is written; k_temporal and the host twin
 * differ only in where the planes and the motion table live.  The constants
 * of the previous camera and the motion table are computed on the host, once
 * per frame, by temporalSetup.
 */
#pragma once
#include <string.h>

#include "denoise_kernels.h"      /* denoiseDen: the moments are those of the demodulated colour */
#include "surf_math.h"
#include "types.h"

namespace surfdev {

constexpr int kTemporalTileW = 32, kTemporalTileH = 8;     /* one 256-thread block, as k_atrous */
constexpr uint32_t kTemporalMotionWords = 25;              /* a motion-table record: moved, 3 x 4 of inv_transform, 3 x 4 of the previous transform */

/* what a tap reads of the previous frame beside its history (rgb, n) and its
 * position: the normal, and the instance id in the fourth word (as the
 * denoiser packs validity there) -- three 16-byte loads per tap */
struct alignas(16) TemporalGuide {
    float x, y, z;
    uint32_t id;
};
static_assert(sizeof(TemporalGuide) == 16, "a tap's guide is one 16-byte load");

/* per frame, from the previous camera and the parameters */
struct TemporalConsts {
    float C[3], G[3], n[3], U[3], V[3];     /* position, first_pixel - position, U x V, u_vector, v_vector */
    float g, iu, iv, resx, resy;
    float alphaMin, maxHistory, normalMin, planeTol, snap, minWeight;
    uint32_t havePrev;                       /* 0: no previous frame, every hit pixel starts a history */
    uint32_t nInst;                          /* records in the motion table (0 without a previous frame) */
};

/* The motion table: kTemporalMotionWords floats per instance --
 * [0] moved (1 / 0), [1 + 4k + j] = V[4j + k] and [13 + 4k + j] = T[4j + k] for
 * the rows k = 0..2 of this frame's inv_transform V and the previous frame's
 * transform T (column-major; the fourth rows are never read). */
inline void temporalMotionRecord(const float* curTransform, const float* curInv, const float* prevTransform, const float* prevInv,
                                 float* rec) {
    const bool moved = memcmp(curTransform, prevTransform, 64) != 0 || memcmp(curInv, prevInv, 64) != 0;
    rec[0] = moved ? 1.0f : 0.0f;
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 4; ++j) {
            rec[1 + 4 * k + j] = curInv[4 * j + k];
            rec[13 + 4 * k + j] = prevTransform[4 * j + k];
        }
}

/* row k of an affine matrix stored as above, applied to a point / a direction */
SURF_HD float temporalRowPoint(const float* r, float x, float y, float z) { return ((r[0] * x + r[1] * y) + r[2] * z) + r[3]; }
SURF_HD float temporalRowDir(const float* r, float x, float y, float z) { return (r[0] * x + r[1] * y) + r[2] * z; }

/* luminance, of the demodulated colour and of a level of the filtered image */
SURF_HD float svgfLum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

/* One pixel: A the accumulator (rgb sum, w = samples), P, N the position and
 * normal planes' records, id the id plane's x (~0 on a miss).  prev.g / .h /
 * .p (qx, qy) return the guide, the history and the position of an in-frame
 * texel of the previous frame; history and position of a tap whose instance
 * id differs are never fetched.  out = (r, 1), hist = (r, n').
 * MOMENTS (the variance-guided filter, surf_svgf*): the luminance moments
 * (mu1, mu2, m, 0) ride the same taps -- prev.m (qx, qy), read for used taps
 * only -- and blend with this frame's luminance of c / den into mom; the
 * colour path is the same arithmetic either way.  Without MOMENTS den is not
 * read, mom not written, prev.m not called. */
template <bool MOMENTS, class Prev>
SURF_HD void temporalPixel(int W, int H, float4 A, float4 P, float4 N, uint32_t id, const TemporalConsts& K, const float* motion,
                           const Prev& prev, float4& out, float4& hist, V3 den, float4& mom) {
    const float inv = A.w > 0.0f ? 1.0f / A.w : 0.0f;
    const V3 c = mk3(A.x * inv, A.y * inv, A.z * inv);
    if (id == 0xFFFFFFFFu) {
        out = make_float4(c.x, c.y, c.z, 1.0f);
        hist = make_float4(c.x, c.y, c.z, 0.0f);
        if (MOMENTS) mom = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float sumW = 0.0f, sumN = 0.0f;
    V3 sumC = mk3(0.0f, 0.0f, 0.0f);
    float sumWm = 0.0f;
    V3 sumM = mk3(0.0f, 0.0f, 0.0f);
    if (K.havePrev) {
        V3 Pp = mk3(P.x, P.y, P.z), Np = mk3(N.x, N.y, N.z);
        const float* m = motion + (size_t)kTemporalMotionWords * (id < K.nInst ? id : 0u);
        if (id < K.nInst && m[0] != 0.0f) {
            const float* Vr = m + 1;
            const float* Tr = m + 13;
            const V3 q = mk3(temporalRowPoint(Vr, P.x, P.y, P.z), temporalRowPoint(Vr + 4, P.x, P.y, P.z), temporalRowPoint(Vr + 8, P.x, P.y, P.z));
            Pp = mk3(temporalRowPoint(Tr, q.x, q.y, q.z), temporalRowPoint(Tr + 4, q.x, q.y, q.z), temporalRowPoint(Tr + 8, q.x, q.y, q.z));
            const V3 qn = mk3(temporalRowDir(Vr, N.x, N.y, N.z), temporalRowDir(Vr + 4, N.x, N.y, N.z), temporalRowDir(Vr + 8, N.x, N.y, N.z));
            const V3 mn = mk3(temporalRowDir(Tr, qn.x, qn.y, qn.z), temporalRowDir(Tr + 4, qn.x, qn.y, qn.z), temporalRowDir(Tr + 8, qn.x, qn.y, qn.z));
            const float il = 1.0f / sqrtf((mn.x * mn.x + mn.y * mn.y) + mn.z * mn.z);
            Np = mk3(mn.x * il, mn.y * il, mn.z * il);
        }
        const float Dx = Pp.x - K.C[0], Dy = Pp.y - K.C[1], Dz = Pp.z - K.C[2];
        const float dn = (Dx * K.n[0] + Dy * K.n[1]) + Dz * K.n[2];
        const float s = K.g / dn;
        const float Hx = Dx * s - K.G[0], Hy = Dy * s - K.G[1], Hz = Dz * s - K.G[2];
        float fx = (((Hx * K.U[0] + Hy * K.U[1]) + Hz * K.U[2]) * K.iu) * K.resx;
        float fy = (((Hx * K.V[0] + Hy * K.V[1]) + Hz * K.V[2]) * K.iv) * K.resy;
        if (s > 0.0f && fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H) {      /* a NaN fails */
            const float rx = rintf(fx), ry = rintf(fy);
            if (fabsf(fx - rx) <= K.snap) fx = rx;
            if (fabsf(fy - ry) <= K.snap) fy = ry;
            const float flx = floorf(fx), fly = floorf(fy);
            const int ix = (int)flx, iy = (int)fly;
            const float tx = fx - flx, ty = fy - fly;
            const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty};
            const float tol = K.planeTol * P.w;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int qx = ix + (t & 1), qy = iy + (t >> 1);
                const float w = wx[t & 1] * wy[t >> 1];
                if (qx < 0 || qx >= W || qy < 0 || qy >= H || !(w > 0.0f)) continue;
                const TemporalGuide Gq = prev.g(qx, qy);
                if (Gq.id != id) continue;
                const float4 Hq = prev.h(qx, qy);
                const float4 Pq = prev.p(qx, qy);
                const float dnn = (Gq.x * Np.x + Gq.y * Np.y) + Gq.z * Np.z;
                const float ex = Pp.x - Pq.x, ey = Pp.y - Pq.y, ez = Pp.z - Pq.z;
                const float pl = (ex * Gq.x + ey * Gq.y) + ez * Gq.z;
                if (!(Hq.w > 0.0f && dnn >= K.normalMin && fabsf(pl) <= tol)) continue;
                sumW = sumW + w;
                sumC.x = sumC.x + w * Hq.x;
                sumC.y = sumC.y + w * Hq.y;
                sumC.z = sumC.z + w * Hq.z;
                sumN = sumN + w * Hq.w;
                if (MOMENTS) {
                    const float4 Mq = prev.m(qx, qy);
                    if (Mq.z > 0.0f) {
                        sumWm = sumWm + w;
                        sumM.x = sumM.x + w * Mq.x;
                        sumM.y = sumM.y + w * Mq.y;
                        sumM.z = sumM.z + w * Mq.z;
                    }
                }
            }
        }
    }
    V3 r = c;
    float n1 = A.w > 0.0f ? 1.0f : 0.0f;
    if (sumW > K.minWeight) {
        const V3 hc = mk3(sumC.x / sumW, sumC.y / sumW, sumC.z / sumW);
        const float hn = sumN / sumW;
        if (A.w > 0.0f) {
            const float nn = hn + 1.0f;
            n1 = nn < K.maxHistory ? nn : K.maxHistory;
            float a = 1.0f / n1;
            a = a < K.alphaMin ? K.alphaMin : a;
            r = mk3(hc.x + (c.x - hc.x) * a, hc.y + (c.y - hc.y) * a, hc.z + (c.z - hc.z) * a);
        } else {
            r = hc;
            n1 = hn;
        }
    }
    out = make_float4(r.x, r.y, r.z, 1.0f);
    hist = make_float4(r.x, r.y, r.z, n1);
    if (MOMENTS) {
        const float l = svgfLum(c.x / den.x, c.y / den.y, c.z / den.z);
        if (sumW > K.minWeight && sumWm > K.minWeight) {
            const V3 hm = mk3(sumM.x / sumWm, sumM.y / sumWm, sumM.z / sumWm);
            if (A.w > 0.0f) {
                const float mm = hm.z + 1.0f;
                const float m1 = mm < K.maxHistory ? mm : K.maxHistory;
                float am = 1.0f / m1;
                am = am < K.alphaMin ? K.alphaMin : am;
                mom = make_float4(hm.x + (l - hm.x) * am, hm.y + (l * l - hm.y) * am, m1, 0.0f);
            } else {
                mom = make_float4(hm.x, hm.y, hm.z, 0.0f);
            }
        } else {
            mom = A.w > 0.0f ? make_float4(l, l * l, 1.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
}

/* taps from the previous frame's full-frame planes in memory (device global memory, host arrays) */
struct TemporalFetchPlanes {
    const float4* Hs;
    const float4* Ps;
    const TemporalGuide* Gs;
    int W;
    const float4* Ms;                        /* the moments plane (MOMENTS only); NULL: every m = 0 */
    SURF_HD float4 m(int qx, int qy) const { return Ms ? Ms[(size_t)qy * W + qx] : make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    SURF_HD TemporalGuide g(int qx, int qy) const { return Gs[(size_t)qy * W + qx]; }
    SURF_HD float4 h(int qx, int qy) const { return Hs[(size_t)qy * W + qx]; }
    SURF_HD float4 p(int qx, int qy) const { return Ps[(size_t)qy * W + qx]; }
};

#if defined(__HIPCC__) || defined(__HIP__)

/* One frame: 256 threads on a 32 x 8 pixel tile, the grid covering partial
 * tiles.  A row of 32 lanes loads consecutive 16-byte records of the four
 * current planes (of the id plane its first word) and stores consecutive
 * records of the images it writes: out, hist and -- when gP, gN are given --
 * this frame's position and packed guide, which the next frame's taps read
 * (the feature-buffer cache does not outlive a camera or instance change).
 * Taps come straight from global memory: a tile's reprojected footprint is
 * unbounded, and an unmoved pixel's single tap is its own, coalesced texel.
 * The motion table is read from global memory whatever its size: a copy in
 * LDS for up to 64 instances was measured and gains nothing (2 - 4 % slower
 * at 1280 x 720 in a same-session A/B, MEASUREMENTS "Temporal accumulation") -- a hit pixel reads one word of it,
 * a moved pixel 25, all lanes of a wave mostly the same record, and the copy
 * and its barrier cost more than those cached loads.  No LDS.  Without a
 * previous frame pH, pP, pG and motion are never read.
 * MOMENTS: the albedo plane in (the demodulation divisor), the previous
 * moments in (a fourth 16-byte load per used tap; NULL: none stored) and
 * this frame's moments out; the other instantiation never touches mo. */
struct TemporalMomentPlanes {
    const float4* alb;
    const float4* pM;
    float4* outM;
    uint32_t demodulate;
};

template <bool MOMENTS>
__global__ __launch_bounds__(256) void k_temporal(const float4* __restrict__ A, const float4* __restrict__ P,
                                                  const float4* __restrict__ N, const uint4* __restrict__ ID,
                                                  const float4* __restrict__ pH, const float4* __restrict__ pP,
                                                  const TemporalGuide* __restrict__ pG, const float* __restrict__ motion,
                                                  TemporalConsts K, int W, int H, float4* __restrict__ out,
                                                  float4* __restrict__ hist, float4* __restrict__ gP,
                                                  TemporalGuide* __restrict__ gN, TemporalMomentPlanes mo) {
    const int x = (int)blockIdx.x * kTemporalTileW + (int)(threadIdx.x & (kTemporalTileW - 1));
    const int y = (int)blockIdx.y * kTemporalTileH + (int)(threadIdx.x / kTemporalTileW);
    if (x >= W || y >= H) return;
    const size_t p = (size_t)y * W + x;
    const float4 a = A[p], pos = P[p], nrm = N[p];
    const uint32_t id = ID[p].x;
    const TemporalFetchPlanes prev{pH, pP, pG, W, MOMENTS ? mo.pM : nullptr};
    float4 o, h, m;
    V3 den = mk3(1.0f, 1.0f, 1.0f);
    if (MOMENTS) den = denoiseDen(mo.alb[p], mo.demodulate);
    temporalPixel<MOMENTS>(W, H, a, pos, nrm, id, K, motion, prev, o, h, den, m);
    out[p] = o;
    hist[p] = h;
    if (MOMENTS) mo.outM[p] = m;
    if (gP) {
        gP[p] = pos;
        TemporalGuide g;
        g.x = nrm.x; g.y = nrm.y; g.z = nrm.z; g.id = id;
        gN[p] = g;
    }
}

#endif  /* HIP */

}  // namespace surfdev
