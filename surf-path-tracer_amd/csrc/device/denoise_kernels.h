/*
 * denoise_kernels.h -- the edge-avoiding a-trous wavelet filter (Dammertz et
 * al. 2010) guided by the first-hit feature buffers, with albedo
 * demodulation (surf_denoise*, include/surf_hip.h gives the arithmetic).  No
 * reference counterpart.
 *
 * The arithmetic is part of the interface: f32, no contraction, in the order
 * the header states, so the host twin (surf_denoise_image_host) and a numpy
 * restatement reproduce the device image bit for bit.  The two per-pixel
 * functions below -- denoisePrepare and denoisePixel -- are the only place
 * that arithmetic is written; the kernels and the host twin differ only in
 * the Fetch object that hands denoisePixel its taps (global memory, the
 * staged LDS tile, host arrays), as shadePath and k_aov share hitNormal.
 */
#pragma once
#include "surf_math.h"
#include "types.h"          /* kDenoiseMaxIterations */

namespace surfdev {

constexpr int kDenoiseTileW = 32, kDenoiseTileH = 8;      /* one 256-thread block */
/* largest step the LDS variant stages: the tile plus its 2*s halo is
 * (32+4s) x (8+4s) texels of 48 B -- 20.3 / 30 / 54 KiB at s = 1 / 2 / 4.  At
 * s = 8 it would be 120 KiB for 2.5 uses per staged texel, at s = 16 more
 * than the LDS: those steps always read their taps directly. */
constexpr int kDenoiseMaxStagedStep = 4;

/* the demodulation divisor of a pixel: albedo clamped from below where the
 * pixel is a hit and demodulation is on, else 1 */
SURF_HD V3 denoiseDen(float4 alb, uint32_t demodulate) {
    const bool valid = alb.w != 0.0f;
    if (!(valid && demodulate)) return mk3(1.0f, 1.0f, 1.0f);
    return mk3(alb.x > 0.01f ? alb.x : 0.01f, alb.y > 0.01f ? alb.y : 0.01f, alb.z > 0.01f ? alb.z : 0.01f);
}

/* Prepare: level 0 of the filtered image, I0 = (acc / samples) / den, and the
 * packed guides a tap reads: gN = (normal, valid ? 1 : 0), gP = (position, 0). */
SURF_HD void denoisePrepare(float4 acc, float4 pos, float4 nrm, float4 alb, uint32_t demodulate, float4& I0, float4& gN,
                            float4& gP) {
    const bool valid = alb.w != 0.0f;
    const float inv = acc.w > 0.0f ? 1.0f / acc.w : 0.0f;
    const V3 c = mk3(acc.x * inv, acc.y * inv, acc.z * inv);
    const V3 den = denoiseDen(alb, demodulate);
    I0 = make_float4(c.x / den.x, c.y / den.y, c.z / den.z, 0.0f);
    gN = make_float4(nrm.x, nrm.y, nrm.z, valid ? 1.0f : 0.0f);
    gP = make_float4(pos.x, pos.y, pos.z, 0.0f);
}

/* One a-trous level at a VALID pixel (x, y): the 25 taps at step s, dy outer
 * and dx inner, weights h (x) h times gExpf(-e).  fetch.n / .i / .p (qx, qy)
 * return the guide normal (w = validity), the image and the guide position
 * of an in-frame texel; the image and the position of a skipped tap are
 * never fetched.  Ip, Np, Pp are the centre's. */
template <class Fetch>
SURF_HD V3 denoisePixel(int x, int y, int W, int H, int s, float kc, float kn, float kp, float4 Ip, float4 Np, float4 Pp,
                        const Fetch& fetch) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float sumW = 0.0f;
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
            const float cx = Iq.x - Ip.x, cy = Iq.y - Ip.y, cz = Iq.z - Ip.z;
            const float dc = (cx * cx + cy * cy) + cz * cz;
            const float nx = Nq.x - Np.x, ny = Nq.y - Np.y, nz = Nq.z - Np.z;
            const float dn = (nx * nx + ny * ny) + nz * nz;
            const float px = Pq.x - Pp.x, py = Pq.y - Pp.y, pz = Pq.z - Pp.z;
            const float pl = (px * Np.x + py * Np.y) + pz * Np.z;
            const float dp = pl * pl;
            float e = (dc * kc + dn * kn) + dp * kp;
            e = e < 100.0f ? e : 100.0f;                 /* NaN -> 100; inside the range gExpf is verified on */
            const float w = (h[dy + 2] * h[dx + 2]) * gExpf(-e);
            sumW = sumW + w;
            sum.x = sum.x + w * Iq.x;
            sum.y = sum.y + w * Iq.y;
            sum.z = sum.z + w * Iq.z;
        }
    }
    return mk3(sum.x / sumW, sum.y / sumW, sum.z / sumW);     /* the centre tap makes sumW > 0 */
}

/* The image an iteration writes for a pixel: the filtered level, and on the
 * last iteration the remodulated output (I_n * den, 1) -- (c, 1) on a miss,
 * whose level is its level 0 = c unchanged. */
SURF_HD float4 denoiseStore(bool valid, float4 Ip, V3 filtered, bool last, float4 alb, uint32_t demodulate) {
    const V3 v = valid ? filtered : mk3(Ip.x, Ip.y, Ip.z);
    if (!last) return make_float4(v.x, v.y, v.z, 0.0f);
    if (!valid) return make_float4(v.x, v.y, v.z, 1.0f);
    const V3 den = denoiseDen(alb, demodulate);
    return make_float4(v.x * den.x, v.y * den.y, v.z * den.z, 1.0f);
}

/* taps from full-frame planes in memory (device global memory, host arrays) */
struct DenoiseFetchPlanes {
    const float4* I;
    const float4* N;
    const float4* P;
    int W;
    SURF_HD float4 n(int qx, int qy) const { return N[(size_t)qy * W + qx]; }
    SURF_HD float4 i(int qx, int qy) const { return I[(size_t)qy * W + qx]; }
    SURF_HD float4 p(int qx, int qy) const { return P[(size_t)qy * W + qx]; }
};

#if defined(__HIPCC__) || defined(__HIP__)

/* taps from the staged tile: three planes of tw x th texels whose texel
 * (0, 0) is frame pixel (x0, y0) */
struct DenoiseFetchTile {
    const float4* N;
    const float4* I;
    const float4* P;
    int x0, y0, tw;
    __device__ __forceinline__ float4 n(int qx, int qy) const { return N[(qy - y0) * tw + (qx - x0)]; }
    __device__ __forceinline__ float4 i(int qx, int qy) const { return I[(qy - y0) * tw + (qx - x0)]; }
    __device__ __forceinline__ float4 p(int qx, int qy) const { return P[(qy - y0) * tw + (qx - x0)]; }
};

/* the pixel a thread of a 256-thread block on a 32 x 8 tile stands for: its
 * place in the tile, the tile's origin (bx, by), the frame pixel (x, y),
 * whether the frame holds it and its index p there */
struct TilePixel {
    int tx, ty, bx, by, x, y;
    bool inside;
    size_t p;
};
__device__ __forceinline__ TilePixel tilePixel(int W, int H) {
    TilePixel t;
    t.tx = (int)(threadIdx.x & (kDenoiseTileW - 1));
    t.ty = (int)(threadIdx.x / kDenoiseTileW);
    t.bx = (int)blockIdx.x * kDenoiseTileW;
    t.by = (int)blockIdx.y * kDenoiseTileH;
    t.x = t.bx + t.tx;
    t.y = t.by + t.ty;
    t.inside = t.x < W && t.y < H;
    t.p = (size_t)t.y * W + t.x;
    return t;
}

/* The block copies the in-frame part of a tw x th tile of three planes, whose
 * texel (0, 0) is frame pixel (x0, y0), from g0..g2 into t0..t2 in LDS, then
 * meets at a barrier: every thread of the block calls it.  Out-of-frame texels
 * are left unwritten. */
__device__ __forceinline__ void stageTile3(float4* t0, float4* t1, float4* t2, const float4* __restrict__ g0,
                                           const float4* __restrict__ g1, const float4* __restrict__ g2, int x0, int y0, int tw,
                                           int th, int W, int H) {
    for (int t = (int)threadIdx.x; t < tw * th; t += 256) {
        const int ly = t / tw, lx = t - ly * tw;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t g = (size_t)gy * W + gx;
            t0[t] = g0[g];
            t1[t] = g1[g];
            t2[t] = g2[g];
        }
    }
    __syncthreads();
}

/* Elementwise: level 0 and the packed guides of n pixels.  (static: the
 * header is included by more than one translation unit; the one that
 * launches it owns it.) */
static __global__ __launch_bounds__(256) void k_denoise_prepare(const float4* __restrict__ acc, const float4* __restrict__ pos,
                                                         const float4* __restrict__ nrm, const float4* __restrict__ alb,
                                                         uint32_t demodulate, uint32_t n, float4* __restrict__ I0,
                                                         float4* __restrict__ gN, float4* __restrict__ gP) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    float4 i0, n4, p4;
    denoisePrepare(acc[p], pos[p], nrm[p], alb[p], demodulate, i0, n4, p4);
    I0[p] = i0;
    gN[p] = n4;
    gP[p] = p4;
}

/* One a-trous iteration at step s: 256 threads on a 32 x 8 pixel tile, the
 * grid covering partial tiles (W, H need be no multiple of the tile).
 * STAGED: the block first copies the tile plus its 2*s halo -- the in-frame
 * part of (32+4s) x (8+4s) texels of normal, image and position -- into
 * dynamic LDS (3 * 16 * (32+4s) * (8+4s) bytes) and takes centre and taps
 * from there; out-of-frame texels are left unwritten, denoisePixel never
 * fetches them.  Consecutive lanes store and read consecutive 16-byte texels
 * of a row: a ds_write_b128 group (8 contiguous lanes, 128 B) and a
 * ds_read_b128 group (16 lanes of one 32-pixel row, 16 distinct slots of the
 * 256-B bank row, whatever the tap's offset) are conflict-free.
 * Not STAGED: centre and taps from global memory (three 16-byte loads per
 * accepted tap).  Both call denoisePixel on the same values: identical bits.
 * `last` fuses the remodulation (alb is read only then). */
template <bool STAGED>
__global__ __launch_bounds__(256) void k_atrous(const float4* __restrict__ I, const float4* __restrict__ gN,
                                                const float4* __restrict__ gP, const float4* __restrict__ alb,
                                                float4* __restrict__ out, int W, int H, int s, float kc, float kn, float kp,
                                                uint32_t demodulate, int last) {
    extern __shared__ float4 dnTile[];
    const TilePixel px = tilePixel(W, H);
    const int x = px.x, y = px.y;
    const size_t p = px.p;
    float4 Ip, Np, Pp;
    V3 f = mk3(0.0f, 0.0f, 0.0f);
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
        if (Np.w != 0.0f) f = denoisePixel(x, y, W, H, s, kc, kn, kp, Ip, Np, Pp, fetch);
    } else {
        if (!px.inside) return;
        const DenoiseFetchPlanes fetch{I, gN, gP, W};
        Np = gN[p];
        Ip = I[p];
        Pp = gP[p];
        if (Np.w != 0.0f) f = denoisePixel(x, y, W, H, s, kc, kn, kp, Ip, Np, Pp, fetch);
    }
    const float4 a = last ? alb[p] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    out[p] = denoiseStore(Np.w != 0.0f, Ip, f, last != 0, a, demodulate);
}

#endif  /* HIP */

}  // namespace surfdev
