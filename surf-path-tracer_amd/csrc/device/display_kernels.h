/*
 * display_kernels.h -- the display stage (surf_display*, include/surf_hip.h):
 * metered exposure, bloom, tone curve, transfer function and ordered dither
 * from a float RGBA image to RGBA8 words.  The arithmetic is written once, in
 * the SURF_HD functions below, which the CPU twin (host/display.hip) compiles
 * for the host; the kernels only fetch, stage and store.
 *
 * Device memory the stage keeps per context (host/display.hip lays it out):
 * the meter record -- 256 histogram words, then counted, black, median_bin and
 * the bits of scale, which is surf_display_meter_result word for word -- in
 * kDisplayStripes copies, of which the meter's blocks fill one each and the
 * scale kernel sums all into the first.  The kernels after k_display_scale
 * read scale from that first copy: no host round trip between the meter and
 * the pack.  The 4096-entry sRGB table is in constant memory, one per device.
 */
#pragma once
#include "device/denoise_kernels.h"

namespace surfdev {

constexpr int kDisplayMaxBloom = 16;                 /* the largest bloom_radius */
constexpr int kDisplayBins = 256;
constexpr uint32_t kDisplayFirstBin = 888;           /* bits(2^-16) >> 20 */
constexpr int kDisplayTable = 4096;
/* the words of the meter record behind the histogram */
enum { kDisplayCounted = kDisplayBins, kDisplayBlack, kDisplayMedian, kDisplayScale, kDisplayRecordWords };
/* The meter's blocks add into kDisplayStripes copies of the record, kDisplayStripeWords apart, block b into copy
 * b % kDisplayStripes: a thousand blocks adding to one address wait for each other.  The scale kernel sums the copies
 * into the first, which is the result. */
#ifndef SURF_DISPLAY_STRIPES
#define SURF_DISPLAY_STRIPES 16                      /* a tuning build may say 1: the single record MEASUREMENTS "Display stage" compares with */
#endif
constexpr uint32_t kDisplayStripes = SURF_DISPLAY_STRIPES;
constexpr uint32_t kDisplayStripeWords = 264;

/* what the host hands every kernel: the parameters and the bloom's normalised weights wn_0..wn_R.
 * A kernel argument: the weights are read with a wave-uniform index, from the kernel's argument segment. */
struct DisplayConsts {
    int R, curve, transfer, dither;
    int autoExposure;
    float exposure, key, minScale, maxScale;
    float threshold, strength, ww;                   /* ww = white * white */
    float wn[kDisplayMaxBloom + 1];
};

struct DisplayRgb { float x, y, z; };

/* rule 1: the mean of the pixel's own samples; a NaN or a negative value becomes 0, +inf stays */
SURF_HD DisplayRgb displayColour(float4 a) {
    const float n = a.w;
    DisplayRgb c;
    c.x = n > 0.0f ? a.x / n : 0.0f;
    c.y = n > 0.0f ? a.y / n : 0.0f;
    c.z = n > 0.0f ? a.z / n : 0.0f;
    c.x = c.x > 0.0f ? c.x : 0.0f;
    c.y = c.y > 0.0f ? c.y : 0.0f;
    c.z = c.z > 0.0f ? c.z : 0.0f;
    return c;
}

/* rule 2 */
SURF_HD float displayLum(DisplayRgb c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

/* rule 3, per pixel: the histogram word the pixel counts in -- its bin, or kDisplayBlack */
SURF_HD uint32_t displayMeterWord(float4 a) {
    const uint32_t b = f2u(displayLum(displayColour(a))) >> 20;
    if (b < kDisplayFirstBin) return (uint32_t)kDisplayBlack;
    const uint32_t bin = b - kDisplayFirstBin;
    return bin < (uint32_t)kDisplayBins - 1u ? bin : (uint32_t)kDisplayBins - 1u;
}

/* rule 3, the scale from the median bin m of `counted` pixels */
SURF_HD float displayScale(const DisplayConsts& K, uint32_t m, uint32_t counted) {
    if (!K.autoExposure) return K.exposure;
    if (counted == 0u) return 1.0f;
    const float Lm = u2f(((m + kDisplayFirstBin) << 20) | 0x80000u);
    float s = K.key / Lm;
    s = s < K.minScale ? K.minScale : s;
    s = s > K.maxScale ? K.maxScale : s;
    return s;
}

/* rule 4 */
SURF_HD DisplayRgb displayExpose(DisplayRgb c, float scale) {
    DisplayRgb e;
    e.x = c.x * scale, e.y = c.y * scale, e.z = c.z * scale;
    return e;
}

/* rule 5, the bright part (w = 0: the record is padding) */
SURF_HD float displayBright1(float e, float threshold) { return (e - threshold) > 0.0f ? e - threshold : 0.0f; }
SURF_HD float4 displayBright(float4 a, float scale, float threshold) {
    const DisplayRgb e = displayExpose(displayColour(a), scale);
    return make_float4(displayBright1(e.x, threshold), displayBright1(e.y, threshold), displayBright1(e.z, threshold), 0.0f);
}

/* rule 5, one pass: the sum from 0.0f over i = -R..R ascending of wn_|i| * tap(i) */
template <class Tap>
SURF_HD float4 displayBlur(const DisplayConsts& K, const Tap& tap) {
    float4 s = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int i = -K.R; i <= K.R; ++i) {
        const float w = K.wn[i < 0 ? -i : i];
        const float4 b = tap(i);
        s.x = s.x + w * b.x;
        s.y = s.y + w * b.y;
        s.z = s.z + w * b.z;
    }
    return s;
}

/* rule 6 */
SURF_HD float displayCurve(const DisplayConsts& K, float x) {
    float t = x;
    if (K.curve == 1) t = (x * (1.0f + x / K.ww)) / (1.0f + x);
    else if (K.curve == 2) t = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    float v = t < 1.0f ? t : 1.0f;                   /* a NaN (from +inf) becomes 1 */
    v = v > 0.0f ? v : 0.0f;
    return v;
}

/* rule 7; T: the sRGB table, indexed by the square root */
SURF_HD float displayTransfer(const DisplayConsts& K, float v, const float* T) {
    if (K.transfer == 0) return v;
    const float r = sqrtf(v);
    if (K.transfer == 1) return r;
    return T[(uint32_t)(r * 4095.0f + 0.5f)];
}

/* the standard 8 x 8 Bayer matrix B8[y & 7][x & 7] (the header writes it out): the bits of
 * x ^ y and y interleaved, most significant pair from the lowest bit */
SURF_HD uint32_t displayBayer8(uint32_t x, uint32_t y) {
    const uint32_t a = (x ^ y) & 7u, b = y & 7u;
    uint32_t v = 0;
    for (uint32_t k = 0; k < 3; ++k) v = (v << 2) | ((((a >> k) & 1u) << 1) | ((b >> k) & 1u));
    return v;
}

/* rule 8, one channel */
SURF_HD uint32_t displayQuant(float u, float d) {
    const uint32_t q = (uint32_t)(u * 255.0f + d);
    return q < 255u ? q : 255u;
}

/* rules 6-8 and the pack, from the pixel's colour before the curve */
SURF_HD uint32_t displayPack(const DisplayConsts& K, DisplayRgb x, uint32_t px, uint32_t py, const float* T) {
    const float d = K.dither ? ((float)displayBayer8(px, py) + 0.5f) / 64.0f : 0.5f;
    const uint32_t r = displayQuant(displayTransfer(K, displayCurve(K, x.x), T), d);
    const uint32_t g = displayQuant(displayTransfer(K, displayCurve(K, x.y), T), d);
    const uint32_t b = displayQuant(displayTransfer(K, displayCurve(K, x.z), T), d);
    return r | (g << 8) | (b << 16) | (255u << 24);
}

/* rules 4 and 5's last line: the exposed colour plus strength times the blurred bright part */
SURF_HD DisplayRgb displayAddBloom(DisplayRgb e, float strength, float4 Vv) {
    DisplayRgb x;
    x.x = e.x + strength * Vv.x;
    x.y = e.y + strength * Vv.y;
    x.z = e.z + strength * Vv.z;
    return x;
}

#if defined(__HIPCC__) || defined(__HIP__)

/* rule 7's table in constant memory: one copy per device, filled by the host before a context's first pack */
__constant__ float kDisplaySrgb[kDisplayTable];

/* The meter: each block counts its pixels in an LDS histogram (integer LDS atomics), then
 * adds each non-empty word to its copy of the global record with one integer atomic.
 * Integers only: the record does not depend on the order of arrival. */
__global__ __launch_bounds__(256) void k_display_meter(const float4* __restrict__ A, uint32_t npx, uint32_t* __restrict__ rec) {
    __shared__ uint32_t h[kDisplayBins + 2];         /* the bins, then counted (unused here) and black at the record's offsets */
    for (uint32_t k = threadIdx.x; k < (uint32_t)kDisplayBins + 2u; k += blockDim.x) h[k] = 0u;
    __syncthreads();
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < npx; p += stride) atomicAdd(&h[displayMeterWord(A[p])], 1u);
    __syncthreads();
    uint32_t* mine = rec + (blockIdx.x % kDisplayStripes) * kDisplayStripeWords;
    for (uint32_t k = threadIdx.x; k < (uint32_t)kDisplayBins + 2u; k += blockDim.x)
        if (h[k] != 0u) atomicAdd(&mine[k], h[k]);
}

/* The scale: one wave sums the record's copies into the first and scans its 256 bins (four
 * per lane), finds the median bin and writes counted, median_bin and scale behind the
 * histogram. */
__global__ __launch_bounds__(64) void k_display_scale(uint32_t* __restrict__ rec, DisplayConsts K) {
    const uint32_t lane = threadIdx.x;
    uint32_t b[4];
    uint32_t own = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[k] = 0u;
        for (uint32_t st = 0; st < kDisplayStripes; ++st) b[k] += rec[st * kDisplayStripeWords + 4 * lane + k];
        rec[4 * lane + k] = b[k];
        own += b[k];
    }
    uint32_t black = 0;
    if (lane == 0)
        for (uint32_t st = 0; st < kDisplayStripes; ++st) black += rec[st * kDisplayStripeWords + kDisplayBlack];
    uint32_t incl = own;                             /* counts fit 32 bits: at most 2^27 pixels */
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    const uint32_t counted = __shfl(incl, 63, 64);
    unsigned long long cum = incl - own;
    uint32_t m = (uint32_t)kDisplayBins;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cum += b[k];
        if (m == (uint32_t)kDisplayBins && 2ull * cum >= (unsigned long long)counted) m = 4u * lane + (uint32_t)k;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const uint32_t o = __shfl_xor(m, d, 64);
        m = o < m ? o : m;
    }
    if (lane == 0) {
        rec[kDisplayCounted] = counted;
        rec[kDisplayBlack] = black;
        rec[kDisplayMedian] = m;
        rec[kDisplayScale] = f2u(displayScale(K, m, counted));
    }
}

/* The pack without bloom: rules 1, 4 and 6-8 per pixel of the 32 x 8 tiles. */
__global__ __launch_bounds__(256) void k_display_pack(const float4* __restrict__ A, int W, int H, const uint32_t* __restrict__ rec,
                                                      uint32_t* __restrict__ out, DisplayConsts K) {
    const TilePixel px = tilePixel(W, H);
    if (!px.inside) return;
    const float scale = u2f(rec[kDisplayScale]);
    out[px.p] = displayPack(K, displayExpose(displayColour(A[px.p]), scale), (uint32_t)px.x, (uint32_t)px.y, kDisplaySrgb);
}

/* The bloom's horizontal pass: the exposed bright part of the tile and its halo of R
 * columns (clamped to the frame) staged in LDS, one record a texel; Hh out. */
__global__ __launch_bounds__(256) void k_display_blur_h(const float4* __restrict__ A, int W, int H, const uint32_t* __restrict__ rec,
                                                        float4* __restrict__ Hh, DisplayConsts K) {
    __shared__ float4 t[kDenoiseTileH * (kDenoiseTileW + 2 * kDisplayMaxBloom)];
    const TilePixel px = tilePixel(W, H);
    const float scale = u2f(rec[kDisplayScale]);
    const int tw = kDenoiseTileW + 2 * K.R;
    for (int k = (int)threadIdx.x; k < tw * kDenoiseTileH; k += 256) {
        const int ty = k / tw, tx = k - ty * tw;
        const int gy = px.by + ty;
        int gx = px.bx - K.R + tx;
        gx = gx < 0 ? 0 : (gx > W - 1 ? W - 1 : gx);
        if (gy < H) t[k] = displayBright(A[(size_t)gy * W + gx], scale, K.threshold);
    }
    __syncthreads();
    if (!px.inside) return;
    const float4* row = t + px.ty * tw + px.tx + K.R;
    Hh[px.p] = displayBlur(K, [&](int i) { return row[i]; });
}

/* The vertical pass, fused with the rest: Hh of the tile and its halo of R rows (clamped
 * to the frame) staged in LDS, then rules 4, 5's sum and 6-8 and the pack. */
__global__ __launch_bounds__(256) void k_display_blur_v_pack(const float4* __restrict__ A, const float4* __restrict__ Hh, int W, int H,
                                                             const uint32_t* __restrict__ rec, uint32_t* __restrict__ out, DisplayConsts K) {
    __shared__ float4 t[(kDenoiseTileH + 2 * kDisplayMaxBloom) * kDenoiseTileW];
    const TilePixel px = tilePixel(W, H);
    const int th = kDenoiseTileH + 2 * K.R;
    for (int k = (int)threadIdx.x; k < th * kDenoiseTileW; k += 256) {
        const int ty = k / kDenoiseTileW, tx = k - ty * kDenoiseTileW;
        const int gx = px.bx + tx;
        int gy = px.by - K.R + ty;
        gy = gy < 0 ? 0 : (gy > H - 1 ? H - 1 : gy);
        if (gx < W) t[k] = Hh[(size_t)gy * W + gx];
    }
    __syncthreads();
    if (!px.inside) return;
    const float scale = u2f(rec[kDisplayScale]);
    const float4* col = t + (px.ty + K.R) * kDenoiseTileW + px.tx;
    const float4 Vv = displayBlur(K, [&](int j) { return col[j * kDenoiseTileW]; });
    const DisplayRgb x = displayAddBloom(displayExpose(displayColour(A[px.p]), scale), K.strength, Vv);
    out[px.p] = displayPack(K, x, (uint32_t)px.x, (uint32_t)px.y, kDisplaySrgb);
}

#endif

}  // namespace surfdev
