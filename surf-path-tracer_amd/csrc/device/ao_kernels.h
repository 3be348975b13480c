/* Ray-traced ambient occlusion and bent normals (surf_read_ao): cosine-weighted
 * any-hit rays from the points of a feature plane.  Included behind
 * wavefront_kernels.h, whose device functions it calls and whose text it
 * leaves alone. */
#pragma once

#include "device/wavefront_kernels.h"

namespace surfdev {

constexpr uint32_t kAoSeedSalt = 0x5AD0CC1Du;   /* SURF_AO_SEED_SALT: keeps the draws off the render's streams */

/* Sample s of pixel p: the direction R and whether the ray from P along R is
 * unoccluded within `radius`.  seed, cosineSample, shadePath's continuation
 * offset with `bias` in kEps's place, and the walk k_trace_any runs. */
template <bool LW>
__device__ __forceinline__ bool aoSampleOpen(const DevScene& S, const TraceTables& Tt, uint32_t p, uint32_t sample, V3 P, V3 N, float radius,
                                             float bias, V3& R, uint32_t* stk, uint32_t stride) {
    uint32_t seed = initSeed((p + 1799u * sample) ^ kAoSeedSalt);
    R = cosineSample(seed, N);
    const V3 O = add(P, lscl(bias, R));
    float depth = radius, u = 0.0f, v = 0.0f;
    uint32_t inst = kUnset, prim = kUnset;
    return !traceScene<true, LW>(S, Tt, O, R, depth, u, v, inst, prim, stk, stride);
}

/* Source planes srcPos / srcNrm / srcAlb: the first-hit planes or the chain's,
 * per shard pixel lp; valid = srcAlb.w != 0.  p is the pixel index the render
 * seeds with (x + row * width over the whole frame, u32 wrap-around).  For a
 * valid pixel, samples s = 0 .. samples - 1 (a power of two up to 64):
 *   bit s of the mask = sample s unoccluded;  nOpen = their number;
 *   sum = the unoccluded R, f32 from 0.0f, one add per unoccluded sample in
 *   sample order (nothing contracted, IEEE division).
 *   open[lp]  valid: (nOpen > 0 ? sum / (float)nOpen : 0, (float)nOpen / (float)samples)   else (0, 0, 0, 1)
 *   bits[lp]  valid: (mask bits 0-31, bits 32-63, nOpen, 1)                                else 0
 * Two lane mappings that write the same words:
 *   RAY = false  one lane per pixel loops over the samples (k_aov_sampled's shape).
 *   RAY = true   one lane per ray: a pixel's `samples` lanes are an aligned
 *     group of one wave (256 / samples pixels per block), they share P and N
 *     and start the walk on the same nodes.  The mask is the group's field of
 *     the wave's ballot; the sum is a loop over the group's lanes in sample
 *     order, each turn one cross-lane read per component -- not a tree, so the
 *     adds are the pixel map's.  No lane leaves before these wave-wide
 *     operations: lanes past the last pixel and lanes of invalid pixels stay
 *     converged, trace nothing and vote "occluded".
 * The trace tables are staged in dynamic LDS by every lane of the block, as
 * k_trace_any stages them; traceScene holds no wave-wide operation.  Reads
 * the scene and the source planes only: no Counters, no pool, nothing of the
 * captured graph. */
template <bool LDS, bool LW = false, bool RAY = false>
__global__ __launch_bounds__(kBlock) void k_ao(DevScene S, const uint32_t* __restrict__ rows, uint32_t width, uint32_t npx,
                                               uint32_t samples, uint32_t firstSample, float radius, float bias,
                                               const float4* __restrict__ srcPos, const float4* __restrict__ srcNrm,
                                               const float4* __restrict__ srcAlb, float4* __restrict__ open,
                                               uint4* __restrict__ bits, uint32_t stackWords) {
    extern __shared__ uint32_t lds[];
    const TraceTables Tt = traceTables<LDS>(S, lds, layout::laneTablesAt(stackWords, false));
    uint32_t* const stk = lds + threadIdx.x;
    const float ns = (float)samples;
    if (!RAY) {
        const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
        if (lp >= npx) return;
        float4 oO = make_float4(0.0f, 0.0f, 0.0f, 1.0f);
        uint4 oB = make_uint4(0u, 0u, 0u, 0u);
        if (srcAlb[lp].w != 0.0f) {
            const uint32_t rowi = lp / width;
            const uint32_t p = (lp - rowi * width) + rows[rowi] * width;
            const V3 P = xyz(srcPos[lp]), N = xyz(srcNrm[lp]);
            uint32_t lo = 0u, hi = 0u, nOpen = 0u;
            V3 sum = mk3(0.0f, 0.0f, 0.0f);
            for (uint32_t s = 0; s < samples; ++s) {
                V3 R;
                if (aoSampleOpen<LW>(S, Tt, p, firstSample + s, P, N, radius, bias, R, stk, blockDim.x)) {
                    lo |= s < 32u ? 1u << s : 0u;
                    hi |= s < 32u ? 0u : 1u << (s - 32u);
                    nOpen += 1u;
                    sum = add(sum, R);
                }
            }
            const float no = (float)nOpen;
            if (nOpen > 0u) sum = mk3(sum.x / no, sum.y / no, sum.z / no);
            oO = make_float4(sum.x, sum.y, sum.z, no / ns);
            oB = make_uint4(lo, hi, nOpen, 1u);
        }
        open[lp] = oO;
        bits[lp] = oB;
        return;
    }
    /* the ray map: samples is a power of two, so a group never straddles a wave */
    const uint32_t perBlock = blockDim.x / samples;
    const uint32_t s = threadIdx.x & (samples - 1u);
    const uint32_t lp = blockIdx.x * perBlock + threadIdx.x / samples;
    const bool inside = lp < npx;
    const bool valid = inside && srcAlb[lp].w != 0.0f;
    V3 R = mk3(0.0f, 0.0f, 0.0f);
    bool isOpen = false;
    if (valid) {
        const uint32_t rowi = lp / width;
        const uint32_t p = (lp - rowi * width) + rows[rowi] * width;
        isOpen = aoSampleOpen<LW>(S, Tt, p, firstSample + s, xyz(srcPos[lp]), xyz(srcNrm[lp]), radius, bias, R, stk, blockDim.x);
    }
    /* wave-wide from here: every lane of the wave takes part */
    const unsigned long long vote = __ballot(isOpen);
    const uint32_t base = (threadIdx.x & 63u) & ~(samples - 1u);   /* the group's first lane in the wave */
    const unsigned long long mask = samples == 64u ? vote : (vote >> base) & ((1ull << samples) - 1ull);
    /* (plain floats, each kept by a select: a select between two V3 objects is compiled through scratch) */
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t j = 0; j < samples; ++j) {
        const int from = (int)(base + j);
        const float rx = __shfl(R.x, from), ry = __shfl(R.y, from), rz = __shfl(R.z, from);
        const bool take = ((mask >> j) & 1ull) != 0ull;
        sx = take ? sx + rx : sx;
        sy = take ? sy + ry : sy;
        sz = take ? sz + rz : sz;
    }
    if (!inside || s != 0u) return;
    const uint32_t nOpen = (uint32_t)__popcll(mask);
    const float no = (float)nOpen;
    if (nOpen > 0u) { sx = sx / no; sy = sy / no; sz = sz / no; }
    open[lp] = valid ? make_float4(sx, sy, sz, no / ns) : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    bits[lp] = valid ? make_uint4((uint32_t)mask, (uint32_t)(mask >> 32), nOpen, 1u) : make_uint4(0u, 0u, 0u, 0u);
}

}  // namespace surfdev
