/* Sampled feature buffers (surf_read_aov_sampled): the first-hit features of
 * the very camera rays the render traces, reduced per pixel.  Included behind
 * wavefront_kernels.h, whose device functions it calls and whose text it
 * leaves alone. */
#pragma once

#include "device/wavefront_kernels.h"

namespace surfdev {

constexpr uint32_t kMatteSlots = 8;    /* distinct keys a pixel's table holds */
constexpr uint32_t kMatteRanks = 4;    /* ... and how many of them go out */

/* One lane per shard pixel lp loops over the samples s = 0 .. samples - 1 in
 * order.  p is the pixel index the render seeds with (x + row * width over the
 * whole frame, u32 wrap-around), and sample s is the primary ray of frame
 * firstSample + s at one sample per frame:
 *   seed = initSeed(p + 1799u * (firstSample + s));  (o, d) = cameraSample's ray
 *   (jy, jx, then the lens disk's sy, sx rejection loop when the camera has a
 *   defocus angle);  closest hit from depth 1e30;  per-sample features k_aov's
 *   expressions term for term.
 * Running sums, f32 from 0.0f, one add per sample in sample order (nothing
 * contracted, IEEE division): nHit; sum P, sum t, sum N over the hit samples;
 * sum a over all samples (a miss adds the background along d).  Planes:
 *   pos[lp]  nHit > 0: (sum P / (float)nHit, sum t / (float)nHit)   else (0, 0, 0, 1e30)
 *   nrm[lp]  nHit > 0: (sum N / (float)nHit, 0), not renormalised   else 0
 *   alb[lp]  (sum a / (float)samples, (float)nHit / (float)samples)
 *   ids[lp]  sample 0's hit (instance, primitive, material, nHit); miss (~0, ~0, ~0, nHit)
 *   mkey[lp], mcnt[lp]  the matte: a sample's key is its instance index
 *            (material index with keyMode 1; ~0 for a miss, counted like any
 *            key).  The table keeps the first kMatteSlots distinct keys in order
 *            of first appearance with their counts; a sample whose key is new
 *            once the table is full is not counted.  Out go the kMatteRanks
 *            best by count descending, ties by first appearance ascending;
 *            empty ranks are key ~0 with count 0.
 * The table lives in registers: every slot is compared and updated unrolled
 * with predicated writes, never indexed by a runtime value.  Tables, dynamic
 * LDS and variants as k_aov.  The lanes of a wave run the same number of
 * turns; traceScene holds no wave-wide operation.  Reads the scene and the
 * camera only: no Counters, no pool, nothing of the captured graph. */
template <bool LDS, bool LW = false>
__global__ __launch_bounds__(kBlock) void k_aov_sampled(DevScene S, DevCamera cam, const uint32_t* __restrict__ rows, uint32_t width,
                                                        uint32_t npx, uint32_t samples, uint32_t firstSample, uint32_t keyMode,
                                                        float4* __restrict__ pos, float4* __restrict__ nrm, float4* __restrict__ alb,
                                                        uint4* __restrict__ ids, uint4* __restrict__ mkey, uint4* __restrict__ mcnt,
                                                        uint32_t stackWords) {
    extern __shared__ uint32_t lds[];
    __shared__ DevInstance sInst[LDS ? kLdsInst : 1];
    __shared__ DevMaterial sMat[LDS ? kLdsMats : 1];
    __shared__ uint2 sLights[LDS ? kLdsLights : 1];
    const TraceTables Tt = traceTables<LDS>(S, lds, layout::laneTablesAt(stackWords, false));
    ShadeTables Tb{S.inst, S.mats, S.lights};
    if (LDS) {
        stageTables(S, sInst, sMat, sLights);
        Tb = ShadeTables{sInst, sMat, sLights};
    }
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npx) return;
    const StreamGeom G{rows, width, npx, 1u, nullptr};    /* cameraSample reads rows and width */
    const uint32_t rowi = lp / width;
    const uint32_t p = (lp - rowi * width) + rows[rowi] * width;
    /* the background's colours, element by element from the kernel argument (no copy of it in scratch) */
    const V3 bgColor = mk3(S.bgColor[0], S.bgColor[1], S.bgColor[2]);
    const V3 bgA = mk3(S.bgA[0], S.bgA[1], S.bgA[2]), bgB = mk3(S.bgB[0], S.bgB[1], S.bgB[2]);
    uint32_t nHit = 0u;
    V3 sP = mk3(0.0f, 0.0f, 0.0f), sN = sP, sA = sP;
    float sT = 0.0f;
    uint4 oI = make_uint4(kUnset, kUnset, kUnset, 0u);
    uint32_t tk[kMatteSlots], tc[kMatteSlots];
#pragma unroll
    for (uint32_t i = 0; i < kMatteSlots; ++i) { tk[i] = kUnset; tc[i] = 0u; }
    uint32_t used = 0u;
    for (uint32_t s = 0; s < samples; ++s) {
        float4 o4, d4, T4;
        cameraSample(cam, G, lp, 0u, initSeed(p + 1799u * (firstSample + s)), o4, d4, T4);
        const V3 o = xyz(o4), d = xyz(d4);
        float depth = kFarAway, hu = 0.0f, hv = 0.0f;
        uint32_t inst = kUnset, prim = kUnset;
        const bool hit = traceScene<false, LW>(S, Tt, o, d, depth, hu, hv, inst, prim, lds + threadIdx.x, blockDim.x);
        uint32_t key = kUnset;
        if (hit) {
            const DevInstance& I = Tb.inst[inst];
            const DevMaterial& m = Tb.mats[I.material];
            const V3 P = add(o, lscl(depth, d));
            const V3 N = hitNormal(S, I, prim, hu, hv, d);
            const bool isLight = m.emit > 0.0f && (m.ec[0] > 0.0f || m.ec[1] > 0.0f || m.ec[2] > 0.0f);
            const V3 a = isLight ? lscl(m.emit, ld3(m.ec)) : ld3(m.albedo);
            nHit += 1u;
            sP = add(sP, P);
            sT = sT + depth;
            sN = add(sN, N);
            sA = add(sA, a);
            key = keyMode ? I.material : inst;
            if (s == 0u) oI = make_uint4(inst, prim, I.material, 0u);
        } else {
            /* SceneBackground along d (scene.cpp:35-51), shadePath's miss */
            V3 bg = mk3(0.0f, 0.0f, 0.0f);
            if (S.bgType == 0u) bg = bgColor;
            else if (S.bgType == 1u) {
                const float a = 0.5f * (1.0f + d.y);
                bg = add(lscl(a, bgB), lscl(1.0f - a, bgA));
            }
            sA = add(sA, bg);
        }
        /* the key table: count the key's slot, or take the next free one */
        bool found = false;
#pragma unroll
        for (uint32_t i = 0; i < kMatteSlots; ++i) {
            const bool same = i < used && tk[i] == key;
            tc[i] += same ? 1u : 0u;
            found = found || same;
        }
        const bool fresh = !found && used < kMatteSlots;
#pragma unroll
        for (uint32_t i = 0; i < kMatteSlots; ++i) {
            const bool take = fresh && i == used;
            tk[i] = take ? key : tk[i];
            tc[i] = take ? 1u : tc[i];
        }
        used += fresh ? 1u : 0u;
    }
    /* the kMatteRanks best: a strictly larger count wins, so the earlier slot keeps a tie */
    uint32_t rk[kMatteRanks], rc[kMatteRanks];
#pragma unroll
    for (uint32_t r = 0; r < kMatteRanks; ++r) {
        uint32_t bk = kUnset, bc = 0u, bi = kMatteSlots;
#pragma unroll
        for (uint32_t i = 0; i < kMatteSlots; ++i) {
            const bool better = tc[i] > bc;
            bk = better ? tk[i] : bk;
            bi = better ? i : bi;
            bc = better ? tc[i] : bc;
        }
        rk[r] = bk;
        rc[r] = bc;
#pragma unroll
        for (uint32_t i = 0; i < kMatteSlots; ++i) tc[i] = (i == bi) ? 0u : tc[i];
    }
    float4 oP = make_float4(0.0f, 0.0f, 0.0f, kFarAway), oN = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (nHit > 0u) {
        const float nh = (float)nHit;
        oP = make_float4(sP.x / nh, sP.y / nh, sP.z / nh, sT / nh);
        oN = make_float4(sN.x / nh, sN.y / nh, sN.z / nh, 0.0f);
    }
    const float ns = (float)samples;
    oI.w = nHit;
    pos[lp] = oP;
    nrm[lp] = oN;
    alb[lp] = make_float4(sA.x / ns, sA.y / ns, sA.z / ns, (float)nHit / ns);
    ids[lp] = oI;
    mkey[lp] = make_uint4(rk[0], rk[1], rk[2], rk[3]);
    mcnt[lp] = make_uint4(rc[0], rc[1], rc[2], rc[3]);
}

}  // namespace surfdev
