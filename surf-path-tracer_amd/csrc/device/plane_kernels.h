/* The per-pixel plane passes: first-hit feature buffers (k_aov), the same
 * through mirrors and glass (k_aov_chain), the sampled feature buffers
 * (k_aov_sampled) and ambient occlusion (k_ao), behind the frame the first two
 * share.  Included behind wavefront_kernels.h, whose device functions it calls
 * and whose text it leaves alone.  Every pass reads the scene, the camera or a
 * source plane only: no Counters, no pool, nothing of the captured graph.
 *
 * k_aov_sampled and k_ao keep their own spelling of what the frame states:
 * through any one of these helpers the compiler orders their instructions
 * differently (profiles/plane_passes/resources.txt), and their code is to stay
 * what it was.  The same holds for the surface record (P, N, emitter or not,
 * albedo or strength * colour, material), which all three feature kernels
 * spell out, and for shadePath's copy of the background. */
#pragma once

#include "device/wavefront_kernels.h"

namespace surfdev {

/* ---- the frame ---------------------------------------------------------- */

/* The tables of a pass that traces and shades: the trace tables in dynamic LDS
 * as k_trace_closest stages them (stack, TraceInst, TLAS order), the shade
 * tables in the kernel's static LDS (sInst, sMat, sLights) as k_shade stages
 * them, or both in global memory.  stageTrace and stageTables each end with a
 * barrier, so every lane of the block calls this before the lanes past the
 * last pixel return. */
struct PlaneTables {
    TraceTables Tt;
    ShadeTables Tb;
};
template <bool LDS>
__device__ __forceinline__ PlaneTables stagePlaneTables(const DevScene& S, uint32_t* lds, uint32_t stackWords, DevInstance* sInst,
                                                        DevMaterial* sMat, uint2* sLights) {
    const TraceTables Tt = traceTables<LDS>(S, lds, layout::laneTablesAt(stackWords, false));
    if (!LDS) return PlaneTables{Tt, ShadeTables{S.inst, S.mats, S.lights}};
    stageTables(S, sInst, sMat, sLights);
    return PlaneTables{Tt, ShadeTables{sInst, sMat, sLights}};
}

/* The unjittered camera ray of shard pixel lp: through the pixel's corner
 * (x, row), from the camera position -- no jitter and no lens sample, also for
 * a camera with a defocus angle.  len2 is summed ((0 + x x) + y y) + z z, as
 * the host restatements sum it. */
__device__ __forceinline__ void pixelRay(const DevCamera& cam, const uint32_t* rows, uint32_t width, uint32_t lp, V3& o, V3& d) {
    const uint32_t rowi = lp / width;
    const uint32_t x = lp - rowi * width;
    const uint32_t row = rows[rowi];
    const float u = (float)x * cam.invW, v = (float)row * cam.invH;
    o = ld3(cam.pos);
    const V3 dir = sub(add(add(ld3(cam.firstPixel), lscl(u, ld3(cam.uVec))), lscl(v, ld3(cam.vVec))), o);
    const float len2 = ((0.0f + dir.x * dir.x) + dir.y * dir.y) + dir.z * dir.z;
    const float inv = 1.0f / sqrtf(len2);
    d = scl(dir, inv);
}

/* SceneBackground along d (scene.cpp:35-51), what a ray that misses sees:
 * shadePath's miss term by term.  S is the kernel argument in every caller;
 * its colours are read element by element, never through a pointer into it,
 * so that no copy of the argument is made in scratch. */
__device__ __forceinline__ V3 backgroundAlong(const DevScene& S, V3 d) {
    V3 bg = mk3(0.0f, 0.0f, 0.0f);
    if (S.bgType == 0u) bg = mk3(S.bgColor[0], S.bgColor[1], S.bgColor[2]);
    else if (S.bgType == 1u) {
        const float a = 0.5f * (1.0f + d.y);
        bg = add(lscl(a, mk3(S.bgB[0], S.bgB[1], S.bgB[2])), lscl(1.0f - a, mk3(S.bgA[0], S.bgA[1], S.bgA[2])));
    }
    return bg;
}

/* ---- first-hit feature buffers ------------------------------------------ */

/* First-hit feature buffers (AOVs, surf_read_aov): one lane per shard pixel lp
 * traces the pixel's unjittered camera ray -- through the pixel's corner
 * (x, row), from the camera position: no jitter and no lens sample, also for a
 * camera with a defocus angle, so the planes are sharp and carry no noise --
 * and writes four planar 16-byte records:
 *   pos[lp]  hit: (o + t d, t)                           miss: (0, 0, 0, 1e30)
 *   nrm[lp]  hit: (shadePath's N, 0), emitters included   miss: 0
 *   alb[lp]  hit: (albedo, 1); emitter: (strength * colour, 1)
 *                                                        miss: (background along d, 0)
 *   ids[lp]  hit: (instance, primitive, material, 0)     miss: (~0, ~0, ~0, 0)
 * The expressions are shadePath's / classifyPixels' term by term (f32, no
 * contraction), so a host restatement reproduces every plane bit for bit.
 * The tables are staged as k_trace_closest (dynamic LDS: stack, TraceInst,
 * TLAS order) and k_shade (static LDS) stage them, by every lane of the block
 * before the lanes past the last pixel leave.  Reads the scene and the camera
 * only: no Counters, no pool, nothing of the captured graph. */
template <bool LDS, bool LW = false>
__global__ __launch_bounds__(kBlock) void k_aov(DevScene S, DevCamera cam, const uint32_t* __restrict__ rows, uint32_t width,
                                                uint32_t npx, float4* __restrict__ pos, float4* __restrict__ nrm,
                                                float4* __restrict__ alb, uint4* __restrict__ ids, uint32_t stackWords) {
    extern __shared__ uint32_t lds[];
    __shared__ DevInstance sInst[LDS ? kLdsInst : 1];
    __shared__ DevMaterial sMat[LDS ? kLdsMats : 1];
    __shared__ uint2 sLights[LDS ? kLdsLights : 1];
    const PlaneTables T = stagePlaneTables<LDS>(S, lds, stackWords, sInst, sMat, sLights);   /* every lane: it ends with a barrier */
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npx) return;
    V3 o, d;
    pixelRay(cam, rows, width, lp, o, d);
    float depth = kFarAway, hu = 0.0f, hv = 0.0f;
    uint32_t inst = kUnset, prim = kUnset;
    const bool hit = traceScene<false, LW>(S, T.Tt, o, d, depth, hu, hv, inst, prim, lds + threadIdx.x, blockDim.x);
    float4 oP = make_float4(0.0f, 0.0f, 0.0f, kFarAway), oN = make_float4(0.0f, 0.0f, 0.0f, 0.0f), oA;
    uint4 oI = make_uint4(kUnset, kUnset, kUnset, 0u);
    if (hit) {
        const DevInstance& I = T.Tb.inst[inst];
        const DevMaterial& m = T.Tb.mats[I.material];
        const V3 P = add(o, lscl(depth, d));
        const V3 N = hitNormal(S, I, prim, hu, hv, d);
        const bool isLight = m.emit > 0.0f && (m.ec[0] > 0.0f || m.ec[1] > 0.0f || m.ec[2] > 0.0f);
        const V3 a = isLight ? lscl(m.emit, ld3(m.ec)) : ld3(m.albedo);
        oP = make_float4(P.x, P.y, P.z, depth);
        oN = make_float4(N.x, N.y, N.z, 0.0f);
        oA = make_float4(a.x, a.y, a.z, 1.0f);
        oI = make_uint4(inst, prim, I.material, 0u);
    } else {
        const V3 bg = backgroundAlong(S, d);   /* shadePath's miss */
        oA = make_float4(bg.x, bg.y, bg.z, 0.0f);
    }
    pos[lp] = oP;
    nrm[lp] = oN;
    alb[lp] = oA;
    ids[lp] = oI;
}

/* ---- feature buffers through mirrors and glass -------------------------- */

/* Feature buffers through mirrors and glass (surf_read_aov_chain): k_aov's
 * ray, followed through the delta interactions -- a material with
 * refl + refr >= 0.5 -- to the first surface that is not one, or to the
 * maxLinks-th link.  shadePath's arithmetic with its random choices replaced
 * by a fixed rule and no RNG at all: refl >= refr reflects; a dielectric
 * transmits whenever it can (no Fresnel draw) and reflects otherwise (total
 * internal reflection).  tint is the product of the links' albedo * medium,
 * L the path length summed along the chain, k the links followed:
 *   pos[lp]  surface: (P, L), the terminal point itself     miss: (0, 0, 0, 1e30)
 *   nrm[lp]  surface: (N, 0), turned against the last d     miss: 0
 *   alb[lp]  surface: ((tint * medium) * a, 1), a the albedo or, on an emitter
 *            (where medium = 1, as shadePath's emitter return absorbs nothing),
 *            strength * colour             miss: (tint * background along the last d, 0)
 *   ids[lp]  surface: (instance, primitive, material, k)    miss: (~0, ~0, ~0, k)
 * With maxLinks = 0 every plane is k_aov's bit for bit (1.0f * x is exact),
 * and at any maxLinks so is a pixel whose first hit is not delta.  Tables,
 * dynamic LDS and variants as k_aov; the lanes of a wave leave the loop one
 * by one, which traceScene allows (it holds no wave-wide operation). */
template <bool LDS, bool LW = false>
__global__ __launch_bounds__(kBlock) void k_aov_chain(DevScene S, DevCamera cam, const uint32_t* __restrict__ rows, uint32_t width,
                                                      uint32_t npx, float4* __restrict__ pos, float4* __restrict__ nrm,
                                                      float4* __restrict__ alb, uint4* __restrict__ ids, uint32_t stackWords,
                                                      uint32_t maxLinks) {
    extern __shared__ uint32_t lds[];
    __shared__ DevInstance sInst[LDS ? kLdsInst : 1];
    __shared__ DevMaterial sMat[LDS ? kLdsMats : 1];
    __shared__ uint2 sLights[LDS ? kLdsLights : 1];
    const PlaneTables T = stagePlaneTables<LDS>(S, lds, stackWords, sInst, sMat, sLights);   /* every lane: it ends with a barrier */
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= npx) return;
    V3 o0, d0;
    pixelRay(cam, rows, width, lp, o0, d0);
    V3 o = o0, d = d0;   /* the links move them */
    V3 tint = mk3(1.0f, 1.0f, 1.0f);
    float L = 0.0f;
    bool inMedium = false;
    float4 oP = make_float4(0.0f, 0.0f, 0.0f, kFarAway), oN = make_float4(0.0f, 0.0f, 0.0f, 0.0f), oA = oN;
    uint4 oI = make_uint4(kUnset, kUnset, kUnset, 0u);
    /* at most maxLinks + 1 turns: the turn with k == maxLinks ends at its surface */
    for (uint32_t k = 0; k <= maxLinks; ++k) {
        float depth = kFarAway, hu = 0.0f, hv = 0.0f;
        uint32_t inst = kUnset, prim = kUnset;
        const bool hit = traceScene<false, LW>(S, T.Tt, o, d, depth, hu, hv, inst, prim, lds + threadIdx.x, blockDim.x);
        if (!hit) {
            const V3 c = mul(tint, backgroundAlong(S, d));   /* shadePath's miss */
            oA = make_float4(c.x, c.y, c.z, 0.0f);
            oI.w = k;
            break;
        }
        const DevInstance& I = T.Tb.inst[inst];
        const DevMaterial& m = T.Tb.mats[I.material];
        const bool isLight = m.emit > 0.0f && (m.ec[0] > 0.0f || m.ec[1] > 0.0f || m.ec[2] > 0.0f);
        L = L + depth;
        V3 medium = mk3(1.0f, 1.0f, 1.0f);
        if (inMedium && !isLight) {
            const float nd = -depth;
            medium = mk3(gExpf(m.absorb[0] * nd), gExpf(m.absorb[1] * nd), gExpf(m.absorb[2] * nd));
        }
        const V3 P = add(o, lscl(depth, d));
        const V3 N = hitNormal(S, I, prim, hu, hv, d);
        const bool delta = (m.refl + m.refr) >= 0.5f;
        if (isLight || !delta || k == maxLinks) {
            const V3 a = isLight ? lscl(m.emit, ld3(m.ec)) : ld3(m.albedo);
            const V3 c = mul(mul(tint, medium), a);
            oP = make_float4(P.x, P.y, P.z, L);
            oN = make_float4(N.x, N.y, N.z, 0.0f);
            oA = make_float4(c.x, c.y, c.z, 1.0f);
            oI = make_uint4(inst, prim, I.material, k);
            break;
        }
        tint = mul(tint, mul(ld3(m.albedo), medium));
        V3 R = sub(d, lscl(2.0f * dot(N, d), N));
        if (!(m.refl >= m.refr)) {
            const float n1f = inMedium ? m.ior : 1.0f, n2f = inMedium ? 1.0f : m.ior;
            const float ratio = n1f / n2f;
            const float cosI = -dot(d, N);
            const float cos2 = 1.0f - (ratio * ratio) * (1.0f - cosI * cosI);
            if (cos2 > 0.0f) {
                R = add(lscl(ratio, d), lscl(ratio * cosI - sqrtf(fabsf(cos2)), N));
                inMedium = !inMedium;
            }
        }
        o = add(P, lscl(kEps, R));
        d = R;
    }
    pos[lp] = oP;
    nrm[lp] = oN;
    alb[lp] = oA;
    ids[lp] = oI;
}

/* ---- sampled feature buffers -------------------------------------------- */

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

/* ---- ambient occlusion -------------------------------------------------- */

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
