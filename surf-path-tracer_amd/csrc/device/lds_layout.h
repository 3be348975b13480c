/*
 * lds_layout.h -- the dynamic-LDS layouts of the traversal kernels, stated
 * once: the kernels take their region offsets from these functions and the
 * host takes every launch's LDS byte count (words x 4) and its residency
 * decisions from the same ones.  Plain C++ (no HIP header): everything is in
 * 32-bit words; device/types.h asserts the element sizes used here.
 */
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SURF_LDS_HD __host__ __device__ constexpr
#else
#define SURF_LDS_HD constexpr
#endif

namespace surfdev {
namespace layout {

/* elements of the staged tables, in words */
constexpr uint32_t kTraceInstWords = 44;      /* TraceInst, 176 B */
constexpr uint32_t kTraceEntryWords = kTraceInstWords + 1u;   /* ... and the instance's tlasIdx entry behind the table */
constexpr uint32_t kInstanceWords = 40;       /* DevInstance, 160 B */
constexpr uint32_t kMaterialWords = 16;       /* DevMaterial, 64 B */
constexpr uint32_t kLightWords = 2;           /* uint2 */
constexpr uint32_t kNodeRecWords = 16;        /* a BLAS node record, 4 float4 */
constexpr uint32_t kTriRecWords = 12;         /* a triangle slot, 3 float4 */

/* the next 16-B boundary (float4 / struct tables) */
SURF_LDS_HD uint32_t align4(uint32_t words) { return (words + 3u) & ~3u; }

/* [TraceInst x nInst][tlasIdx x nInst] (stageTrace) */
SURF_LDS_HD uint32_t traceTableWords(uint32_t nInst) { return nInst * kTraceEntryWords; }

/* ---- lane traversal: [stack: depth x block entries][trace tables]
 * (k_extend, k_connect, k_trace_*, k_aov, k_tail).  The kernels
 * get the stack as `stack32`, its words with 32-bit entries. */
SURF_LDS_HD uint32_t laneStack32(uint32_t depth, uint32_t block) { return depth * block; }
SURF_LDS_HD uint32_t laneStackWords(uint32_t stack32, bool entries16) { return entries16 ? (stack32 + 1u) / 2u : stack32; }
SURF_LDS_HD uint32_t laneTablesAt(uint32_t stack32, bool entries16) { return laneStackWords(stack32, entries16); }
SURF_LDS_HD uint32_t laneTotal(uint32_t stack32, bool entries16, bool tables, uint32_t nInst) {
    return laneTablesAt(stack32, entries16) + (tables ? traceTableWords(nInst) : 0u);
}

/* ---- staged k_connect: [16-bit stack][trace tables][emitter BLAS records,
 * 16-B aligned][their triangles] */
SURF_LDS_HD uint32_t stagedTablesAt(uint32_t stack32) { return stack32 / 2u; }
SURF_LDS_HD uint32_t stagedBlasAt(uint32_t stack32, uint32_t nInst) { return align4(stagedTablesAt(stack32) + traceTableWords(nInst)); }
SURF_LDS_HD uint32_t stagedTrisAt(uint32_t stack32, uint32_t nInst, uint32_t recN) {
    return stagedBlasAt(stack32, nInst) + kNodeRecWords * recN;
}
SURF_LDS_HD uint32_t stagedTotal(uint32_t stack32, uint32_t nInst, uint32_t recN, uint32_t triN) {
    return stagedTrisAt(stack32, nInst, recN) + kTriRecWords * triN;
}

/* ---- one ray per wave: per wave [record stack][prologue table], then
 * [trace tables][shading tables, 16-B aligned] (k_trace_*_coop: one wave, no
 * shading tables; k_tail_coop, k_segment_cycles: one wave; k_tail_pair: two).
 * The kernels get the record stack's words as `stack`. */
SURF_LDS_HD uint32_t recStackWords(uint32_t depth, bool twoLevel) { return depth * (twoLevel ? 64u : 16u); }
SURF_LDS_HD uint32_t proWords(uint32_t nInst) { return 16u * nInst; }
SURF_LDS_HD uint32_t wavePerWords(uint32_t stack, uint32_t nInst) { return stack + proWords(nInst); }
SURF_LDS_HD uint32_t waveStackAt(uint32_t stack, uint32_t nInst, uint32_t wave) { return wave * wavePerWords(stack, nInst); }
SURF_LDS_HD uint32_t waveProAt(uint32_t stack, uint32_t nInst, uint32_t wave) { return waveStackAt(stack, nInst, wave) + stack; }
SURF_LDS_HD uint32_t waveTablesAt(uint32_t stack, uint32_t nInst, uint32_t waves) { return waves * wavePerWords(stack, nInst); }
SURF_LDS_HD uint32_t waveShadeAt(uint32_t stack, uint32_t nInst, uint32_t waves) {
    return align4(waveTablesAt(stack, nInst, waves) + traceTableWords(nInst));
}
SURF_LDS_HD uint32_t shadeTableWords(uint32_t nInst, uint32_t nMats, uint32_t nLights) {
    return nInst * kInstanceWords + nMats * kMaterialWords + nLights * kLightWords;
}
SURF_LDS_HD uint32_t waveTraceTotal(uint32_t stack, uint32_t nInst, bool tables) {
    return waveTablesAt(stack, nInst, 1u) + (tables ? traceTableWords(nInst) : 0u);
}
SURF_LDS_HD uint32_t waveTailTotal(uint32_t stack, uint32_t nInst, uint32_t nMats, uint32_t nLights, bool tables, uint32_t waves) {
    return tables ? waveShadeAt(stack, nInst, waves) + shadeTableWords(nInst, nMats, nLights) : waveTablesAt(stack, nInst, waves);
}

/* Representative points: the bundled scene's tables (11 instances, 8
 * materials, 2 lights) at a depth of 24, and the largest staged tables (64
 * instances, materials and lights) at depth 120.
 * Regions do not overlap, the 16-B alignments hold, each total is the end of
 * its last region. */
namespace check {
constexpr uint32_t kN[2] = {11u, 64u}, kM[2] = {8u, 64u}, kL[2] = {2u, 64u}, kD[2] = {24u, 120u}, kBlocks[3] = {64u, 128u, 256u};
constexpr bool lane(uint32_t n, uint32_t d, uint32_t block, bool e16) {
    const uint32_t s = laneStack32(d, block);
    return laneTablesAt(s, e16) * (e16 ? 2u : 1u) >= d * block &&              /* the stack's entries end before the tables */
           laneTotal(s, e16, true, n) == laneTablesAt(s, e16) + traceTableWords(n) && laneTotal(s, e16, false, n) == laneStackWords(s, e16);
}
constexpr bool staged(uint32_t n, uint32_t d, uint32_t recN, uint32_t triN) {
    const uint32_t s = laneStack32(d, 256u);
    return stagedTablesAt(s) * 2u >= d * 256u && stagedBlasAt(s, n) >= stagedTablesAt(s) + traceTableWords(n) &&
           stagedBlasAt(s, n) % 4u == 0u && stagedTrisAt(s, n, recN) == stagedBlasAt(s, n) + 16u * recN &&
           stagedTrisAt(s, n, recN) % 4u == 0u && stagedTotal(s, n, recN, triN) == stagedTrisAt(s, n, recN) + 12u * triN;
}
constexpr bool wave(uint32_t n, uint32_t m, uint32_t l, uint32_t d, bool w2, uint32_t waves) {
    const uint32_t s = recStackWords(d, w2), last = waves - 1u;
    return waveProAt(s, n, 0u) == s && waveProAt(s, n, 0u) % 4u == 0u && waveProAt(s, n, last) % 4u == 0u &&
           waveProAt(s, n, last) + proWords(n) == waveTablesAt(s, n, waves) &&
           (waves == 1u || waveStackAt(s, n, 1u) == waveProAt(s, n, 0u) + proWords(n)) && waveTablesAt(s, n, waves) % 4u == 0u &&
           waveShadeAt(s, n, waves) >= waveTablesAt(s, n, waves) + traceTableWords(n) && waveShadeAt(s, n, waves) % 4u == 0u &&
           waveTraceTotal(s, n, true) == waveTablesAt(s, n, 1u) + traceTableWords(n) && waveTraceTotal(s, n, false) == wavePerWords(s, n) &&
           waveTailTotal(s, n, m, l, true, waves) == waveShadeAt(s, n, waves) + shadeTableWords(n, m, l) &&
           waveTailTotal(s, n, m, l, false, waves) == waves * wavePerWords(s, n);
}
constexpr bool all() {
    bool ok = true;
    for (int k = 0; k < 2; ++k) {
        for (uint32_t block : kBlocks) ok = ok && lane(kN[k], kD[k], block, false) && lane(kN[k], kD[k], block, true);
        ok = ok && staged(kN[k], kD[k], 11u, 12u) && staged(kN[k], kD[k], 0u, 0u);
        for (uint32_t waves = 1u; waves <= 2u; ++waves)
            ok = ok && wave(kN[k], kM[k], kL[k], kD[k], false, waves) && wave(kN[k], kM[k], kL[k], kD[k], true, waves);
    }
    return ok;
}
static_assert(all(), "LDS regions overlap, are misaligned, or a total is not the end of its last region");
static_assert(lane(11u, 24u, 255u, true), "an odd 16-bit stack rounds up to a whole word");
}  // namespace check

}  // namespace layout
}  // namespace surfdev
