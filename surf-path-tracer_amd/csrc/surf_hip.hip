/*
 * surf_hip.hip -- the kernels' translation unit: kernel selection, the
 * wavefront render loop (hipGraph-captured phases), the sample stream's pump
 * and drain, feature buffers and the C ABI (include/surf_hip.h) around them.
 * Replaces WaveFrontRenderer's Vulkan orchestration
 * (renderer.cpp:604-1454) -- without its per-bounce host round trip: the
 * host only polls a pinned counter block once per replayed graph of
 * kPhasesPerGraph phases.  Scene validation and re-layout launch no kernel
 * and live in host/scene_upload.hip; the image-space filters, with their
 * kernels, each in a file of host/.
 */
#include "host/surf_ctx.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>

#include "device/wavefront_kernels.h"
#include "device/plane_kernels.h"

namespace {

/* phases per full replay: 16 (C3 515.2 / 513.9 → 520.7 / 520.0 Mrays/s against
 * 8 on one box, C4, the drop-in loop and the 8-shard projection unchanged;
 * MEASUREMENTS r6) */
#ifndef SURF_PHASES_GRAPH
#define SURF_PHASES_GRAPH 16
#endif
constexpr int kPhasesPerGraph = SURF_PHASES_GRAPH;   /* even: parity returns to 0 after a replay */
static_assert(kPhasesPerGraph % 2 == 0, "even: parity returns to 0 after a replay");
/* The short graph: a render call with at most one frame left to issue (the
 * drop-in loop's 1-spp render(), main.cpp:381-446) replays 4 phases per host
 * poll instead of 16, so a per-frame call does not keep the pool a quarter full
 * for 16 phases per frame.  4096 one-frame calls at 1280x720: 625 / 641 / 637
 * Mrays/s with 2 / 4 / 8 phases (each replay's end joins its last k_connect,
 * which then overlaps nothing; MEASUREMENTS round 5). */
#ifndef SURF_PHASES_SHORT
#define SURF_PHASES_SHORT 4
#endif
constexpr int kPhasesShort = SURF_PHASES_SHORT;
static_assert(kPhasesShort % 2 == 0 && kPhasesShort <= kPhasesPerGraph, "even: parity returns to 0 after a replay");
constexpr int kPhaseEvents = 6;             /* profiling events per phase: sort, extend, shade, sort, connect, regen */
constexpr uint64_t kMaxIterations = 1ull << 22;  /* safety net: a path longer than this is a bug */

std::mutex gErrMutex;
std::string gLastError;

}  // namespace

void surfhost::setGlobalError(const std::string& e) { std::lock_guard<std::mutex> l(gErrMutex); gLastError = e; }

void surfhost::destroyGraph(surf_ctx* c) {
    if (c->graphExec) (void)hipGraphExecDestroy(c->graphExec);
    if (c->graph) (void)hipGraphDestroy(c->graph);
    if (c->graphExecShort) (void)hipGraphExecDestroy(c->graphExecShort);
    if (c->graphShort) (void)hipGraphDestroy(c->graphShort);
    c->graphExec = c->graphExecShort = nullptr;
    c->graph = c->graphShort = nullptr;
    if (c->graphExecM) (void)hipGraphExecDestroy(c->graphExecM);
    if (c->graphM) (void)hipGraphDestroy(c->graphM);
    if (c->graphExecShortM) (void)hipGraphExecDestroy(c->graphExecShortM);
    if (c->graphShortM) (void)hipGraphDestroy(c->graphShortM);
    c->graphExecM = c->graphExecShortM = nullptr;
    c->graphM = c->graphShortM = nullptr;
}

namespace {

/* ---- kernel selection -----------------------------------------------------
 * Everything the context decides about a launch is decided here: the facts
 * that pick an instantiation (Variant), one selector per kernel family, and
 * with each choice the dynamic LDS it needs -- taken from the layout the
 * kernel itself reads (device/lds_layout.h), so an instantiation and its LDS
 * size cannot be paired wrongly at a call site.  Nothing below this section
 * spells a kernel's template arguments. */

/* an instantiation and the dynamic LDS bytes a launch of it needs */
template <class F>
struct Kernel { F fn; size_t lds; };
template <class F>
Kernel<F> kernel(F fn, size_t lds) { return {fn, lds}; }

size_t ldsBytes(uint32_t words) { return (size_t)words * sizeof(uint32_t); }

/* the kernels' `stackWords` argument: the lane kernels' stack with 32-bit
 * entries, the wave kernels' stack of node records */
uint32_t stackWords(const surf_ctx* c, uint32_t block) { return layout::laneStack32(c->stackDepth, block); }
uint32_t recStackWords(const surf_ctx* c) { return layout::recStackWords(c->stackDepth, c->S.wnodes != nullptr); }

size_t laneLds(const surf_ctx* c, uint32_t block, bool entries16, bool tables) {
    return ldsBytes(layout::laneTotal(stackWords(c, block), entries16, tables, c->nInstances));
}
size_t stagedLds(const surf_ctx* c) {
    return ldsBytes(layout::stagedTotal(stackWords(c, kBlock), c->nInstances, c->S.sbRecN, c->S.sbTriN));
}
size_t waveTraceLds(const surf_ctx* c) { return ldsBytes(layout::waveTraceTotal(recStackWords(c), c->nInstances, c->ldsTables)); }
size_t waveTailLds(const surf_ctx* c, uint32_t waves) {
    return ldsBytes(layout::waveTailTotal(recStackWords(c), c->nInstances, c->nMaterials, c->nLightsUp, c->ldsTables, waves));
}
/* the one-ray-per-wave kernels fit the LDS: the largest of them, k_tail_pair, within 64 KiB */
bool coopLdsOk(const surf_ctx* c) { return waveTailLds(c, 2u) <= 65536; }

struct Variant {
    bool lds;      /* the trace and shading tables fit the per-workgroup LDS copy */
    bool laneW;    /* the lane walk over the two-level records (HBM-resident BVHs) */
    bool w2;       /* the wave walk over the two-level records */
    bool sk16;     /* k_extend's stack in 16-bit entries: every node index fits (the two-level lane walk stacks 32-bit packed leaf references) */
    bool ldsC;     /* k_connect's tables in LDS (else global: LDS holds only its stack) */
    bool stg;      /* ... and the emitters' BLAS beside them, behind a 16-bit stack */
};
Variant variantOf(const surf_ctx* c) {
    Variant v;
    v.lds = c->ldsTables;
    v.laneW = c->S.laneW != 0u;
    v.w2 = c->S.wnodes != nullptr;
    v.sk16 = c->extStack16 && !v.laneW && c->nBlasNodes < 65536u && c->tlasNodeCount < 65536u;
    v.ldsC = v.lds && !c->connectGlobal;
    /* staged only where the copy still leaves 5 workgroups of 256 per CU
     * (k_connect's residency; 144 B of static LDS each) */
    v.stg = v.ldsC && !v.laneW && c->S.sbRecN > 0u && (stagedLds(c) + 256) * 5 <= 163840;
    return v;
}

/* the four instantiations of a kernel template over two bools */
#define SURF_PICK2(K, a, b) ((a) ? ((b) ? K<true, true> : K<true, false>) : ((b) ? K<false, true> : K<false, false>))
/* ... and of one whose third argument, SF, is a compile-time constant at the call site */
#define SURF_PICK2S(K, a, b, SF) ((a) ? ((b) ? K<true, true, SF> : K<true, false, SF>) : ((b) ? K<false, true, SF> : K<false, false, SF>))

/* The sensor of the context's stream -- the camera, or the caller's surfels
 * (surf_set_surfel_sensor) -- picks the SURFEL argument of every kernel that
 * starts a sample (k_regen*, k_shade and the drains) and, with it, the type of
 * the kernel's stream-geometry argument (Geom<SURFEL>): f(std::bool_constant<SURFEL>)
 * launches with the selectors below and geomArg, both instantiated on it. */
template <class F>
void withSensor(const surf_ctx* c, F&& f) {
    if (c->ssOn) f(std::true_type{});
    else f(std::false_type{});
}

/* k_extend<LDS, LW, SK>: 6 of the 8 -- the two-level lane walk never takes a 16-bit stack */
template <bool LDS>
auto extendFn(const Variant& v) {
    if (v.laneW) return k_extend<LDS, true, uint32_t>;
    if (v.sk16) return k_extend<LDS, false, uint16_t>;
    return k_extend<LDS, false, uint32_t>;
}
auto extendKernel(const surf_ctx* c, const Variant& v) {
    return kernel(v.lds ? extendFn<true>(v) : extendFn<false>(v), laneLds(c, c->extBlock, v.sk16, v.lds) + c->extLdsPad);
}

/* k_shade<LDS, HV>: HV with the shadow key's heavy-box layouts (SURF_SH_KEY 1, 2) */
template <bool SF>
auto shadeKernel(const surf_ctx* c, const Variant& v) { return SURF_PICK2S(k_shade, v.lds, c->Q.bins > kShBinsBase, SF); }

/* k_connect<LDS, LW, STG>: staged only over LDS tables and one-level records */
auto connectKernel(const surf_ctx* c, const Variant& v) {
    const auto fn = v.laneW ? (v.ldsC ? k_connect<true, true, false> : k_connect<false, true, false>)
                   : v.stg ? k_connect<true, false, true>
                           : (v.ldsC ? k_connect<true, false, false> : k_connect<false, false, false>);
    return kernel(fn, (v.stg ? stagedLds(c) : laneLds(c, kBlock, false, v.ldsC)) + c->conLdsPad);
}

/* the lane kernels of 256 threads over <LDS, LW>, and k_tail's 64 */
auto traceClosestKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_trace_closest, v.lds, v.laneW), laneLds(c, kBlock, false, v.lds)); }
auto traceAnyKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_trace_any, v.lds, v.laneW), laneLds(c, kBlock, false, v.lds)); }
auto aovKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_aov, v.lds, v.laneW), laneLds(c, kBlock, false, v.lds)); }
auto aovChainKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_aov_chain, v.lds, v.laneW), laneLds(c, kBlock, false, v.lds)); }
auto aovSampledKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_aov_sampled, v.lds, v.laneW), laneLds(c, kBlock, false, v.lds)); }
/* k_ao<LDS, LW, RAY>: the lane mapping is the context's (SURF_AO_MAP) */
template <bool RAY>
auto aoFn(const Variant& v) {
    return v.lds ? (v.laneW ? k_ao<true, true, RAY> : k_ao<true, false, RAY>) : (v.laneW ? k_ao<false, true, RAY> : k_ao<false, false, RAY>);
}
auto aoKernel(const surf_ctx* c, const Variant& v) { return kernel(c->aoRayMap ? aoFn<true>(v) : aoFn<false>(v), laneLds(c, kBlock, false, v.lds)); }
static_assert(kAoSeedSalt == SURF_AO_SEED_SALT, "the kernel's salt is the header's");
template <bool SF>
auto tailKernel(const surf_ctx* c, const Variant& v) { return kernel(v.lds ? k_tail<true, SF> : k_tail<false, SF>, laneLds(c, 64, false, v.lds)); }

/* the one-ray-per-wave kernels over <LDS, W2> */
template <bool SF>
auto tailPairKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2S(k_tail_pair, v.lds, v.w2, SF), waveTailLds(c, 2u)); }
template <bool SF>
auto tailCoopKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2S(k_tail_coop, v.lds, v.w2, SF), waveTailLds(c, 1u)); }
auto segmentCyclesKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_segment_cycles, v.lds, v.w2), waveTailLds(c, 1u)); }
/* planted paths (surf_debug_trace_paths): the lane kernels' and the cooperative drain's variants and LDS */
auto debugPathsLaneKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_debug_paths_lane, v.lds, v.laneW), laneLds(c, kBlock, false, v.lds)); }
auto debugPathsWaveKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_debug_paths_wave, v.lds, v.w2), waveTailLds(c, 1u)); }
auto traceClosestCoopKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_trace_closest_coop, v.lds, v.w2), waveTraceLds(c)); }
auto traceAnyCoopKernel(const surf_ctx* c, const Variant& v) { return kernel(SURF_PICK2(k_trace_any_coop, v.lds, v.w2), waveTraceLds(c)); }

/* k_accumulate<SQUARES>: the squares plane rides the sum where surf_set_sample_squares switched it on */
auto accumulateKernel(const surf_ctx* c) { return c->sqOn ? k_accumulate<true> : k_accumulate<false>; }
/* ... and a masked stream's frames go through the active list */
auto accumulateListKernel(const surf_ctx* c) { return c->sqOn ? k_accumulate_list<true> : k_accumulate_list<false>; }
/* k_accumulate_buckets<SQUARES, M> / k_accumulate_buckets_list<SQUARES, M>: chosen instead while
 * surf_set_sample_buckets has M planes on (c->bkM is 2, 4, 8 or 16) */
#define SURF_PICK_BUCKETS(K, SQ, M) \
    ((M) == 2u ? ((SQ) ? K<true, 2u> : K<false, 2u>) : (M) == 4u ? ((SQ) ? K<true, 4u> : K<false, 4u>) \
     : (M) == 8u ? ((SQ) ? K<true, 8u> : K<false, 8u>) : ((SQ) ? K<true, 16u> : K<false, 16u>))
auto accumulateBucketsKernel(const surf_ctx* c) { return SURF_PICK_BUCKETS(k_accumulate_buckets, c->sqOn, c->bkM); }
auto accumulateBucketsListKernel(const surf_ctx* c) { return SURF_PICK_BUCKETS(k_accumulate_buckets_list, c->sqOn, c->bkM); }
/* k_regen<MASKED> / k_regen_count<MASKED>: a masked stream issues frame-major over the active list */
template <bool SF>
auto regenKernel(const surf_ctx* c) { return c->streamMasked ? k_regen<true, SF> : k_regen<false, SF>; }
template <bool SF>
auto regenCountKernel(const surf_ctx* c) { return c->streamMasked ? k_regen_count<true, SF> : k_regen_count<false, SF>; }
/* shadow-queue order bins in use: the key layout's (SURF_SH_KEY, shadowKey), or 1 without a shadow order */
uint32_t shadowBins(const surf_ctx* c) {
    static const uint32_t kLayoutBins[3] = {kShBinsBase, 2u * kShBinsBase, kShBins};
    return (c->sortRays && c->sortShadow) ? kLayoutBins[c->shKey] : 1u;
}

int allocWavefront(surf_ctx* c) {
    if (c->allocated) return SURF_OK;
    if (c->capacity == 0) {
        /* default: 5 full frames of paths in flight, bounded at 16M paths
         * (measured, DESIGN §4 "Pool sizing": C3 435-439 -> 470-475 Mrays/s
         * from 4 to 5 frames, 4.5 frames no better than 4, 6 slower again).
         * Sized from the whole frame, not the shard: a row shard of G GPUs
         * keeps the same pool, so its stream needs ~G times fewer wavefront
         * phases (each phase pays launch and poll latency however few paths it
         * holds). */
        const uint64_t want = (uint64_t)c->width * c->height * 5;
        c->capacity = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 65536), 1u << 24);
    }
    const size_t cap = c->capacity;
    int rc;
    for (int p = 0; p < 2; ++p) {
        if ((rc = devAlloc(c, c->wfAllocs, &c->pool[p].od, 2 * cap))) return rc;
        if ((rc = devAlloc(c, c->wfAllocs, &c->pool[p].T, cap))) return rc;
        if ((rc = devAlloc(c, c->wfAllocs, &c->pool[p].key, cap))) return rc;
    }
    if ((rc = devAlloc(c, c->wfAllocs, &c->order, cap))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->binHist, (size_t)kBins * kSortBlocks))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->dPerm, c->npx))) return rc;
    /* grid: 8 workgroups of 256 per CU saturate the 256-CU chip; grid-stride beyond */
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    /* drain stages: survivors of a tail stage, ping-pong */
    c->survCap = (uint32_t)std::min<size_t>(std::max<size_t>(cap / 16, 4096), 1u << 18);
    for (int q = 0; q < 2; ++q) {
        if ((rc = devAlloc(c, c->wfAllocs, &c->surv[q].od, 2 * (size_t)c->survCap))) return rc;
        if ((rc = devAlloc(c, c->wfAllocs, &c->surv[q].T, c->survCap))) return rc;
    }
    if ((rc = devAlloc(c, c->wfAllocs, &c->hitTUV, cap))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->hitInst, cap))) return rc;
    /* shadow queue: the key layout's bin regions -- 16 of a quarter pool each
     * (a phase queues at most one shadow ray per path; C3 puts <= 30 % of them
     * in one bin), 32 of an eighth or 40 of a tenth: four pools of slots in
     * every layout -- then an overflow region of a whole pool */
    c->Q.bins = shadowBins(c);
    const size_t perPool = (size_t)std::max(c->Q.bins, kShBinsBase) / 4 * kShXcds;    /* regions per pool of slots */
    c->Q.region = (uint32_t)(((c->shRegion ? std::min<size_t>(c->shRegion, cap) : cap / perPool) + 255) / 256 * 256);
    const size_t qslots = (size_t)shOverflowSeg(c->Q.bins) * c->Q.region + cap;
    if ((rc = devAlloc(c, c->wfAllocs, &c->Q.od, 2 * qslots))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->Q.c, qslots))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->Q.cur, (size_t)2 * kShSegs * kShStride))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->ctr, 1))) return rc;
    if ((rc = devAlloc(c, c->wfAllocs, &c->dOutRGBA, c->npx))) return rc;
    if (hipHostMalloc((void**)&c->hctr, sizeof(Counters), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc((void**)&c->hLimit, surf_ctx::kLimitRing * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess)
        return fail(c, SURF_ERR_OOM, "hipHostMalloc of the counter block failed");
    for (auto& sn : c->snap) {
        if (hipHostMalloc((void**)&sn.h, sizeof(Counters), hipHostMallocDefault) != hipSuccess)
            return fail(c, SURF_ERR_OOM, "hipHostMalloc of a counter snapshot failed");
        SURF_CHECK(c, hipEventCreateWithFlags(&sn.ev, hipEventDisableTiming));
    }
    for (auto& pr : c->tev)
        for (auto& e : pr) SURF_CHECK(c, hipEventCreate(&e));
    for (auto& e : c->pev) SURF_CHECK(c, hipEventCreate(&e));
    if (const char* e = std::getenv("SURF_PHASE_LOG")) {         /* diagnostics: per-phase cost vs size */
        if (hipHostMalloc((void**)&c->hPhaseN, kPhasesPerGraph * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
            return fail(c, SURF_ERR_OOM, "hipHostMalloc of the phase log failed");
        c->phaseLog = std::fopen(e, "a");
    }
    const uint64_t maxBlocks = (cap + kBlock - 1) / kBlock;
    uint64_t perCu = 8;                                   /* workgroups per CU of the wavefront kernels (SURF_GRID_PER_CU) */
    if (const char* e = std::getenv("SURF_GRID_PER_CU")) perCu = (uint64_t)std::max(1, std::atoi(e));
    c->gridWork = (uint32_t)std::min<uint64_t>(maxBlocks, (uint64_t)cus * perCu);
    /* per-kernel grids (measured): k_extend gains from one ray per
     * thread (latency hiding across many short-lived blocks), k_connect peaks
     * at 14-15 workgroups per CU with its LDS-staged light BLAS (5 resident:
     * the dispatcher rebalances the grid-stride chunks; past ~15 every extra
     * workgroup re-stages the BLAS -- MEASUREMENTS round 5), k_shade at 8 */
    uint64_t extPerCu = 48, conPerCu = 15;
    const char* eExt = std::getenv("SURF_GRID_EXTEND");
    if (eExt) extPerCu = (uint64_t)std::max(1, std::atoi(eExt));
    if (const char* e = std::getenv("SURF_GRID_CONNECT")) conPerCu = (uint64_t)std::max(1, std::atoi(e));
    if (c->extBlock == 128) extPerCu *= 2;                 /* the same threads per CU in half-size workgroups */
    c->gridExtend = (uint32_t)std::min<uint64_t>((cap + c->extBlock - 1) / c->extBlock, (uint64_t)cus * extPerCu);
    /* k_extend: ~1.5 rays per thread at a full pool (grid-stride).  Measured
     * (DESIGN §4 "Pool sizing"): with the heavy-first ray order the launch
     * time is flat from 1.2 to 1.5 rays per thread (C3 117-118 ms per render at
     * 48-56 workgroups per CU), slower at one ray per thread (131 ms) and at
     * >= 1.7 (C3 127 ms at 36; C4: 1.56 -> 1094 ms, 3.1 -> 1170 ms) */
    if (!eExt) c->gridExtend = (uint32_t)std::max<uint64_t>(c->gridExtend, (cap * 2 / 3 + c->extBlock - 1) / c->extBlock);
    c->gridConnect = (uint32_t)std::min<uint64_t>(maxBlocks, (uint64_t)cus * conPerCu);
    c->coopMax = (uint32_t)cus * 4 * SURF_TAIL_WAVES;
    c->cus = (uint32_t)cus;
    if (const char* e = std::getenv("SURF_DRAIN_REPLAYS")) c->drainReplays = std::max(1, std::atoi(e));
    c->gridRegen = (uint32_t)std::min<uint64_t>(maxBlocks, (uint64_t)cus * 8);
    c->allocated = true;
    return SURF_OK;
}

/* The radiance ring (float4 per frame slot x pixel) and the per-slot
 * completion counters, sized for the stream about to start (no stream active):
 * as many slots as the stream requests frames -- so no frame waits for an old
 * frame's long Russian-roulette paths to free a slot -- at least kWindowFloor,
 * and at least kLoopFloor for a stream opened by a one-frame request (a
 * drop-in loop extends its stream one frame per call, so its first request
 * says nothing about its length; 4096 one-frame calls at 1280x720 run at
 * 552 / 593 / 614 Mrays/s with 1024 / 2048 / 4096 slots, MEASUREMENTS round 5), at most
 * 4096 and at most what min(64 GiB, a quarter of the free HBM) holds (HBM3E:
 * 288 GB per GPU; 4096 slots at 1280x720 take 60 GB).  A
 * later, longer stream grows the ring; a window set by surf_set_frame_batch
 * is kept as given. */
constexpr uint64_t kWindowFloor = 256, kLoopFloor = 4096;
int ensureWindow(surf_ctx* c, uint64_t frames, uint32_t spp) {
    const uint64_t passes = frames * spp;
    const uint64_t floor = frames == 1 ? kLoopFloor : kWindowFloor;
    uint64_t want = c->windowFixed ? c->window : std::min<uint64_t>(4096, std::max<uint64_t>(passes, floor));
    if (c->windowFixed && c->window % spp != 0)
        return fail(c, SURF_ERR_INVALID, "frame window " + std::to_string(c->window) + " is not a multiple of samples_per_frame " +
                                             std::to_string(spp));
    if (!c->windowFixed) {
        uint64_t budget = 64ull << 30;
        size_t freeB = 0, totalB = 0;
        if (hipMemGetInfo(&freeB, &totalB) == hipSuccess && freeB > 0)
            budget = std::min<uint64_t>(budget, (freeB + (c->rad ? (size_t)c->npx * c->window * sizeof(float4) : 0)) / 4);
        want = std::max<uint64_t>(1, std::min<uint64_t>(want, budget / ((uint64_t)c->npx * sizeof(float4))));
        /* a frame's samples take consecutive slots of one window turn */
        want = std::max<uint64_t>(spp, want / spp * spp);
        if ((uint64_t)c->npx * want >= (1ull << 32))
            return fail(c, SURF_ERR_OOM, "radiance ring of " + std::to_string(want) + " passes exceeds 32-bit sample ids");
        if (c->rad && want <= c->window && c->window % spp == 0) return SURF_OK;
    }
    if (c->rad && want == c->window) return SURF_OK;
    if (c->rad) {
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
        (void)hipFree(c->rad); (void)hipFree(c->frameDone);
        for (auto& sn : c->snap) { (void)hipHostFree(sn.fd); sn.fd = nullptr; }
        c->rad = nullptr; c->frameDone = nullptr;
        destroyGraph(c);                          /* the ring and the window are kernel arguments */
    }
    c->window = (uint32_t)want;
    bool ok = hipMalloc(&c->rad, (size_t)c->npx * c->window * sizeof(float4)) == hipSuccess &&
              hipMalloc(&c->frameDone, (size_t)kStripes * c->window * sizeof(uint32_t)) == hipSuccess;
    for (auto& sn : c->snap)
        ok = ok && hipHostMalloc((void**)&sn.fd, (size_t)kStripes * c->window * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        if (c->rad) (void)hipFree(c->rad);
        if (c->frameDone) (void)hipFree(c->frameDone);
        for (auto& sn : c->snap) { if (sn.fd) (void)hipHostFree(sn.fd); sn.fd = nullptr; }
        c->rad = nullptr; c->frameDone = nullptr;
        return fail(c, SURF_ERR_OOM, "radiance ring of " + std::to_string(c->window) + " frames does not fit");
    }
    return SURF_OK;
}

/* (a masked stream's issue list takes the place of the class order it never uses) */
StreamGeom geom(const surf_ctx* c) {
    return StreamGeom{c->dRows, c->width, c->npx, c->window, c->streamMasked ? (const uint32_t*)c->pmList : (const uint32_t*)c->dPerm};
}
/* ... as the kernels of withSensor's choice take it: a sensor stream's carries the sensor's two planes */
template <bool SF>
Geom<SF> geomArg(const surf_ctx* c) {
    if constexpr (SF) return SurfelGeom{geom(c), c->ssPlanes[0], c->ssPlanes[1]};
    else return geom(c);
}

/* Counting sort of the pool (which 0) or shadow queue (which 1) of phase par
 * by its 4-bit key into c->order. */
void launchSort(surf_ctx* c, const uint8_t* key, int par, int which, hipStream_t st, uint32_t* hist, uint32_t* out, bool count = true) {
    if (count)   /* (else k_regen_count left the counts) */
        hipLaunchKernelGGL(k_bincount, dim3(kSortBlocks), dim3(kSortThreads), 0, st, key, (const Counters*)c->ctr, par, which, hist);
#if !SURF_SORT_FUSED_SCAN
    hipLaunchKernelGGL(k_binscan, dim3(1), dim3(1024), 0, st, hist, kBins * kSortBlocks);
#endif
    hipLaunchKernelGGL(k_binscatter, dim3(kSortBlocks), dim3(kSortThreads), 0, st, key, (const Counters*)c->ctr, par, which,
                       (const uint32_t*)hist, out);
}

/* One wavefront phase (ph = 0..kPhasesPerGraph-1): sort -> extend -> shade
 * -> sort -> connect -> regen.  With ev != null, ev[0..5] are recorded before
 * the pool sort, k_extend, k_shade, the shadow sort, k_connect and k_regen
 * (the phase ends at the next phase's ev[0]); everything on one stream.
 * Overlapped (graph capture, c->overlap): the shadow sort and k_connect of
 * phase ph run on the side stream, beside k_regen and the next phase's pool
 * sort and k_extend, which do not touch what they use (the shadow queue, its
 * order and histograms, the radiance of paths still being shaded); the next
 * k_shade waits for them: it reuses the shadow queue, and a path's NEE
 * contribution of bounce i must be added before what bounce i+1 adds. */
void launchPhase(surf_ctx* c, int ph, hipEvent_t* ev) {
    const int par = ph & 1;
    const Variant v = variantOf(c);
    const bool ovl = !ev && c->overlap;
    hipStream_t s0 = c->stream, s1 = ovl ? c->side : c->stream;
    if (ev && c->phaseLog)
        (void)hipMemcpyAsync(&c->hPhaseN[ph], &c->ctr->nIn[par], sizeof(uint32_t), hipMemcpyDeviceToHost, s0);
    if (ev) (void)hipEventRecord(ev[0], s0);
    const uint32_t* order = nullptr;
    const bool sortOn = c->sortRays && c->sortPool;
    const bool fused = sortOn && c->regenCount;    /* k_regen_count counts the next pool for its sort */
    if (sortOn) {
        launchSort(c, c->pool[par].key, par, 0, s0, c->binHist, c->order, !fused);
        order = c->order;
    }
    auto regen = [&]() {
        withSensor(c, [&](auto sf) {
            constexpr bool SF = decltype(sf)::value;
            if (fused)
                hipLaunchKernelGGL(regenCountKernel<SF>(c), dim3(kSortBlocks), dim3(kSortThreads), 0, s0, c->cam, c->pool[par ^ 1], c->rad,
                                   c->ctr, par, c->capacity, geomArg<SF>(c), c->Q, c->binHist);
            else
                hipLaunchKernelGGL(regenKernel<SF>(c), dim3(c->gridRegen), dim3(kBlock), 0, s0, c->cam, c->pool[par ^ 1], c->rad, c->ctr,
                                   par, c->capacity, geomArg<SF>(c), c->Q);
        });
    };
    if (ev) (void)hipEventRecord(ev[1], s0);
    const Pool cur = c->pool[par];                 /* the pool k_extend / k_shade read */
    const auto extend = extendKernel(c, v);
    hipLaunchKernelGGL(extend.fn, dim3(c->gridExtend), dim3(c->extBlock), extend.lds, s0, c->S,
                       cur, c->hitTUV, c->hitInst, (const Counters*)c->ctr, par, stackWords(c, c->extBlock), order);
    if (ev) (void)hipEventRecord(ev[2], s0);
    if (ovl && ph > 0) (void)hipStreamWaitEvent(s0, c->capEv[2 * (ph - 1) + 1], 0);   /* the previous phase's connect */
    withSensor(c, [&](auto sf) {
        constexpr bool SF = decltype(sf)::value;
        hipLaunchKernelGGL(shadeKernel<SF>(c, v), dim3(c->gridWork), dim3(kBlock), 0, s0, c->S, cur, c->pool[par ^ 1],
                           c->hitTUV, (const uint32_t*)c->hitInst, c->Q, c->rad, c->frameDone, c->npx, c->window, c->ctr, par, order,
                           c->cam, geomArg<SF>(c));
    });
    if (ev) (void)hipEventRecord(ev[3], s0);
    /* k_regen before the fork (SURF_REGEN_FIRST): alone it takes ~17 us, beside
     * k_connect it waits for CU slots on the next phase's critical path */
    if (c->regenFirst) regen();
    if (ovl) {
        (void)hipEventRecord(c->capEv[2 * ph], s0);
        (void)hipStreamWaitEvent(s1, c->capEv[2 * ph], 0);
    }
    /* (the shadow rays are already in bin order: k_shade appends each to its
     * bin's region of the queue -- no sort pass) */
    if (ev) (void)hipEventRecord(ev[4], s0);
    /* staged (the emitters' BLAS in LDS): 16-bit stack entries (half the
     * stack's LDS) leave room for the copy beside 5 workgroups of 256 per CU,
     * the residency k_connect runs at */
    c->connectStaged = v.stg;
    const auto connect = connectKernel(c, v);
    hipLaunchKernelGGL(connect.fn, dim3(c->gridConnect), dim3(kBlock), connect.lds, s1, c->S, c->Q, c->rad, c->ctr, par,
                       stackWords(c, kBlock));
    if (ovl) (void)hipEventRecord(c->capEv[2 * ph + 1], s1);
    if (ev) (void)hipEventRecord(ev[5], s0);
    if (!c->regenFirst) regen();
}

int buildGraph(surf_ctx* c) {
    const bool m = c->streamMasked;            /* the graphs of the open stream's kind */
    if (m ? c->graphExecM : c->graphExec) return SURF_OK;
    for (int shortG = 0; shortG < 2; ++shortG) {
        SURF_CHECK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        const int nph = shortG ? kPhasesShort : kPhasesPerGraph;
        for (int ph = 0; ph < nph; ++ph) launchPhase(c, ph, nullptr);
        if (c->overlap) (void)hipStreamWaitEvent(c->stream, c->capEv[2 * (nph - 1) + 1], 0);   /* join the last connect */
        hipGraph_t& g = m ? (shortG ? c->graphShortM : c->graphM) : (shortG ? c->graphShort : c->graph);
        hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e));
        hipGraphExec_t* ex = m ? (shortG ? &c->graphExecShortM : &c->graphExecM) : (shortG ? &c->graphExecShort : &c->graphExec);
        SURF_CHECK(c, hipGraphInstantiate(ex, g, nullptr, nullptr, 0));
    }
    return SURF_OK;
}

/* Closest hits of n host rays (o, d: 3 floats per ray) on the context's
 * stream: upload, k_trace_closest -- one ray per lane, or per wave (perWave:
 * k_trace_closest_coop) -- and the records read back: (instance, primitive)
 * into ip and, when asked for, (t, u, v) into tuv.  `what` names the caller
 * in an error. */
int traceClosestRays(surf_ctx* c, uint32_t n, const float* o, const float* d, bool perWave, std::vector<float4>* tuv,
                     std::vector<uint2>& ip, const char* what) {
    std::vector<void*> tmp;
    float *dO, *dD; float4* dT; uint2* dI;
    int rc;
    if ((rc = devAlloc(c, tmp, &dO, 3 * (size_t)n)) || (rc = devAlloc(c, tmp, &dD, 3 * (size_t)n)) ||
        (rc = devAlloc(c, tmp, &dT, n)) || (rc = devAlloc(c, tmp, &dI, n))) { freeList(tmp); return rc; }
    (void)hipMemcpyAsync(dO, o, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dD, d, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    const Variant v = variantOf(c);
    if (perWave) {
        const auto k = traceClosestCoopKernel(c, v);
        hipLaunchKernelGGL(k.fn, dim3(n), dim3(64), k.lds, c->stream, c->S, (const float*)dO, (const float*)dD, n, dT, dI,
                           recStackWords(c));
    } else {
        const auto k = traceClosestKernel(c, v);
        hipLaunchKernelGGL(k.fn, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), k.lds, c->stream, c->S, (const float*)dO,
                           (const float*)dD, n, dT, dI, stackWords(c, kBlock));
    }
    ip.resize(n);
    if (tuv) {
        tuv->resize(n);
        (void)hipMemcpyAsync(tuv->data(), dT, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    }
    (void)hipMemcpyAsync(ip.data(), dI, sizeof(uint2) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    freeList(tmp);
    if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return SURF_OK;
}

/* Pixel classes of the issue order (cached until the camera, the scene or
 * the instances change): class A = the local pixels whose centre camera ray
 * first hits one of the heavy instances (setKeys).  Long Russian-roulette
 * paths start there (C3 frame 2: 67 % of the paths longer than 100 segments
 * from 4.3 % of the pixels, the two Suzannes); issuing those samples first
 * gives their paths more wavefront phases before the drain takes the
 * survivors.  Only the issue order changes: each sample is the same function
 * of (pixel, frame) and frames are still accumulated in order. */
int classifyPixels(surf_ctx* c) {
    if (c->permValid) return SURF_OK;
    const uint32_t n = c->npx;
    std::vector<float> o(3 * (size_t)n), d(3 * (size_t)n);
    const DevCamera& k = c->cam;
    for (uint32_t lp = 0; lp < n; ++lp) {
        const uint32_t x = lp % c->width, row = c->rows[lp / c->width];
        const float u = (float)x * k.invW, v = (float)row * k.invH;
        float dir[3], len2 = 0.0f;
        for (int a = 0; a < 3; ++a) {
            dir[a] = k.firstPixel[a] + u * k.uVec[a] + v * k.vVec[a] - k.pos[a];
            len2 += dir[a] * dir[a];
        }
        const float inv = 1.0f / std::sqrt(len2);
        for (int a = 0; a < 3; ++a) { o[3 * (size_t)lp + a] = k.pos[a]; d[3 * (size_t)lp + a] = dir[a] * inv; }
    }
    std::vector<uint2> ip;
    if (int rc = traceClosestRays(c, n, o.data(), d.data(), false, nullptr, ip, "pixel classification")) return rc;
    std::vector<uint32_t> perm;
    perm.reserve(n);
    for (int cls = 0; cls < 2; ++cls)
        for (uint32_t lp = 0; lp < n; ++lp) {
            const bool heavy = std::find(c->heavyInst.begin(), c->heavyInst.end(), ip[lp].x) != c->heavyInst.end();
            if (heavy == (cls == 0)) perm.push_back(lp);
        }
    c->permA = (uint32_t)std::count_if(ip.begin(), ip.end(), [&](const uint2& h) {
        return std::find(c->heavyInst.begin(), c->heavyInst.end(), h.x) != c->heavyInst.end();
    });
    SURF_CHECK(c, hipMemcpy(c->dPerm, perm.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
    c->permValid = true;
    return SURF_OK;
}

/* The driver of the per-pixel plane passes (device/plane_kernels.h): the
 * preconditions, the cached return, the planes' allocation, one timed launch
 * on the render stream and the marking valid.  A pass supplies `same` -- its
 * cached key equals the request's -- and `launch`, its hipLaunchKernelGGL
 * line; it validates its parameters before it calls this, and keeps its key
 * once this returns SURF_OK.  The launch goes behind whatever replays are in
 * flight: the kernels read the scene, the camera and source planes only, so
 * the sample stream is neither drained nor touched. */
template <class Same, class Launch>
int ensurePlanes(surf_ctx* c, PassPlanes& pp, const char* what, Same same, Launch launch) {
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (!c->hasCamera) return fail(c, SURF_ERR_NO_SCENE, "no camera set");
    SURF_CHECK(c, hipSetDevice(c->device));
    if (pp.valid && same()) return SURF_OK;
    pp.valid = false;
    for (int k = 0; k < pp.count; ++k)
        if (void*& p = pp.p[k]; !p && (hipMalloc(&p, (size_t)c->npx * 16) != hipSuccess || !p)) {
            p = nullptr;
            (void)hipGetLastError();
            return fail(c, SURF_ERR_OOM, std::string("hipMalloc of ") + what + " (" + std::to_string((size_t)c->npx * 16) + " bytes) failed");
        }
    SURF_CHECK(c, hipEventRecord(c->ev0, c->stream));
    launch();
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, hipEventRecord(c->ev1, c->stream));
    SURF_CHECK(c, hipEventSynchronize(c->ev1));
    (void)hipEventElapsedTime(&pp.ms, c->ev0, c->ev1);
    pp.valid = true;
    return SURF_OK;
}

/* plane k of a pass as the kernels take it */
template <class T>
T* planeOf(const PassPlanes& pp, int k) { return static_cast<T*>(pp.p[k]); }

/* The four feature planes (k_aov), computed on first use and kept until the
 * camera, the scene or the instances change. */
int ensureAov(surf_ctx* c) {
    PassPlanes& pp = c->aov;
    return ensurePlanes(c, pp, "a feature plane", [] { return true; }, [&] {
        const auto aov = aovKernel(c, variantOf(c));
        hipLaunchKernelGGL(aov.fn, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), aov.lds, c->stream, c->S, c->cam, (const uint32_t*)c->dRows, c->width, c->npx,
                           planeOf<float4>(pp, SURF_AOV_POSITION), planeOf<float4>(pp, SURF_AOV_NORMAL), planeOf<float4>(pp, SURF_AOV_ALBEDO),
                           planeOf<uint4>(pp, SURF_AOV_ID), stackWords(c, kBlock));
    });
}

/* The same planes traced through mirrors and glass (k_aov_chain), in device
 * planes of their own: kept until what drops the first-hit planes, or a read
 * with another max_links. */
int ensureAovChain(surf_ctx* c, uint32_t maxLinks) {
    if (maxLinks > SURF_AOV_CHAIN_MAX_LINKS)
        return fail(c, SURF_ERR_INVALID, "max_links is above SURF_AOV_CHAIN_MAX_LINKS (" + std::to_string(SURF_AOV_CHAIN_MAX_LINKS) + ")");
    PassPlanes& pp = c->aovChain;
    const int rc = ensurePlanes(c, pp, "a feature plane", [&] { return c->aovChainLinks == maxLinks; }, [&] {
        const auto aov = aovChainKernel(c, variantOf(c));
        hipLaunchKernelGGL(aov.fn, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), aov.lds, c->stream, c->S, c->cam, (const uint32_t*)c->dRows, c->width, c->npx,
                           planeOf<float4>(pp, SURF_AOV_POSITION), planeOf<float4>(pp, SURF_AOV_NORMAL), planeOf<float4>(pp, SURF_AOV_ALBEDO),
                           planeOf<uint4>(pp, SURF_AOV_ID), stackWords(c, kBlock), maxLinks);
    });
    if (rc == SURF_OK) c->aovChainLinks = maxLinks;
    return rc;
}

/* surf_aov_sampled_params as the header states them */
bool aovSampledParamsOk(const surf_aov_sampled_params* p) {
    return p && p->samples >= 1u && p->samples <= SURF_AOVS_MAX_SAMPLES && (p->key == SURF_MATTE_INSTANCE || p->key == SURF_MATTE_MATERIAL) &&
           p->reserved == 0u;
}

/* The six sampled planes (k_aov_sampled), in device planes of their own: kept
 * until what drops the first-hit planes, or a read with other params. */
int ensureAovSampled(surf_ctx* c, const surf_aov_sampled_params& q) {
    if (!aovSampledParamsOk(&q)) return fail(c, SURF_ERR_INVALID, "sampled feature buffers: samples outside 1.." + std::to_string(SURF_AOVS_MAX_SAMPLES) + ", an unknown key or reserved != 0");
    PassPlanes& pp = c->aovSampled;
    const int rc = ensurePlanes(c, pp, "a feature plane", [&] { return std::memcmp(&c->aovSampledParams, &q, sizeof q) == 0; }, [&] {
        const auto aov = aovSampledKernel(c, variantOf(c));
        hipLaunchKernelGGL(aov.fn, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), aov.lds, c->stream, c->S, c->cam, (const uint32_t*)c->dRows, c->width, c->npx, q.samples, q.first_sample, q.key,
                           planeOf<float4>(pp, SURF_AOVS_POSITION), planeOf<float4>(pp, SURF_AOVS_NORMAL), planeOf<float4>(pp, SURF_AOVS_ALBEDO),
                           planeOf<uint4>(pp, SURF_AOVS_ID), planeOf<uint4>(pp, SURF_AOVS_MATTE_KEY), planeOf<uint4>(pp, SURF_AOVS_MATTE_COUNT),
                           stackWords(c, kBlock));
    });
    if (rc == SURF_OK) c->aovSampledParams = q;
    return rc;
}

/* surf_ao_params as the header states them */
bool aoParamsOk(const surf_ao_params* p) {
    const auto ranged = [](float v, bool zeroOk) { return !std::isnan(v) && (v > 0.0f || (zeroOk && v == 0.0f)); };
    return p && p->samples >= 1u && p->samples <= SURF_AO_MAX_SAMPLES && (p->samples & (p->samples - 1u)) == 0u && ranged(p->radius, false) &&
           ranged(p->bias, true) && (p->source == SURF_AO_FIRST_HIT || p->source == SURF_AO_CHAIN) &&
           (p->source == SURF_AO_FIRST_HIT || p->max_links <= SURF_AOV_CHAIN_MAX_LINKS) && p->reserved[0] == 0u && p->reserved[1] == 0u;
}

/* The two occlusion planes (k_ao), in device planes of their own: kept until
 * what drops the first-hit planes, or a read with other params.  The source
 * planes first, as a read of them would compute them. */
int ensureAo(surf_ctx* c, const surf_ao_params& q) {
    if (!aoParamsOk(&q))
        return fail(c, SURF_ERR_INVALID, "ambient occlusion: samples not a power of two in 1.." + std::to_string(SURF_AO_MAX_SAMPLES) +
                                             ", radius not > 0, bias not >= 0, an unknown source, max_links above SURF_AOV_CHAIN_MAX_LINKS or reserved != 0");
    const bool chain = q.source == SURF_AO_CHAIN;
    if (int rc = chain ? ensureAovChain(c, q.max_links) : ensureAov(c)) return rc;
    const PassPlanes& src = chain ? c->aovChain : c->aov;
    PassPlanes& pp = c->ao;
    const int rc = ensurePlanes(c, pp, "an occlusion plane", [&] { return std::memcmp(&c->aoParams, &q, sizeof q) == 0; }, [&] {
        /* pixels per block: one per lane, or one per group of `samples` lanes */
        const uint32_t perBlock = c->aoRayMap ? (uint32_t)kBlock / q.samples : (uint32_t)kBlock;
        const auto ao = aoKernel(c, variantOf(c));
        hipLaunchKernelGGL(ao.fn, dim3((c->npx + perBlock - 1) / perBlock), dim3(kBlock), ao.lds, c->stream, c->S, (const uint32_t*)c->dRows, c->width, c->npx, q.samples, q.first_sample, q.radius, q.bias,
                           planeOf<const float4>(src, SURF_AOV_POSITION), planeOf<const float4>(src, SURF_AOV_NORMAL), planeOf<const float4>(src, SURF_AOV_ALBEDO),
                           planeOf<float4>(pp, SURF_AO_OPENNESS), planeOf<uint4>(pp, SURF_AO_BITS), stackWords(c, kBlock));
    });
    if (rc == SURF_OK) c->aoParams = q;
    return rc;
}

/* The body of the eight surf_read_* / surf_copy_*_device entry points of the
 * plane passes: `ensure` computes the pass's planes (and reports through the
 * context), then one copy of plane `plane` on the render stream. */
template <class Ensure>
int copyPlane(surf_ctx* c, bool argsOk, const PassPlanes surf_ctx::*pass, int plane, void* dst, hipMemcpyKind kind, Ensure ensure) {
    if (!c || !argsOk || !dst || plane < 0 || plane >= (c->*pass).count) return SURF_ERR_INVALID;
    if (int rc = ensure()) return rc;
    SURF_CHECK(c, hipMemcpyAsync(dst, (c->*pass).p[plane], (size_t)c->npx * 16, kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* ... and of their four surf_debug_*_time */
int passTime(const surf_ctx* c, const PassPlanes surf_ctx::*pass, float* kernel_ms) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    *kernel_ms = (c->*pass).ms;
    return SURF_OK;
}

/* ---- sample stream ------------------------------------------------------ */
int startStream(surf_ctx* c, uint64_t baseFrame, uint32_t maxSeg, uint32_t frames, uint32_t spp) {
    Counters h{};
    for (uint32_t& v : h.capped) v = kUnset;
    /* a multi-frame request that fits the window: its pixels in class order */
    c->permFrames = 0;
    c->streamMasked = c->pmOn;
    c->streamPx = c->pmOn ? c->pmActive : c->npx;
    h.nActive = c->pmOn ? c->pmActive : 0u;
    if (!c->pmOn && !c->ssOn && c->reorder && frames >= 2 && (uint64_t)frames * spp <= c->window && c->heavyInst.size()) {
        int rc = classifyPixels(c);
        if (rc) return rc;
        if (c->permA > 0 && c->permA < c->npx) c->permFrames = frames;
    }
    h.permFrames = c->permFrames;
    h.permA = c->permFrames ? c->permA : 0u;
    h.maxSeg = maxSeg;
    /* automatic: on for 1-sample frames (radiance-neutral); off for
     * multi-sample frames, whose next sample starts from the RNG state the
     * reference's path ends with -- which an early end would change */
    h.zeroCutoff = (c->zeroCutoff < 0 ? spp == 1 : c->zeroCutoff != 0) ? 1u : 0u;
    h.spp = spp;
    h.baseFrame = baseFrame;
    h.survCap = c->survCap;
    /* The fused count (k_regen_count) relies on this: binHist is valid only
     * for the pool the previous phase's k_regen_count produced, and the first
     * phase's sort does not recount it.  So every pool change outside the
     * graph zeroes nIn -- here both pools start empty (h is zeroed), so the
     * stale counts order no path. */
    *c->hctr = h;
    SURF_CHECK(c, hipMemcpyAsync(c->ctr, c->hctr, sizeof(Counters), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemsetAsync(c->frameDone, 0, (size_t)kStripes * c->window * sizeof(uint32_t), c->stream));
    SURF_CHECK(c, hipMemsetAsync(c->Q.cur, 0, (size_t)2 * kShSegs * kShStride * sizeof(uint32_t), c->stream));
    c->streamActive = true;
    c->baseFrame = baseFrame;
    c->targetFrames = 0;
    c->accPasses = 0;
    c->spp = spp;
    c->streamMaxSeg = maxSeg;
    c->pushedLimit = 0;
    c->issuePerPhase = 0;          /* predicted from this stream's own replays only */
    return SURF_OK;
}

/* Chains (first samples of (frame, pixel)) that may be issued: a frame is
 * issued only when all its passes fit the window past the accumulated ones. */
uint64_t issueLimit(const surf_ctx* c) {
    return std::min<uint64_t>(c->targetFrames, (c->accPasses + c->window) / c->spp) * (uint64_t)c->streamPx;
}
uint64_t targetPasses(const surf_ctx* c) { return c->targetFrames * c->spp; }

int pushLimit(surf_ctx* c) {
    const uint64_t lim = issueLimit(c);
    if (lim == c->pushedLimit) return SURF_OK;
    uint64_t* src = &c->hLimit[c->hLimitNext++ % surf_ctx::kLimitRing];
    *src = lim;
    SURF_CHECK(c, hipMemcpyAsync(&c->ctr->limit, src, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    c->pushedLimit = lim;
    return SURF_OK;
}

/* Frames whose every chain is issued after `iss` chains (k_regen's order:
 * the permuted head of permFrames frames, then frame-major). */
uint64_t fullyIssuedFrames(const surf_ctx* c, uint64_t iss) {
    const uint64_t P = c->permFrames;
    if (!P || iss >= (uint64_t)c->npx * P) return iss / c->streamPx;      /* (masked streams have no permuted head) */
    const uint64_t endA = (uint64_t)c->permA * P;
    return iss <= endA ? 0 : (iss - endA) / (c->npx - c->permA);
}

/* Finished paths of a frame slot in a snapshot: sum over the completion stripes. */
uint64_t framePaths(const surf_ctx* c, const uint32_t* fd, uint32_t slot) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < kStripes; ++k) n += fd[(size_t)k * c->window + slot];
    return n;
}

/* Event totals of the current stream: plain counters + the block stripes. */
void streamEvents(const Counters& h, unsigned long long out[kEvents]) {
    for (int k = 0; k < kEvents; ++k) {
        out[k] = h.ev[k];
        for (uint32_t s = 0; s < kStripes; ++s) out[k] += h.evS[s][k];
    }
}

/* Queues a snapshot of the counters and of the open passes' completion
 * stripes ([accPasses, targetPasses), at most a window: a strided copy of
 * their slots in each stripe row), taken after `replays` graph replays. */
int enqueueSnap(surf_ctx* c, int phases) {
    surf_ctx::Snap& sn = c->snap[(c->snapHead + c->snapCount) % surf_ctx::kSnaps];
    SURF_CHECK(c, hipMemcpyAsync(sn.h, c->ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    const uint64_t tp = targetPasses(c);
    const uint64_t open = std::min<uint64_t>(tp - std::min(c->accPasses, tp), c->window);
    const uint32_t s0 = (uint32_t)(c->accPasses % c->window);
    const uint32_t n0 = (uint32_t)std::min<uint64_t>(open, c->window - s0);
    const size_t pitch = (size_t)c->window * sizeof(uint32_t);
    if (n0)
        SURF_CHECK(c, hipMemcpy2DAsync(sn.fd + s0, pitch, c->frameDone + s0, pitch, n0 * sizeof(uint32_t), kStripes,
                                       hipMemcpyDeviceToHost, c->stream));
    if (open > n0)
        SURF_CHECK(c, hipMemcpy2DAsync(sn.fd, pitch, c->frameDone, pitch, (open - n0) * sizeof(uint32_t), kStripes,
                                       hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipEventRecord(sn.ev, c->stream));
    sn.acc = c->accPasses;
    sn.open = open;
    sn.phases = phases;
    ++c->snapCount;
    return SURF_OK;
}

/* Waits for the oldest snapshot, makes it the host's view of the counters and
 * accumulates, in pass order, every leading pass whose samples have all
 * finished in it.  A pass is complete when all its samples were issued and
 * all finished; a slot is reused only after its pass is accumulated, so passes
 * of frames not yet fully issued must not be tested (their slot may still
 * count an older pass), nor passes past the snapshot's copied range.  Later
 * replays already queued cannot touch the slots accumulated here: the issue
 * limit they run under was pushed before this accumulation. */
int consumeSnap(surf_ctx* c) {
    surf_ctx::Snap& sn = c->snap[c->snapHead];
    SURF_CHECK(c, hipEventSynchronize(sn.ev));
    const uint64_t before = c->hctr->issued[0];
    std::memcpy(c->hctr, sn.h, sizeof(Counters));
    /* per phase (a replay is kPhasesPerGraph or kPhasesShort phases), and only from a replay
     * that issued under its limit the whole time: a starved one undercounts */
    if (sn.phases > 0 && c->hctr->issued[0] > before && c->hctr->issued[0] < c->hctr->limit)
        c->issuePerPhase = (c->hctr->issued[0] - before) / (uint64_t)sn.phases;
    c->snapHead = (c->snapHead + 1) % surf_ctx::kSnaps;
    --c->snapCount;
    for (int k = 0; k < 2; ++k)                       /* calls whose end this snapshot has passed */
        if (c->tevPending[k] && hipEventQuery(c->tev[k][1]) == hipSuccess) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->tev[k][0], c->tev[k][1]);
            c->stats.ms_total += ms;
            c->tevPending[k] = false;
        }
    const uint64_t tp = targetPasses(c);
    const uint64_t issuedPasses = fullyIssuedFrames(c, c->hctr->issued[0]) * c->spp;
    const uint64_t hi = sn.acc + sn.open;
    uint64_t f = c->accPasses;
    while (f < tp && f < issuedPasses && f < hi && framePaths(c, sn.fd, (uint32_t)(f % c->window)) == c->streamPx) ++f;
    if (f == c->accPasses) return SURF_OK;
    const uint32_t count = (uint32_t)(f - c->accPasses);
    const uint32_t threads = std::max<uint32_t>(c->streamPx, count * kStripes);
    if (c->profiling) {                                /* events of its own: ev0 / ev1 bracket the drain this launch runs inside */
        for (auto& e : c->accEv)
            if (!e) SURF_CHECK(c, hipEventCreate(&e));
        SURF_CHECK(c, hipEventRecord(c->accEv[0], c->stream));
    }
    if (c->bkM && c->streamMasked)
        hipLaunchKernelGGL(accumulateBucketsListKernel(c), dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->rad,
                           c->acc, c->npx, (unsigned long long)c->accPasses, count, c->window, c->frameDone, c->sqOn ? c->sq : nullptr,
                           c->bk, (const uint32_t*)c->pmList, c->pmActive);
    else if (c->bkM)
        hipLaunchKernelGGL(accumulateBucketsKernel(c), dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->rad,
                           c->acc, c->npx, (unsigned long long)c->accPasses, count, c->window, c->frameDone, c->sqOn ? c->sq : nullptr,
                           c->bk);
    else if (c->streamMasked)
        hipLaunchKernelGGL(accumulateListKernel(c), dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->rad,
                           c->acc, c->npx, (unsigned long long)c->accPasses, count, c->window, c->frameDone, c->sqOn ? c->sq : nullptr,
                           (const uint32_t*)c->pmList, c->pmActive);
    else
        hipLaunchKernelGGL(accumulateKernel(c), dim3((threads + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->rad,
                           c->acc, c->npx, (unsigned long long)c->accPasses, count, c->window, c->frameDone, c->sqOn ? c->sq : nullptr);
    SURF_CHECK(c, hipGetLastError());
    if (c->profiling) {                                /* surf_stats.ms_accum; profiling waits for every launch anyway */
        SURF_CHECK(c, hipEventRecord(c->accEv[1], c->stream));
        SURF_CHECK(c, hipEventSynchronize(c->accEv[1]));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->accEv[0], c->accEv[1]);
        c->stats.ms_accum += ms;
    }
    c->accPasses = f;
    return pushLimit(c);
}

int consumeAll(surf_ctx* c) {
    int rc;
    while (c->snapCount)
        if ((rc = consumeSnap(c))) return rc;
    return SURF_OK;
}

/* Reads counters + per-pass completion (one sync) and accumulates. */
int syncAndAccumulate(surf_ctx* c, int phases = 0) {
    int rc;
    if ((rc = consumeAll(c)) || (rc = enqueueSnap(c, phases))) return rc;
    return consumeSnap(c);
}

/* One unit of forward progress: kPhasesPerGraph phases (graph replay, or
 * direct launches with per-kernel events when profiling). */
int advance(surf_ctx* c, bool shortRun = false) {
    const int phases = shortRun ? kPhasesShort : kPhasesPerGraph;
    if (c->profiling) {
        for (int ph = 0; ph < phases; ++ph) launchPhase(c, ph, &c->pev[kPhaseEvents * ph]);
        SURF_CHECK(c, hipEventRecord(c->pev[kPhaseEvents * phases], c->stream));
        SURF_CHECK(c, hipGetLastError());
        SURF_CHECK(c, hipEventSynchronize(c->pev[kPhaseEvents * phases]));
        for (int ph = 0; ph < phases; ++ph) {
            float t[kPhaseEvents];
            for (int k = 0; k < kPhaseEvents; ++k)
                (void)hipEventElapsedTime(&t[k], c->pev[kPhaseEvents * ph + k], c->pev[kPhaseEvents * ph + k + 1]);
            /* (t[3]: k_regen when it runs before the fork, else nothing) */
            c->stats.ms_sort += t[0];
            c->stats.ms_extend += t[1]; c->stats.ms_shade += t[2]; c->stats.ms_connect += t[4]; c->stats.ms_regen += t[3] + t[5];
            c->stats.launches_extend++;
            if (c->phaseLog)
                std::fprintf(c->phaseLog, "phase %u sort %.4f extend %.4f shade %.4f regen %.4f connect %.4f\n", c->hPhaseN[ph], t[0], t[1],
                             t[2], t[3] + t[5], t[4]);
        }
        if (c->phaseLog) std::fflush(c->phaseLog);
    } else {
        if (c->streamMasked)
            SURF_CHECK(c, hipGraphLaunch(shortRun ? c->graphExecShortM : c->graphExecM, c->stream));
        else
            SURF_CHECK(c, hipGraphLaunch(shortRun ? c->graphExecShort : c->graphExec, c->stream));
    }
    c->stats.iterations += phases;
    if (c->stats.iterations > kMaxIterations)
        return fail(c, SURF_ERR_LIMIT, "wavefront did not drain after " + std::to_string(c->stats.iterations) + " iterations");
    return SURF_OK;
}

/* Finishes every path of pool 0 in one k_tail launch (counters at an even
 * phase boundary: pool 0 is the next to be extended, nothing else pending). */
void launchTail(surf_ctx* c, Pool in, uint32_t n, uint32_t lpw, uint32_t firstCounted, uint32_t budget, Pool out) {
    const uint32_t blocks = (n + lpw - 1) / lpw;
    withSensor(c, [&](auto sf) {
        constexpr bool SF = decltype(sf)::value;
        const auto tail = tailKernel<SF>(c, variantOf(c));
        hipLaunchKernelGGL(tail.fn, dim3(blocks), dim3(64), tail.lds, c->stream, c->S, in, n, lpw, c->rad, c->frameDone,
                           c->npx, c->window, c->ctr, stackWords(c, 64), firstCounted, budget, out, c->cam, geomArg<SF>(c));
    });
}

/* Finishes every path of pool 0 (counters at an even phase boundary: pool 0 is
 * the next to be extended, nothing else pending).  Lane-parallel stages (many
 * paths per wave) run each path for up to tailBudget segments and hand the
 * paths still alive to the next stage; once few enough remain (they are the
 * reference's Russian-roulette survivors that run for thousands of segments),
 * the cooperative tail runs each on a whole wave, which cuts the latency of a
 * segment -- the quantity the last paths of a drain are bound by. */
/* The cooperative drain uses the lanes-as-planes wave traversal (traceWave):
 * single-leaf TLAS of <= 64 instances, stack of node records in 64 lanes. */
/* Any TLAS (traceWaveTlas walks one whose root splits or that holds > 64
 * instances); the TLAS stack is one VGPR (<= 64 entries). */
bool waveEligible(const surf_ctx* c) { return c->hasScene && c->stackDepth <= 64 && coopLdsOk(c); }

/* Regen counted each pool-0 path's next extension ray (firstCounted). */
int runTail(surf_ctx* c) {
    const uint32_t n = c->hctr->nIn[0];
    if (n == 0) return SURF_OK;
    if (c->profiling) SURF_CHECK(c, hipEventRecord(c->pev[0], c->stream));
    Pool in = c->pool[0];
    const Variant v = variantOf(c);
    uint32_t cnt = n, firstCounted = 1u;
    c->tailFirstRays += n;
    int buf = 0;
    static const bool dbg = std::getenv("SURF_DEBUG_TAIL") != nullptr;   /* diagnostics: per-stage log on stderr */
    auto t0 = std::chrono::steady_clock::now();
    for (int stage = 0; cnt; ++stage) {
        if (dbg) {
            SURF_CHECK(c, hipStreamSynchronize(c->stream));
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            std::fprintf(stderr, "[surf tail] stage %d: %u paths at %.2f ms\n", stage, cnt, ms);
        }
        if (c->tailPair && waveEligible(c) && cnt <= c->coopAll) {
            /* as many two-wave workgroups as are resident at once, each wave
             * taking paths from the queue; idle waves trace their sibling's
             * shadow rays once the queue is empty */
            SURF_CHECK(c, hipMemsetAsync(&c->ctr->rowNext, 0, sizeof(uint32_t), c->stream));
            withSensor(c, [&](auto sf) {
                constexpr bool SF = decltype(sf)::value;
                int per = 0;
                const auto pair = tailPairKernel<SF>(c, v);
                if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, pair.fn, 128, pair.lds) != hipSuccess || per < 1)
                    per = 2 * SURF_COOP_WAVES;
                const uint32_t blocks = std::max<uint32_t>(1u, std::min<uint32_t>((cnt + 1u) / 2u, c->cus * (uint32_t)per));
                hipLaunchKernelGGL(pair.fn, dim3(blocks), dim3(128), pair.lds, c->stream, c->S, in, cnt, c->rad, c->frameDone,
                                   c->npx, c->window, c->ctr, recStackWords(c), firstCounted, c->cam, geomArg<SF>(c));
            });
            SURF_CHECK(c, hipGetLastError());
            c->stats.tail_survivors += cnt;
            break;
        }
        if (waveEligible(c) && cnt <= c->coopAll) {
            withSensor(c, [&](auto sf) {
                constexpr bool SF = decltype(sf)::value;
                const auto coop = tailCoopKernel<SF>(c, v);
                hipLaunchKernelGGL(coop.fn, dim3(cnt), dim3(64), coop.lds, c->stream, c->S, in, cnt, c->rad, c->frameDone,
                                   c->npx, c->window, c->ctr, recStackWords(c), firstCounted, c->cam, geomArg<SF>(c));
            });
            SURF_CHECK(c, hipGetLastError());
            c->stats.tail_survivors += cnt;
            break;
        }
        /* no more waves than fit at once (2 per SIMD at the tail's register
         * count): a second round would wait for the first round's longest path */
        const uint32_t lpw = c->tailLanes ? std::min<uint32_t>(64u, c->tailLanes)
                                          : std::min<uint32_t>(64u, std::max<uint32_t>(1u, (cnt + c->coopMax - 1) / c->coopMax));
        c->hctr->survN = 0;
        SURF_CHECK(c, hipMemcpyAsync(&c->ctr->survN, &c->hctr->survN, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        launchTail(c, in, cnt, lpw, firstCounted, c->tailBudget, c->surv[buf]);
        SURF_CHECK(c, hipGetLastError());
        if (!c->tailBudget) break;
        SURF_CHECK(c, hipMemcpyAsync(&c->hctr->survN, &c->ctr->survN, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
        in = c->surv[buf];
        cnt = std::min(c->hctr->survN, c->survCap);
        firstCounted = 0u;
        buf ^= 1;
    }
    if (c->profiling) {
        SURF_CHECK(c, hipEventRecord(c->pev[1], c->stream));
        SURF_CHECK(c, hipEventSynchronize(c->pev[1]));
        float t; (void)hipEventElapsedTime(&t, c->pev[0], c->pev[1]);
        c->stats.ms_tail += t;
    }
#if SURF_DRAIN_TRACE
    if (const char* path = std::getenv("SURF_DRAIN_TRACE_FILE")) {
        /* diagnostics: one line per path the cooperative drain finished */
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
        uint32_t nrec = 0;
        SURF_CHECK(c, hipMemcpyFromSymbol(&nrec, HIP_SYMBOL(g_drainEndN), sizeof nrec));
        nrec = std::min(nrec, kDrainTraceCap);
        std::vector<uint4> rec(nrec);
        if (nrec) SURF_CHECK(c, hipMemcpyFromSymbol(rec.data(), HIP_SYMBOL(g_drainEnd), nrec * sizeof(uint4)));
        int khz = 0;
        (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device);
        if (FILE* f = std::fopen(path, "a")) {
            std::fprintf(f, "# drain %u paths, clock %d kHz: end_lo state segments start_lo\n", n, khz);
            for (const uint4& r : rec) std::fprintf(f, "%u %u %u %u\n", r.x, r.y, r.z, r.w);
            std::fclose(f);
        }
        const uint32_t zero = 0;
        SURF_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_drainEndN), &zero, sizeof zero));
    }
#endif
#if SURF_SEG_TIMING
    if (dbg) {
        SURF_CHECK(c, hipMemcpyAsync(c->hctr, c->ctr, sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
        const unsigned long long* g = c->hctr->dbg;
        const double ns = (double)std::max(1ull, g[3]);
        std::fprintf(stderr, "[surf tail] coop cycles per segment: extend %.0f shade %.0f connect %.0f (%llu segments, %llu shadow)\n",
                     g[0] / ns, g[1] / ns, g[2] / ns, g[3], g[4]);
        unsigned long long h[8];
        SURF_CHECK(c, hipMemcpyFromSymbol(h, HIP_SYMBOL(g_segStats), sizeof(h)));
        std::fprintf(stderr, "[surf tail] extend per segment: instance prologues %.0f cycles, BLAS loops %.0f cycles, %.1f interior visits, "
                     "%.1f leaves, %.1f triangles, %.2f instances entered; %.0f cycles waiting for prefetched records, %.0f in leaves\n",
                     h[0] / ns, h[1] / ns, h[2] / ns, h[3] / ns, h[4] / ns, h[5] / ns, h[6] / ns, h[7] / ns);
        const unsigned long long zero[8] = {};
        SURF_CHECK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_segStats), zero, sizeof(zero)));   /* per drain, like the counters */
    }
#endif
    /* pool 0 is now empty: the next phase starts from regen's refill.  The
     * fused count relies on this too: binHist still holds k_regen_count's
     * counts of the pool the tail just finished, valid for no other pool, and
     * the next replay's first sort does not recount -- with nIn zeroed it
     * orders no path, and that phase's k_regen_count counts the refill. */
    c->hctr->nIn[0] = 0;
    SURF_CHECK(c, hipMemcpyAsync(&c->ctr->nIn[0], &c->hctr->nIn[0], sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* Drain hand-over (automatic): a quarter frame of paths (W * H / 4, what
 * capacity / 16 was at the round-2 pool of 4 frames), at most capacity / 16:
 * tied to the pool, a larger pool handed C5's deep-BVH drain 280 k paths
 * (drain 2.2 -> 5.8 s per render). */
uint32_t tailThreshold(const surf_ctx* c) {
    if (c->tailPaths) return c->tailPaths;
    const uint64_t quarter = (uint64_t)c->width * c->height / 4;
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(quarter, c->capacity / 16), 4096u);
}

/* Runs until every requested sample is issued (drain = false) or until every
 * requested frame is accumulated (drain = true).  While issuing, a call runs
 * pipelined: it queues the next replay before it has read the previous one's
 * counters -- predicting what the replays in flight issue -- and may return
 * with up to kSnaps replays in flight, so the GPU does not wait for the host
 * between polls or calls (the drop-in loop's one-frame calls).  Drains, the
 * tail and a starved stream decide from fresh counters. */
int pump(surf_ctx* c, bool drain, uint64_t lag) {
    int rc;
    const bool pipe = c->pipeline && !drain;
    if (!pipe && (rc = consumeAll(c))) return rc;
    if ((rc = pushLimit(c))) return rc;
    const uint64_t target = c->targetFrames * (uint64_t)c->streamPx;
    for (;;) {
        if (pipe)       /* the snapshots that have landed, and the oldest when both are in flight */
            while (c->snapCount && (c->snapCount == surf_ctx::kSnaps || hipEventQuery(c->snap[c->snapHead].ev) == hipSuccess))
                if ((rc = consumeSnap(c))) return rc;
        const uint64_t issued = c->hctr->issued[0];
        /* what the replays in flight issue: predicted per phase, never past the pushed limit */
        uint64_t inflightPhases = 0;
        for (int k = 0; k < c->snapCount; ++k) inflightPhases += (uint64_t)c->snap[(c->snapHead + k) % surf_ctx::kSnaps].phases;
        const uint64_t ahead = std::min<uint64_t>(inflightPhases * c->issuePerPhase, c->pushedLimit - std::min(issued, c->pushedLimit));
        /* in flight at a replay boundary: the pool the next phase extends */
        const uint32_t inflight = c->hctr->nIn[0];
        if (!drain && issued + ahead + lag >= target) return SURF_OK;
        if (drain && c->accPasses >= targetPasses(c)) return SURF_OK;
        const bool starved = issued >= c->pushedLimit;     /* nothing more may be issued right now */
        if (c->snapCount && starved) {                     /* decided from fresh counters */
            if ((rc = consumeAll(c))) return rc;
            continue;
        }
        const uint64_t accBefore = c->accPasses;
        static const bool dbgDrain = std::getenv("SURF_DEBUG_DRAIN") != nullptr;   /* diagnostics: drain timeline */
        if (dbgDrain && starved) {
            static auto tS = std::chrono::steady_clock::now();
            std::fprintf(stderr, "[surf drain] iteration %llu: %u paths in flight, %llu/%llu passes at %.3f ms\n",
                         (unsigned long long)c->stats.iterations, inflight, (unsigned long long)c->accPasses,
                         (unsigned long long)targetPasses(c),
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tS).count());
        }
        int phases = 0;
        if (starved && inflight > 0 && inflight <= tailThreshold(c)) {
            if ((rc = runTail(c))) return rc;
        } else if (starved && inflight == 0) {
            /* every issued sample finished: accumulating re-opens the window */
        } else {
            /* draining (nothing left to issue): several replays per host poll --
             * the per-replay poll, not the kernels, is what a small pool pays */
            const int reps = starved ? c->drainReplays : 1;
            /* a per-frame render call (lagged, or at most one frame left to
             * issue): short replays (SURF_DRAIN_SHORT=1: also once nothing is
             * left to issue, so the drain takes over within kPhasesShort phases instead
             * of up to kPhasesPerGraph (16) -- measured slower) */
            const bool shortRun = (!drain && (lag > 0 || target - issued <= c->streamPx)) || (starved && c->drainShort);
            for (int k = 0; k < reps; ++k)
                if ((rc = advance(c, shortRun))) return rc;
            phases = reps * (shortRun ? kPhasesShort : kPhasesPerGraph);
            if (pipe) {                                    /* read later: queue the next replay first */
                if ((rc = enqueueSnap(c, phases))) return rc;
                continue;
            }
        }
        if ((rc = syncAndAccumulate(c, phases))) return rc;
        if (starved && inflight == 0 && c->accPasses == accBefore)
            return fail(c, SURF_ERR_HIP, "sample stream stalled: pool empty but frames incomplete");
    }
}

/* Adds the device time of calls that returned with replays in flight (their
 * ends have passed once the stream is idle). */
void collectCallTimes(surf_ctx* c) {
    for (int k = 0; k < 2; ++k)
        if (c->tevPending[k]) {
            (void)hipEventSynchronize(c->tev[k][1]);
            float ms = 0;
            (void)hipEventElapsedTime(&ms, c->tev[k][0], c->tev[k][1]);
            c->stats.ms_total += ms;
            c->tevPending[k] = false;
        }
}

int ensureDrained(surf_ctx* c) {
    if (!c->streamActive) return SURF_OK;
    SURF_CHECK(c, hipSetDevice(c->device));
    {
        const int rc = consumeAll(c);                 /* the host's counters as of the last replay */
        if (rc) return rc;
        collectCallTimes(c);
    }
    if (c->accPasses >= targetPasses(c)) return SURF_OK;
    if (!c->profiling) {
        int rc = buildGraph(c);
        if (rc) return rc;
    }
    SURF_CHECK(c, hipEventRecord(c->ev0, c->stream));
    int rc = pump(c, true, 0);
    if (rc) return rc;
    SURF_CHECK(c, hipEventRecord(c->ev1, c->stream));
    SURF_CHECK(c, hipEventSynchronize(c->ev1));
    float ms = 0;
    (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
    c->stats.ms_total += ms;
    return SURF_OK;
}

}  // namespace

int surfhost::drainStream(surf_ctx* c) { return ensureDrained(c); }
int surfhost::featurePlanes(surf_ctx* c) { return ensureAov(c); }
int surfhost::guidePlanes(surf_ctx* c, void* const** planes) {
    if (c->guides == SURF_GUIDES_SAMPLED) {
        *planes = c->aovSampled.p;
        return ensureAovSampled(c, c->guideSampled);
    }
    const bool chain = c->guides == SURF_GUIDES_CHAIN;
    *planes = chain ? c->aovChain.p : c->aov.p;
    return chain ? ensureAovChain(c, c->guideLinks) : ensureAov(c);
}

/* A stream ends when its pool is empty and all its frames are accumulated. */
int surfhost::endStream(surf_ctx* c) {
    int rc = ensureDrained(c);
    if (rc) return rc;
    if (c->streamActive) {
        unsigned long long e[kEvents];
        streamEvents(*c->hctr, e);
        for (int k = 0; k < kEvents; ++k) c->evBase[k] += e[k];
        c->segMaxBase = std::max(c->segMaxBase, c->hctr->segMax);
    }
    c->streamActive = false;
    return SURF_OK;
}

namespace {

/* Which rows a shard owns. */
std::vector<uint32_t> shardRows(uint32_t height, uint32_t shard, uint32_t shards, uint32_t block) {
    std::vector<uint32_t> rows;
    if (block == 0) {
        const uint32_t r0 = (uint32_t)((uint64_t)height * shard / shards), r1 = (uint32_t)((uint64_t)height * (shard + 1) / shards);
        for (uint32_t r = r0; r < r1; ++r) rows.push_back(r);
    } else {
        for (uint32_t r = 0; r < height; ++r)
            if ((r / block) % shards == shard) rows.push_back(r);
    }
    return rows;
}

int createCtx(int dev, uint32_t w, uint32_t h, std::vector<uint32_t> rows, surf_ctx** out) {
    if (!out) return fail(nullptr, SURF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (w == 0 || h == 0 || rows.empty()) return fail(nullptr, SURF_ERR_INVALID, "empty frame or shard");
    if ((uint64_t)w * rows.size() > (1ull << 31)) return fail(nullptr, SURF_ERR_INVALID, "shard too large");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || dev < 0 || dev >= count) return fail(nullptr, SURF_ERR_NO_DEVICE, "no HIP device " + std::to_string(dev));
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(nullptr, SURF_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
        return fail(nullptr, SURF_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950");
    /* tuning knobs (A/B runs): read once per context, invalid values refused */
    uint32_t extBlock = 128;
    if (const char* e = std::getenv("SURF_EXTEND_BLOCK")) {
        const int b = std::atoi(e);
        if (b != 128 && b != 256) return fail(nullptr, SURF_ERR_INVALID, std::string("SURF_EXTEND_BLOCK must be 128 or 256, not ") + e);
        extBlock = (uint32_t)b;
    }
    auto* c = new surf_ctx();
    c->capEv.assign(2 * kPhasesPerGraph, nullptr);
    c->pev.assign(kPhasesPerGraph * kPhaseEvents + 1, nullptr);
    c->device = dev;
    c->extBlock = extBlock;
    if (const char* e = std::getenv("SURF_SORT")) {
        c->sortRays = e[0] != '0';
        c->sortPool = e[0] != '3';
        c->sortShadow = e[0] != '2';
    }
    if (const char* e = std::getenv("SURF_SH_KEY")) c->shKey = e[0] == '1' ? 1u : (e[0] == '2' ? 2u : 0u);
    if (const char* e = std::getenv("SURF_SH_REGION")) c->shRegion = (uint32_t)std::max(0, std::atoi(e));
    if (const char* e = std::getenv("SURF_CONNECT_GLOBAL")) c->connectGlobal = e[0] != '0';
    if (const char* e = std::getenv("SURF_EXT_STACK16")) c->extStack16 = e[0] != '0';
    if (const char* e = std::getenv("SURF_REGEN_COUNT")) c->regenCount = e[0] != '0';
    if (const char* e = std::getenv("SURF_KEY")) c->keyMode = e[0] == '0' ? 0u : (e[0] == '1' ? 1u : 2u);
    if (const char* e = std::getenv("SURF_LEAF_RUN")) c->leafRun = e[0] != '0';
    if (const char* e = std::getenv("SURF_OVERLAP")) c->overlap = e[0] != '0';
    if (const char* e = std::getenv("SURF_LOOP_LAG")) c->loopLag = e[0] != '0';
    if (const char* e = std::getenv("SURF_EXT_LDS_PAD")) c->extLdsPad = (size_t)std::max(0, std::atoi(e));
    if (const char* e = std::getenv("SURF_CON_LDS_PAD")) c->conLdsPad = (size_t)std::max(0, std::atoi(e));
    if (const char* e = std::getenv("SURF_LDS_LIGHTBLAS")) c->ldsLightBlas = e[0] != '0';
    if (const char* e = std::getenv("SURF_REORDER")) c->reorder = e[0] != '0';
    if (const char* e = std::getenv("SURF_TAIL_PAIR")) c->tailPair = e[0] != '0';
    if (const char* e = std::getenv("SURF_DRAIN_SHORT")) c->drainShort = e[0] == '1';
    if (const char* e = std::getenv("SURF_REGEN_FIRST")) c->regenFirst = e[0] == '1';
    if (const char* e = std::getenv("SURF_PIPELINE")) c->pipeline = e[0] != '0';
    if (const char* e = std::getenv("SURF_DENOISE_LDS")) c->dnLdsMax = (uint32_t)std::max(0, std::atoi(e));
    if (const char* e = std::getenv("SURF_SVGF_LDS")) c->svVarStaged = std::atoi(e) != 0;
    if (const char* e = std::getenv("SURF_NLM_LDS")) c->nlStaged = std::atoi(e) != 0;
    if (const char* e = std::getenv("SURF_REGRESS_LDS")) c->rgStaged = std::atoi(e) != 0;
    if (const char* e = std::getenv("SURF_AO_MAP")) c->aoRayMap = e[0] != '0';
    if (const char* e = std::getenv("SURF_ATLAS_MAP")) c->atlasTileMap = e[0] != '0';
    c->width = w;
    c->height = h;
    c->rows = std::move(rows);
    c->npx = (uint32_t)(w * c->rows.size());
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail(nullptr, SURF_ERR_HIP, "stream/event creation failed");
    }
    for (auto& e : c->capEv)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            delete c;
            return fail(nullptr, SURF_ERR_HIP, "event creation failed");
        }
    if (hipMalloc(&c->acc, (size_t)c->npx * sizeof(float4)) != hipSuccess ||
        hipMalloc(&c->dRows, c->rows.size() * sizeof(uint32_t)) != hipSuccess) {
        surf_destroy(c);
        return fail(nullptr, SURF_ERR_OOM, "accumulator allocation failed");
    }
    (void)hipMemset(c->acc, 0, (size_t)c->npx * sizeof(float4));
    (void)hipMemcpy(c->dRows, c->rows.data(), c->rows.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    *out = c;
    return SURF_OK;
}

}  // namespace

extern "C" {

int surf_abi_version(void) { return SURF_ABI_VERSION; }

int surf_device_count(int* count) {
    if (!count) return SURF_ERR_INVALID;
    *count = 0;
    if (hipGetDeviceCount(count) != hipSuccess) { *count = 0; return fail(nullptr, SURF_ERR_NO_DEVICE, "hipGetDeviceCount failed"); }
    return SURF_OK;
}

int surf_create(int dev, uint32_t w, uint32_t h, uint32_t r0, uint32_t r1, surf_ctx** out) {
    if (r0 >= r1 || r1 > h) return fail(nullptr, SURF_ERR_INVALID, "row range out of frame");
    std::vector<uint32_t> rows;
    for (uint32_t r = r0; r < r1; ++r) rows.push_back(r);
    return createCtx(dev, w, h, std::move(rows), out);
}

int surf_create_sharded(int dev, uint32_t w, uint32_t h, uint32_t shard, uint32_t shards, uint32_t block, surf_ctx** out) {
    if (shards == 0 || shard >= shards) return fail(nullptr, SURF_ERR_INVALID, "bad shard index");
    return createCtx(dev, w, h, shardRows(h, shard, shards, block), out);
}

void surf_destroy(surf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    destroyGraph(c);
    freeList(c->sceneAllocs);
    freeList(c->wfAllocs);
    if (c->hctr) (void)hipHostFree(c->hctr);
    if (c->hLimit) (void)hipHostFree(c->hLimit);
    for (auto& sn : c->snap) {
        if (sn.h) (void)hipHostFree(sn.h);
        if (sn.fd) (void)hipHostFree(sn.fd);
        if (sn.ev) (void)hipEventDestroy(sn.ev);
    }
    for (auto& pr : c->tev)
        for (auto& e : pr) if (e) (void)hipEventDestroy(e);
    if (c->rad) (void)hipFree(c->rad);
    if (c->frameDone) (void)hipFree(c->frameDone);
    for (auto& e : c->pev) if (e) (void)hipEventDestroy(e);
    if (c->hPhaseN) (void)hipHostFree(c->hPhaseN);
    if (c->phaseLog) std::fclose(c->phaseLog);
    if (c->acc) (void)hipFree(c->acc);
    if (c->sq) (void)hipFree(c->sq);
    if (c->bk) (void)hipFree(c->bk);
    for (auto& e : c->accEv) if (e) (void)hipEventDestroy(e);
    for (PassPlanes* pp : {&c->aov, &c->aovChain, &c->aovSampled, &c->ao})
        for (void*& p : pp->p) { if (p) (void)hipFree(p); p = nullptr; }
    freeDenoise(c);
    freeTemporal(c);
    freeAdaptive(c);
    c->ssPlanes.free();
    if (c->ssValidDev) (void)hipFree(c->ssValidDev);
    freeRobust(c);
    freeNlm(c);
    freeRegress(c);
    freeErrorMask(c);
    freeDisplay(c);
    freeAtlas(c);
    if (c->dRows) (void)hipFree(c->dRows);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    for (auto& e : c->capEv)
        if (e) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

const char* surf_last_error(const surf_ctx* c) {
    if (c) return c->err.c_str();
    std::lock_guard<std::mutex> l(gErrMutex);
    static thread_local std::string copy;
    copy = gLastError;
    return copy.c_str();
}

int surf_shard_rows(const surf_ctx* c, uint32_t* rows, uint32_t* count) {
    if (!c || !count) return SURF_ERR_INVALID;
    if (rows) std::memcpy(rows, c->rows.data(), c->rows.size() * sizeof(uint32_t));
    *count = (uint32_t)c->rows.size();
    return SURF_OK;
}

int surf_get_device(const surf_ctx* c, int* dev) {
    if (!c || !dev) return SURF_ERR_INVALID;
    *dev = c->device;
    return SURF_OK;
}

int surf_shard_row_list(uint32_t height, uint32_t shard, uint32_t shards, uint32_t block, uint32_t* rows, uint32_t* count) {
    if (!count || shards == 0 || shard >= shards) return fail(nullptr, SURF_ERR_INVALID, "bad shard index");
    const std::vector<uint32_t> r = shardRows(height, shard, shards, block);
    if (rows && !r.empty()) std::memcpy(rows, r.data(), r.size() * sizeof(uint32_t));
    *count = (uint32_t)r.size();
    return SURF_OK;
}

int surf_set_pool_capacity(surf_ctx* c, uint32_t paths) {
    if (!c || paths < 64) return SURF_ERR_INVALID;
    if (c->allocated) return fail(c, SURF_ERR_INVALID, "pool capacity is fixed after the first render");
    c->capacity = paths;
    return SURF_OK;
}

int surf_set_frame_batch(surf_ctx* c, uint32_t frames) {
    if (!c || frames == 0 || (uint64_t)frames * c->npx >= (1ull << 32)) return SURF_ERR_INVALID;
    if (c->allocated) return fail(c, SURF_ERR_INVALID, "frame window is fixed after the first render");
    c->window = frames;
    c->windowFixed = true;
    return SURF_OK;
}

/* Diagnostics: how many paths the segment cap ended in the current stream, and
 * sample ids (slot * npx + shard pixel) of up to 64 of them (unused entries ~0). */
int surf_debug_capped(surf_ctx* c, uint32_t* sids, uint32_t max, uint64_t* count) {
    if (!c || !count) return SURF_ERR_INVALID;
    int rc = ensureDrained(c);
    if (rc) return rc;
    *count = 0;
    if (c->hctr) {
        unsigned long long e[kEvents];
        streamEvents(*c->hctr, e);
        *count = e[7];
    }
    /* the recorded ids: slot blockIdx % 64 of each workgroup that capped a path (racy, any one per slot) */
    uint32_t n = 0;
    if (c->hctr)
        for (uint32_t k = 0; k < 64 && n < max && n < *count; ++k)
            if (c->hctr->capped[k] != kUnset) { if (sids) sids[n] = c->hctr->capped[k]; ++n; }
    if (sids)
        for (uint32_t k = n; k < std::min<uint32_t>(max, 64u); ++k) sids[k] = kUnset;
    return SURF_OK;
}

int surf_debug_issue_order(surf_ctx* c, uint32_t* heavy_pixels, uint32_t* permuted_frames) {
    if (!c || !heavy_pixels || !permuted_frames) return SURF_ERR_INVALID;
    *heavy_pixels = c->permFrames ? c->permA : 0u;
    *permuted_frames = c->permFrames;
    return SURF_OK;
}

int surf_set_tail_policy(surf_ctx* c, uint32_t threshold_paths, uint32_t lanes_per_wave, uint32_t stage_segments) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "ctx is NULL");
    if (lanes_per_wave > 64) return fail(c, SURF_ERR_INVALID, "lanes_per_wave must be <= 64");
    SURF_CHECK(c, hipSetDevice(c->device));
    const int rc = endStream(c);
    if (rc) return rc;
    c->tailPaths = threshold_paths;
    c->tailLanes = lanes_per_wave;
    c->tailBudget = stage_segments;
    return SURF_OK;
}

int surf_set_tail_coop(surf_ctx* c, uint32_t max_paths) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "ctx is NULL");
    SURF_CHECK(c, hipSetDevice(c->device));
    const int rc = endStream(c);
    if (rc) return rc;
    c->coopAll = max_paths;
    return SURF_OK;
}

int surf_set_trace_mode(surf_ctx* c, int mode) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "ctx is NULL");
    if (mode < 0 || mode > 1) return fail(c, SURF_ERR_INVALID, "trace mode must be 0 or 1");
    if (mode == 1 && !waveEligible(c))
        return fail(c, SURF_ERR_INVALID, "one-ray-per-wave traversal needs a BVH stack <= 64 entries");
    c->traceMode = mode;
    return SURF_OK;
}

int surf_set_zero_cutoff(surf_ctx* c, int enabled) {
    if (!c) return SURF_ERR_INVALID;
    int rc = endStream(c);
    if (rc) return rc;
    c->zeroCutoff = enabled < 0 ? -1 : (enabled != 0 ? 1 : 0);
    return SURF_OK;
}

int surf_set_profiling(surf_ctx* c, int enabled) {
    if (!c) return SURF_ERR_INVALID;
    int rc = endStream(c);
    if (rc) return rc;
    c->profiling = enabled != 0;
    return SURF_OK;
}

int surf_set_camera(surf_ctx* c, const surf_camera_ubo* u) {
    if (!c || !u) return SURF_ERR_INVALID;
    if (c->hasCamera && std::memcmp(u, &c->camUbo, sizeof *u) == 0) return SURF_OK;   /* unchanged: keep the stream */
    int rc0 = endStream(c);
    if (rc0) return rc0;
    if (!(u->resolution[0] > 0.0f) || !(u->resolution[1] > 0.0f)) return fail(c, SURF_ERR_INVALID, "camera resolution must be positive");
    DevCamera k{};
    const float pos[3] = {u->position.x, u->position.y, u->position.z};
    std::memcpy(k.pos, pos, sizeof pos);
    k.firstPixel[0] = u->first_pixel.x; k.firstPixel[1] = u->first_pixel.y; k.firstPixel[2] = u->first_pixel.z;
    k.uVec[0] = u->u_vector.x; k.uVec[1] = u->u_vector.y; k.uVec[2] = u->u_vector.z;
    k.vVec[0] = u->v_vector.x; k.vVec[1] = u->v_vector.y; k.vVec[2] = u->v_vector.z;
    k.invW = 1.0f / u->resolution[0];
    k.invH = 1.0f / u->resolution[1];
    k.defocus = (u->defocus_angle == 0.0f) ? 0u : 1u;
    /* sampleDefocusDisk constants (camera.h:73-75), computed once on the host */
    const V3 up = mk3(u->up.x, u->up.y, u->up.z), fwd = mk3(u->fwd.x, u->fwd.y, u->fwd.z);
    const V3 right = normalize(cross(up, fwd));
    const float deg = u->defocus_angle / 2.0f;
    const float radius = u->focal_length * tanf((deg * 3.14159265358979323846264f) * 0.005555555555555f);
    const V3 du = scl(right, radius), dv = scl(lscl(-1.0f, up), radius);
    k.diskU[0] = du.x; k.diskU[1] = du.y; k.diskU[2] = du.z;
    k.diskV[0] = dv.x; k.diskV[1] = dv.y; k.diskV[2] = dv.z;
    c->cam = k;
    dropDerivedPlanes(c);
    c->camUbo = *u;
    c->hasCamera = true;
    destroyGraph(c);     /* camera is a kernel argument of the captured graph */
    return SURF_OK;
}

int surf_render(surf_ctx* c, uint32_t frames, uint32_t firstSample, uint32_t maxSeg, uint32_t spp) {
    if (!c) return SURF_ERR_INVALID;
    if (spp == 0 || spp > 4096) return fail(c, SURF_ERR_INVALID, "samples_per_frame must be 1..4096");
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (!c->hasCamera) return fail(c, SURF_ERR_NO_SCENE, "no camera set");
    if (frames == 0) return SURF_OK;
    if (c->pmOn && c->pmActive == 0) return SURF_OK;      /* an all-zero mask: nothing to trace, nothing changes */
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = allocWavefront(c);
    if (rc) return rc;
    /* continue the open stream only for the next consecutive frames of the same kind */
    if (c->streamActive && ((uint64_t)firstSample != c->baseFrame + targetPasses(c) || maxSeg != c->streamMaxSeg || spp != c->spp))
        if ((rc = endStream(c))) return rc;
    if (!c->streamActive) {
        if ((rc = ensureWindow(c, frames, spp))) return rc;
        if ((rc = startStream(c, firstSample, maxSeg, frames, spp))) return rc;
    }
    if (!c->profiling && (rc = buildGraph(c))) return rc;         /* (re)captured if the ring moved */
    /* this call's device time: an event pair of its own (the pair two calls
     * back is read first, if that call returned with replays in flight) */
    const int tp = c->tevCur;
    if (c->tevPending[tp]) {
        SURF_CHECK(c, hipEventSynchronize(c->tev[tp][1]));
        float ms0 = 0;
        (void)hipEventElapsedTime(&ms0, c->tev[tp][0], c->tev[tp][1]);
        c->stats.ms_total += ms0;
        c->tevPending[tp] = false;
    }
    SURF_CHECK(c, hipEventRecord(c->tev[tp][0], c->stream));
    c->targetFrames += frames;
    /* A one-frame call (the drop-in loop, main.cpp:381-446) may return with up
     * to a pool's worth of its stream not yet issued: the next calls, or the
     * drain a read of the accumulator starts, issue it.  Issuing each call's
     * frame at once would run a short replay per frame on a pool a third full
     * (DESIGN 4 "Pool sizing"); with the lag the pool stays full and the
     * calls replay only as many phases as the stream retires. */
    const uint64_t lag = frames == 1 && c->loopLag ? c->capacity : 0;
    if ((rc = pump(c, false, lag))) return rc;
    SURF_CHECK(c, hipEventRecord(c->tev[tp][1], c->stream));
    if (c->snapCount) {
        /* replays still in flight (a pipelined one-frame call): timed when read */
        c->tevPending[tp] = true;
        c->tevCur ^= 1;
    } else {
        SURF_CHECK(c, hipEventSynchronize(c->tev[tp][1]));
        float ms = 0;
        (void)hipEventElapsedTime(&ms, c->tev[tp][0], c->tev[tp][1]);
        c->stats.ms_total += ms;
    }
    c->totalSamples += (uint64_t)frames * spp;
    c->stats.samples += (uint64_t)frames * spp * c->streamPx;
    return SURF_OK;
}

int surf_clear_accumulator(surf_ctx* c) {
    if (!c) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);
    if (rc) return rc;
    SURF_CHECK(c, hipMemsetAsync(c->acc, 0, (size_t)c->npx * sizeof(float4), c->stream));
    if (c->sq) SURF_CHECK(c, hipMemsetAsync(c->sq, 0, (size_t)c->npx * sizeof(float4), c->stream));
    if (c->bk) SURF_CHECK(c, hipMemsetAsync(c->bk, 0, (size_t)c->bkPlanes * c->npx * sizeof(float4), c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    c->totalSamples = 0;
    std::memset(&c->stats, 0, sizeof c->stats);
    std::memset(c->evBase, 0, sizeof c->evBase);
    c->segMaxBase = 0;
    c->tailFirstRays = 0;
    return resetSensorMask(c);     /* the mask is back to "every pixel" (every valid texel of a surfel sensor) */
}

/* surf_set_surfel_sensor*: the open stream ended, the
 * validity bytes taken from the caller's normals (and the call refused before
 * anything changes if one is unusable), the two planes copied into the
 * context's own (kind: from the host or from the context's device), the graphs
 * of the other sensor's kernels dropped and the mask set back to every valid
 * texel. */
static int setSensor(surf_ctx* c, const void* position, const void* normal, hipMemcpyKind kind, const char* who) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, std::string(who) + ": ctx is NULL");
    if (!position != !normal) return fail(c, SURF_ERR_INVALID, std::string(who) + ": one of position and normal is NULL");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);                     /* a stream's sensor is fixed when it opens */
    if (rc) return rc;
    if (!position) {
        if (c->ssOn) destroyGraph(c);          /* (captured with the surfel kernels) */
        c->ssOn = false;
        c->ssValid = 0;
        return resetSensorMask(c);
    }
    const size_t npx = c->npx, bytes = npx * sizeof(float4);
    /* validity first, from the caller's normals: nothing of the context changes before the planes are known to be usable */
    std::vector<float4> n(npx);
    if (kind == hipMemcpyHostToDevice) std::memcpy(n.data(), normal, bytes);
    else {
        SURF_CHECK(c, hipMemcpyAsync(n.data(), normal, bytes, hipMemcpyDeviceToHost, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
    }
    std::vector<uint8_t> validHost(npx);
    uint32_t valid = 0;
    for (size_t p = 0; p < npx; ++p) {
        const bool v = n[p].x != 0.0f || n[p].y != 0.0f || n[p].z != 0.0f;   /* (a NaN component: valid) */
        /* a nonzero normal whose squared length underflows: cosineSample's retry test dot(R, N) == 0 could hold on every try */
        if (v && (n[p].x * n[p].x + n[p].y * n[p].y) + n[p].z * n[p].z < 1.17549435e-38f)
            return fail(c, SURF_ERR_INVALID, std::string(who) + ": the normal of texel " + std::to_string(p) +
                                                 " is nonzero but its squared length underflows (supply unit normals)");
        validHost[p] = v ? 1 : 0;
        valid += v ? 1u : 0u;
    }
    if ((rc = c->ssPlanes.grow(c, npx))) return rc;
    if (!c->ssValidDev && hipMalloc((void**)&c->ssValidDev, npx) != hipSuccess) {
        (void)hipGetLastError();
        c->ssValidDev = nullptr;
        return fail(c, SURF_ERR_OOM, std::string(who) + ": hipMalloc of " + std::to_string(npx) + " validity bytes failed");
    }
    /* from here the planes are overwritten: a copy that fails leaves the context on the camera, with no mask, not on
     * new planes under the old validity */
    const bool was = c->ssOn;
    c->ssOn = false;
    c->ssValid = 0;
    const auto copies = [&]() -> int {
        SURF_CHECK(c, hipMemcpyAsync(c->ssPlanes[0], position, bytes, kind, c->stream));
        SURF_CHECK(c, hipMemcpyAsync(c->ssPlanes[1], normal, bytes, kind, c->stream));
        SURF_CHECK(c, hipMemcpyAsync(c->ssValidDev, validHost.data(), npx, hipMemcpyHostToDevice, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
        return SURF_OK;
    };
    if ((rc = copies())) {
        if (was) destroyGraph(c);              /* (captured with the surfel kernels) */
        const std::string why = c->err;
        (void)resetSensorMask(c);              /* ssOn is off: every pixel */
        return fail(c, rc, why);
    }
    if (!was) destroyGraph(c);                 /* (captured with the camera kernels) */
    c->ssValidHost.swap(validHost);
    c->ssOn = true;
    c->ssValid = valid;
    return resetSensorMask(c);
}

int surf_set_surfel_sensor(surf_ctx* c, const float* position, const float* normal) {
    return setSensor(c, position, normal, hipMemcpyHostToDevice, "surf_set_surfel_sensor");
}

int surf_set_surfel_sensor_device(surf_ctx* c, const void* position_device, const void* normal_device) {
    return setSensor(c, position_device, normal_device, hipMemcpyDeviceToDevice, "surf_set_surfel_sensor_device");
}

int surf_get_sensor(surf_ctx* c, int* kind, uint32_t* valid) {
    if (!c) return fail(nullptr, SURF_ERR_INVALID, "surf_get_sensor: ctx is NULL");
    if (kind) *kind = c->ssOn ? SURF_SENSOR_SURFELS : SURF_SENSOR_CAMERA;
    if (valid) *valid = c->ssOn ? c->ssValid : c->npx;
    return SURF_OK;
}

int surf_read_accumulator(surf_ctx* c, float* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, c->acc, (size_t)c->npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_copy_accumulator_device(surf_ctx* c, void* dst) {
    if (!c || !dst) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(dst, c->acc, (size_t)c->npx * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_set_sample_squares(surf_ctx* c, int enabled) {
    if (!c) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    if (c->totalSamples != 0)
        return fail(c, SURF_ERR_INVALID, "surf_set_sample_squares: the accumulator holds samples whose squares are lost; call "
                                         "surf_clear_accumulator first");
    if (enabled && !c->sq) {
        if (hipMalloc(&c->sq, (size_t)c->npx * sizeof(float4)) != hipSuccess || !c->sq) {
            c->sq = nullptr;
            (void)hipGetLastError();
            return fail(c, SURF_ERR_OOM, "hipMalloc of the squares plane (" + std::to_string((size_t)c->npx * sizeof(float4)) + " bytes) failed");
        }
        SURF_CHECK(c, hipMemsetAsync(c->sq, 0, (size_t)c->npx * sizeof(float4), c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
    }
    c->sqOn = enabled != 0;
    return SURF_OK;
}

/* surf_read_sample_squares / surf_copy_sample_squares_device */
static int copySquares(surf_ctx* c, void* dst, hipMemcpyKind kind) {
    if (!c || !dst) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    if (!c->sqOn) return fail(c, SURF_ERR_INVALID, "sample squares are off (surf_set_sample_squares)");
    SURF_CHECK(c, hipMemcpyAsync(dst, c->sq, (size_t)c->npx * sizeof(float4), kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_read_sample_squares(surf_ctx* c, float* out) { return copySquares(c, out, hipMemcpyDeviceToHost); }

int surf_copy_sample_squares_device(surf_ctx* c, void* dst) { return copySquares(c, dst, hipMemcpyDeviceToDevice); }

int surf_set_sample_buckets(surf_ctx* c, uint32_t M) {
    if (!c) return SURF_ERR_INVALID;
    if (M != 0 && M != 2 && M != 4 && M != 8 && M != 16)
        return fail(c, SURF_ERR_INVALID, "surf_set_sample_buckets: M is none of 0, 2, 4, 8 and 16");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    if (c->totalSamples != 0)
        return fail(c, SURF_ERR_INVALID, "surf_set_sample_buckets: the accumulator holds samples whose buckets are lost; call "
                                         "surf_clear_accumulator first");
    if (M > c->bkPlanes) {
        const size_t bytes = (size_t)M * c->npx * sizeof(float4);
        float4* planes = nullptr;
        if (hipMalloc(&planes, bytes) != hipSuccess || !planes) {
            (void)hipGetLastError();
            return fail(c, SURF_ERR_OOM, "hipMalloc of the bucket planes (" + std::to_string(bytes) + " bytes) failed");
        }
        if (c->bk) (void)hipFree(c->bk);
        c->bk = planes;
        c->bkPlanes = M;
    }
    /* the accumulator is empty, so the planes are too: zeroed here whatever an earlier, other M left in them */
    if (c->bk) {
        SURF_CHECK(c, hipMemsetAsync(c->bk, 0, (size_t)c->bkPlanes * c->npx * sizeof(float4), c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
    }
    c->bkM = M;
    return SURF_OK;
}

int surf_get_sample_buckets(const surf_ctx* c, uint32_t* M) {
    if (!c || !M) return SURF_ERR_INVALID;
    *M = c->bkM;
    return SURF_OK;
}

/* surf_read_sample_buckets / surf_copy_sample_buckets_device */
static int copyBuckets(surf_ctx* c, void* dst, hipMemcpyKind kind) {
    if (!c || !dst) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    if (!c->bkM) return fail(c, SURF_ERR_INVALID, "sample buckets are off (surf_set_sample_buckets)");
    SURF_CHECK(c, hipMemcpyAsync(dst, c->bk, (size_t)c->bkM * c->npx * sizeof(float4), kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_read_sample_buckets(surf_ctx* c, float* out) { return copyBuckets(c, out, hipMemcpyDeviceToHost); }

int surf_copy_sample_buckets_device(surf_ctx* c, void* dst) { return copyBuckets(c, dst, hipMemcpyDeviceToDevice); }

int surf_read_aov(surf_ctx* c, int plane, void* out) {
    return copyPlane(c, true, &surf_ctx::aov, plane, out, hipMemcpyDeviceToHost, [&] { return ensureAov(c); });
}

int surf_copy_aov_device(surf_ctx* c, int plane, void* dst) {
    return copyPlane(c, true, &surf_ctx::aov, plane, dst, hipMemcpyDeviceToDevice, [&] { return ensureAov(c); });
}

int surf_debug_aov_time(surf_ctx* c, float* kernel_ms) { return passTime(c, &surf_ctx::aov, kernel_ms); }

int surf_read_aov_chain(surf_ctx* c, int plane, uint32_t max_links, void* out) {
    return copyPlane(c, true, &surf_ctx::aovChain, plane, out, hipMemcpyDeviceToHost, [&] { return ensureAovChain(c, max_links); });
}

int surf_copy_aov_chain_device(surf_ctx* c, int plane, uint32_t max_links, void* dst) {
    return copyPlane(c, true, &surf_ctx::aovChain, plane, dst, hipMemcpyDeviceToDevice, [&] { return ensureAovChain(c, max_links); });
}

int surf_debug_aov_chain_time(surf_ctx* c, float* kernel_ms) { return passTime(c, &surf_ctx::aovChain, kernel_ms); }

int surf_set_filter_guides(surf_ctx* c, int guides, uint32_t max_links) {
    if (!c) return SURF_ERR_INVALID;
    if (guides != SURF_GUIDES_FIRST_HIT && guides != SURF_GUIDES_CHAIN) return fail(c, SURF_ERR_INVALID, "surf_set_filter_guides: unknown guides mode");
    if (max_links > SURF_AOV_CHAIN_MAX_LINKS)
        return fail(c, SURF_ERR_INVALID, "surf_set_filter_guides: max_links is above SURF_AOV_CHAIN_MAX_LINKS (" + std::to_string(SURF_AOV_CHAIN_MAX_LINKS) + ")");
    c->guides = guides;
    c->guideLinks = max_links;
    return SURF_OK;
}

int surf_get_filter_guides(const surf_ctx* c, int* guides, uint32_t* max_links) {
    if (!c || !guides || !max_links) return SURF_ERR_INVALID;
    *guides = c->guides;
    *max_links = c->guides == SURF_GUIDES_SAMPLED ? c->guideSampled.samples : c->guideLinks;
    return SURF_OK;
}

int surf_aov_sampled_default_params(surf_aov_sampled_params* p) {
    if (!p) return SURF_ERR_INVALID;
    *p = surf_aov_sampled_params{16u, 0u, SURF_MATTE_INSTANCE, 0u};
    return SURF_OK;
}

int surf_read_aov_sampled(surf_ctx* c, const surf_aov_sampled_params* p, int plane, void* out) {
    return copyPlane(c, p != nullptr, &surf_ctx::aovSampled, plane, out, hipMemcpyDeviceToHost, [&] { return ensureAovSampled(c, *p); });
}

int surf_copy_aov_sampled_device(surf_ctx* c, const surf_aov_sampled_params* p, int plane, void* dst) {
    return copyPlane(c, p != nullptr, &surf_ctx::aovSampled, plane, dst, hipMemcpyDeviceToDevice, [&] { return ensureAovSampled(c, *p); });
}

int surf_debug_aov_sampled_time(surf_ctx* c, float* kernel_ms) { return passTime(c, &surf_ctx::aovSampled, kernel_ms); }

int surf_ao_default_params(surf_ao_params* p) {
    if (!p) return SURF_ERR_INVALID;
    *p = surf_ao_params{16u, 0u, 1.0f, 1e-5f, SURF_AO_FIRST_HIT, 8u, {0u, 0u}};
    return SURF_OK;
}

int surf_read_ao(surf_ctx* c, const surf_ao_params* p, int plane, void* out) {
    return copyPlane(c, p != nullptr, &surf_ctx::ao, plane, out, hipMemcpyDeviceToHost, [&] { return ensureAo(c, *p); });
}

int surf_copy_ao_device(surf_ctx* c, const surf_ao_params* p, int plane, void* dst) {
    return copyPlane(c, p != nullptr, &surf_ctx::ao, plane, dst, hipMemcpyDeviceToDevice, [&] { return ensureAo(c, *p); });
}

int surf_debug_ao_time(surf_ctx* c, float* kernel_ms) { return passTime(c, &surf_ctx::ao, kernel_ms); }

int surf_set_filter_guides_sampled(surf_ctx* c, const surf_aov_sampled_params* p) {
    if (!c || !p) return SURF_ERR_INVALID;
    if (!aovSampledParamsOk(p)) return fail(c, SURF_ERR_INVALID, "surf_set_filter_guides_sampled: samples outside 1.." + std::to_string(SURF_AOVS_MAX_SAMPLES) + ", an unknown key or reserved != 0");
    c->guides = SURF_GUIDES_SAMPLED;
    c->guideSampled = *p;
    return SURF_OK;
}

int surf_finalize_rgba8(surf_ctx* c, uint32_t* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    if (c->totalSamples == 0) return fail(c, SURF_ERR_INVALID, "nothing rendered since the last clear");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = allocWavefront(c);
    if (rc) return rc;
    if ((rc = ensureDrained(c))) return rc;
    const float inv = 1.0f / (float)c->totalSamples;     /* renderer.cpp:160 */
    hipLaunchKernelGGL(k_finalize, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->acc,
                       c->dOutRGBA, c->npx, inv);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, hipMemcpyAsync(out, c->dOutRGBA, (size_t)c->npx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_display_rgba8(surf_ctx* c, uint32_t* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    if (c->totalSamples == 0) return fail(c, SURF_ERR_INVALID, "nothing rendered since the last clear");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = allocWavefront(c);
    if (rc) return rc;
    if ((rc = ensureDrained(c))) return rc;
    const float inv = 1.0f / (float)c->totalSamples;
    hipLaunchKernelGGL(k_display, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->acc,
                       c->dOutRGBA, c->npx, inv);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, hipMemcpyAsync(out, c->dOutRGBA, (size_t)c->npx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_finalize_rgba8_weighted(surf_ctx* c, int display, uint32_t* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = allocWavefront(c);
    if (rc) return rc;
    if ((rc = ensureDrained(c))) return rc;
    hipLaunchKernelGGL(k_pack_weighted, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const float4*)c->acc,
                       c->dOutRGBA, c->npx, display ? 1u : 0u);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, hipMemcpyAsync(out, c->dOutRGBA, (size_t)c->npx * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* The CPU twin: packWeighted compiled for the host. */
int surf_pack_rgba8_weighted(const float* acc, uint32_t n, int display, uint32_t* out) {
    if (!acc || !out) return fail(nullptr, SURF_ERR_INVALID, "surf_pack_rgba8_weighted: NULL argument");
    for (size_t p = 0; p < n; ++p) {
        float4 a;                                                /* the caller's plane need not be 16-byte aligned */
        std::memcpy(&a, acc + 4 * p, sizeof a);
        out[p] = packWeighted(a, display != 0);
    }
    return SURF_OK;
}

int surf_get_stats(surf_ctx* c, surf_stats* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    int rc = ensureDrained(c);
    if (rc) return rc;
    surf_stats s = c->stats;
    unsigned long long ev[kEvents];
    unsigned long long cur[kEvents] = {};
    if (c->streamActive && c->hctr) streamEvents(*c->hctr, cur);
    for (int k = 0; k < kEvents; ++k) ev[k] = c->evBase[k] + cur[k];
    s.n_ext = ev[0]; s.n_hit = ev[1]; s.n_cont = ev[2]; s.n_shadow = ev[3]; s.n_acc = ev[4]; s.n_unocc = ev[5];
    s.tail_paths = ev[6];
    s.n_ext_wavefront = ev[8] - c->tailFirstRays;
    s.n_shadow_overflow = ev[9];
    s.max_segments = std::max(c->segMaxBase, (c->streamActive && c->hctr) ? c->hctr->segMax : 0u);
    s.stack_depth = c->stackDepth;
    s.pool_capacity = c->capacity;
    s.frame_window = c->window;
    if (c->totalSamples) {
        /* Lumen energy, renderer.cpp:191-201: per-pixel terms on the GPU
         * (k_energy_terms), then the reference's serial sum in pixel order */
        if ((rc = allocWavefront(c))) return rc;
        const float inv = 1.0f / (float)c->totalSamples;
        float* terms = reinterpret_cast<float*>(c->dOutRGBA);          /* npx words, reused */
        hipLaunchKernelGGL(k_energy_terms, dim3((c->npx + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream,
                           (const float4*)c->acc, terms, c->npx, inv);
        SURF_CHECK(c, hipGetLastError());
        std::vector<float> h(c->npx);
        SURF_CHECK(c, hipMemcpyAsync(h.data(), terms, (size_t)c->npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
        float e = 0.0f;
        for (size_t p = 0; p < c->npx; ++p) e = e + h[p];
        s.energy = e;
    }
    *out = s;
    return SURF_OK;
}

int surf_synchronize(surf_ctx* c) {
    if (!c) return SURF_ERR_INVALID;
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = ensureDrained(c);
    if (rc) return rc;
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_trace_closest(surf_ctx* c, uint32_t n, const float* o, const float* d, float* ot, float* ou, float* ov,
                       uint32_t* oi, uint32_t* op) {
    if (!c || (n && (!o || !d || !ot || !ou || !ov || !oi || !op))) return SURF_ERR_INVALID;
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return SURF_OK;
    if (c->traceMode == 1 && !waveEligible(c))
        return fail(c, SURF_ERR_INVALID, "scene no longer fits the selected cooperative traversal");
    SURF_CHECK(c, hipSetDevice(c->device));
    std::vector<float4> t;
    std::vector<uint2> ip;
    if (int rc = traceClosestRays(c, n, o, d, c->traceMode == 1, &t, ip, "trace_closest")) return rc;
    for (uint32_t i = 0; i < n; ++i) { ot[i] = t[i].x; ou[i] = t[i].y; ov[i] = t[i].z; oi[i] = ip[i].x; op[i] = ip[i].y; }
    return SURF_OK;
}

int surf_trace_any(surf_ctx* c, uint32_t n, const float* o, const float* d, const float* tm, uint8_t* occ) {
    if (!c || (n && (!o || !d || !tm || !occ))) return SURF_ERR_INVALID;
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (n == 0) return SURF_OK;
    if (c->traceMode == 1 && !waveEligible(c))
        return fail(c, SURF_ERR_INVALID, "scene no longer fits the selected cooperative traversal");
    SURF_CHECK(c, hipSetDevice(c->device));
    std::vector<void*> tmp;
    float *dO, *dD, *dM; uint8_t* dR;
    int rc;
    if ((rc = devAlloc(c, tmp, &dO, 3 * (size_t)n)) || (rc = devAlloc(c, tmp, &dD, 3 * (size_t)n)) ||
        (rc = devAlloc(c, tmp, &dM, n)) || (rc = devAlloc(c, tmp, &dR, n))) { freeList(tmp); return rc; }
    (void)hipMemcpyAsync(dO, o, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dD, d, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dM, tm, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    const Variant v = variantOf(c);
    if (c->traceMode == 1) {
        const auto k = traceAnyCoopKernel(c, v);
        hipLaunchKernelGGL(k.fn, dim3(n), dim3(64), k.lds, c->stream, c->S, (const float*)dO, (const float*)dD, (const float*)dM, n,
                           dR, recStackWords(c));
    } else {
        const auto k = traceAnyKernel(c, v);
        hipLaunchKernelGGL(k.fn, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), k.lds, c->stream, c->S, (const float*)dO,
                           (const float*)dD, (const float*)dM, n, dR, stackWords(c, kBlock));
    }
    (void)hipMemcpyAsync(occ, dR, n, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    freeList(tmp);
    if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string("trace_any: ") + hipGetErrorString(e));
    return SURF_OK;
}

int surf_debug_shadow_keys(surf_ctx* c, uint32_t n, const float* o, const float* d, const float* tmax, const uint32_t* light,
                           uint32_t* keys, uint32_t* bins, float* layout) {
    if (!c || !bins || (n && (!o || !d || !tmax || !light || !keys))) return SURF_ERR_INVALID;
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    *bins = shadowBins(c);
    if (layout) {
        const DevScene& S = c->S;
        for (int a = 0; a < 3; ++a) { layout[a] = S.cellLo[a]; layout[3 + a] = S.cellScale[a]; }
        layout[6] = (float)S.nHeavy;
        for (int h = 0; h < 3; ++h) {
            const float b[6] = {S.hvLo[h].x, S.hvLo[h].y, S.hvLo[h].z, S.hvHi[h].x, S.hvHi[h].y, S.hvHi[h].z};
            std::copy(b, b + 6, layout + 7 + 6 * h);
        }
    }
    if (n == 0) return SURF_OK;
    SURF_CHECK(c, hipSetDevice(c->device));
    std::vector<void*> tmp;
    float *dO, *dD, *dM; uint32_t *dL, *dK;
    int rc;
    if ((rc = devAlloc(c, tmp, &dO, 3 * (size_t)n)) || (rc = devAlloc(c, tmp, &dD, 3 * (size_t)n)) ||
        (rc = devAlloc(c, tmp, &dM, n)) || (rc = devAlloc(c, tmp, &dL, n)) || (rc = devAlloc(c, tmp, &dK, n))) { freeList(tmp); return rc; }
    (void)hipMemcpyAsync(dO, o, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dD, d, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dM, tmax, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dL, light, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_shadow_keys, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->S, *bins, (const float*)dO,
                       (const float*)dD, (const float*)dM, (const uint32_t*)dL, n, dK);
    (void)hipMemcpyAsync(keys, dK, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    freeList(tmp);
    if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string("debug_shadow_keys: ") + hipGetErrorString(e));
    return SURF_OK;
}

int surf_debug_connect_staging(surf_ctx* c, uint32_t* records, uint32_t* triangles) {
    if (!c || !records || !triangles) return SURF_ERR_INVALID;
    *records = c->connectStaged ? c->S.sbRecN : 0u;
    *triangles = c->connectStaged ? c->S.sbTriN : 0u;
    return SURF_OK;
}

int surf_debug_kernel_selection(surf_ctx* c, uint32_t* lds_tables, uint32_t* stack16, uint32_t* lane_two_level, uint32_t* wave_eligible) {
    if (!c || !lds_tables || !stack16 || !lane_two_level || !wave_eligible) return SURF_ERR_INVALID;
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    const Variant v = variantOf(c);
    *lds_tables = v.lds ? 1u : 0u;
    *stack16 = v.sk16 ? 1u : 0u;
    *lane_two_level = v.laneW ? 1u : 0u;
    *wave_eligible = waveEligible(c) ? 1u : 0u;
    return SURF_OK;
}

int surf_debug_segment_cycles(surf_ctx* c, const float* path12, uint32_t reps, uint64_t* cycles15) {
    if (!c || !path12 || !cycles15 || reps == 0) return SURF_ERR_INVALID;
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (!waveEligible(c)) return fail(c, SURF_ERR_INVALID, "scene does not fit the one-ray-per-wave traversal");
    SURF_CHECK(c, hipSetDevice(c->device));
    unsigned long long* d = nullptr;
    SURF_CHECK(c, hipMalloc(&d, 16 * sizeof(unsigned long long)));
    const float4 o4 = make_float4(path12[0], path12[1], path12[2], path12[3]);
    const float4 d4 = make_float4(path12[4], path12[5], path12[6], path12[7]);
    const float4 T4 = make_float4(path12[8], path12[9], path12[10], path12[11]);
    const auto k = segmentCyclesKernel(c, variantOf(c));
    hipLaunchKernelGGL(k.fn, dim3(1), dim3(64), k.lds, c->stream, c->S, o4, d4, T4, reps, d, recStackWords(c));
    hipError_t e = hipMemcpyAsync(cycles15, d, 15 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string("segment cycles: ") + hipGetErrorString(e));
    return SURF_OK;
}

int surf_debug_math(surf_ctx* c, int op, uint32_t n, const float* in, float* out) {
    if (!c || op < SURF_MATH_EXPF || op > SURF_MATH_SINCOSF || (n && (!in || !out))) return SURF_ERR_INVALID;
    if (n == 0) return SURF_OK;
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t per = op == SURF_MATH_SINCOSF ? 2 : 1;
    std::vector<void*> tmp;
    float *dIn, *dOut;
    int rc;
    if ((rc = devAlloc(c, tmp, &dIn, (size_t)n)) || (rc = devAlloc(c, tmp, &dOut, per * (size_t)n))) { freeList(tmp); return rc; }
    (void)hipMemcpyAsync(dIn, in, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)n + kBlock - 1) / kBlock, 4096);    /* grid-stride beyond */
    hipLaunchKernelGGL(k_debug_math, dim3(blocks), dim3(kBlock), 0, c->stream, (uint32_t)op, n, (const float*)dIn, dOut);
    (void)hipMemcpyAsync(out, dOut, 4 * per * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    freeList(tmp);
    if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string("debug_math: ") + hipGetErrorString(e));
    return SURF_OK;
}

/* surf_debug_math's ops and output layout through the host build of the same source */
int surf_debug_math_host(int op, uint32_t n, const float* in, float* out) {
    if (op < SURF_MATH_EXPF || op > SURF_MATH_SINCOSF || (n && (!in || !out))) return SURF_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) {
        if (op == SURF_MATH_EXPF) out[i] = surfdev::gExpf(in[i]);
        else if (op == SURF_MATH_SINF) out[i] = surfdev::gSinf(in[i]);
        else if (op == SURF_MATH_COSF) out[i] = surfdev::gCosf(in[i]);
        else surfdev::gSinCosf(in[i], out[2 * i], out[2 * i + 1]);
    }
    return SURF_OK;
}

int surf_debug_trace_paths(surf_ctx* c, uint32_t n, const float* o, const float* d, const uint32_t* seed, uint32_t max_segments,
                           int mode, float* out_energy_segments, uint32_t* out_seed) {
    if (!c || (n && (!o || !d || !seed || !out_energy_segments || !out_seed))) return SURF_ERR_INVALID;
    if (max_segments < 1u || max_segments > 4096u) return fail(c, SURF_ERR_INVALID, "debug_trace_paths: max_segments must be 1..4096");
    if (mode < 0 || mode > 1) return fail(c, SURF_ERR_INVALID, "debug_trace_paths: mode must be 0 or 1");
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (mode == 1 && !waveEligible(c))
        return fail(c, SURF_ERR_INVALID, "one-ray-per-wave traversal needs a BVH stack <= 64 entries");
    if (n == 0) return SURF_OK;
    SURF_CHECK(c, hipSetDevice(c->device));
    std::vector<void*> tmp;
    float *dO, *dD; uint32_t *dS, *dR; float4* dE;
    int rc;
    if ((rc = devAlloc(c, tmp, &dO, 3 * (size_t)n)) || (rc = devAlloc(c, tmp, &dD, 3 * (size_t)n)) || (rc = devAlloc(c, tmp, &dS, n)) ||
        (rc = devAlloc(c, tmp, &dE, n)) || (rc = devAlloc(c, tmp, &dR, n))) { freeList(tmp); return rc; }
    (void)hipMemcpyAsync(dO, o, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dD, d, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    (void)hipMemcpyAsync(dS, seed, 4 * (size_t)n, hipMemcpyHostToDevice, c->stream);
    const uint32_t cutoff = c->zeroCutoff != 0 ? 1u : 0u;       /* automatic (-1): on, as for one-sample frames */
    const Variant v = variantOf(c);
    if (mode == 1) {
        const auto k = debugPathsWaveKernel(c, v);
        hipLaunchKernelGGL(k.fn, dim3(n), dim3(64), k.lds, c->stream, c->S, (const float*)dO, (const float*)dD, (const uint32_t*)dS, n,
                           max_segments, cutoff, dE, dR, recStackWords(c));
    } else {
        const auto k = debugPathsLaneKernel(c, v);
        hipLaunchKernelGGL(k.fn, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), k.lds, c->stream, c->S, (const float*)dO,
                           (const float*)dD, (const uint32_t*)dS, n, max_segments, cutoff, dE, dR, stackWords(c, kBlock));
    }
    (void)hipMemcpyAsync(out_energy_segments, dE, 16 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(out_seed, dR, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e = hipStreamSynchronize(c->stream);
    freeList(tmp);
    if (e != hipSuccess) return fail(c, SURF_ERR_HIP, std::string("debug_trace_paths: ") + hipGetErrorString(e));
    return SURF_OK;
}

int surf_pack_rgba8(const float* acc, uint32_t n, float inv, int display, uint32_t* out) {
    if ((n && (!acc || !out))) return fail(nullptr, SURF_ERR_INVALID, "bad arguments");
    for (uint32_t p = 0; p < n; ++p) {
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k) {
            const uint32_t c8 = packChannel((acc[4 * (size_t)p + k] * inv) * 255.0f);
            w |= (display ? displayChannel(c8) : c8) << (8 * k);
        }
        out[p] = w;
    }
    return SURF_OK;
}

/* Host restatements of the glibc kernels' libm, for CPU tests (same source as the device). */
float surf_ref_sinf(float x) { return surfdev::gSinf(x); }
float surf_ref_cosf(float x) { return surfdev::gCosf(x); }
float surf_ref_expf(float x) { return surfdev::gExpf(x); }

}  // extern "C"
