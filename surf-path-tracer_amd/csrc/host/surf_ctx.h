/*
 * surf_ctx.h -- internal: the device context behind include/surf_hip.h, the two
 * records the image-space filters keep on it (PlaneGroup, StageTimer) and the
 * helpers every host translation unit of the library uses (error reporting,
 * device allocation lists, scene-table upload).  Includes no kernel.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "surf_hip.h"
#include "device/types.h"

using namespace surfdev;                     /* internal header: the host code names the shared records unqualified */

constexpr uint32_t kMaxStack = 120;         /* LDS stack entries per ray (block 256 -> 120 KiB max) */

/* N device images of `cap` 16-byte records each that a filter keeps on the
 * context: allocated on first use, grown (contents dropped) only when a larger
 * frame arrives, freed with the context.  `what` names the group in an
 * out-of-memory message. */
template <int N>
struct PlaneGroup {
    const char* what;
    float4* p[N] = {};
    size_t cap = 0;
    float4* operator[](int k) const { return p[k]; }
    int grow(surf_ctx* c, size_t npx);
    void free() {
        for (float4*& q : p) { if (q) (void)hipFree(q); q = nullptr; }
        cap = 0;
    }
};

/* The device times of a filter's last run: N stages between N + 1 events on
 * the context's stream, created on first use.  mark(i) records event i, the
 * start of stage i and the end of stage i - 1; collect(n) waits for event n and
 * fills ms[0..n), zeroing the rest; read() is the body of a surf_debug_*_time. */
template <int N>
struct StageTimer {
    hipEvent_t ev[N + 1] = {};
    float ms[N] = {};
    hipError_t mark(int i, hipStream_t stream) {
        if (!ev[i])
            if (const hipError_t e = hipEventCreate(&ev[i]); e != hipSuccess) return e;
        return hipEventRecord(ev[i], stream);
    }
    hipError_t collect(int n) {
        if (const hipError_t e = hipEventSynchronize(ev[n]); e != hipSuccess) return e;
        for (int k = 0; k < N; ++k) {
            ms[k] = 0.0f;
            if (k < n) (void)hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]);
        }
        return hipSuccess;
    }
    void read(float* out, uint32_t count) const {
        for (uint32_t k = 0; k < count; ++k) out[k] = k < (uint32_t)N ? ms[k] : 0.0f;
    }
    void destroy() {
        for (hipEvent_t& e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
};

/* The cached planes of one per-pixel plane pass (first-hit, chain and sampled
 * feature buffers, ambient occlusion): `count` device planes of npx 16-byte
 * records, allocated on first use and freed with the context; valid until
 * dropDerivedPlanes or a read with another key (the key is kept beside the
 * record); ms is the device time of the pass's last launch
 * (surf_debug_*_time).  ensurePlanes in surf_hip.hip is the one driver. */
struct PassPlanes {
    int count;
    void* p[SURF_AOVS_COUNT] = {};   /* the most planes a pass has */
    bool valid = false;
    float ms = 0.0f;
};

struct surf_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    uint32_t width = 0, height = 0;
    std::vector<uint32_t> rows;
    uint32_t npx = 0;
    uint32_t capacity = 0;
    uint32_t window = 0;           /* frames whose samples may be in flight (radiance slots; ensureWindow) */
    bool windowFixed = false;      /* set by surf_set_frame_batch */
    bool profiling = false;
    std::string err;

    /* scene */
    bool hasScene = false;
    uint32_t extBlock = 128;       /* k_extend workgroup size (SURF_EXTEND_BLOCK=128|256): 128 measured 5 % faster on k_extend */
    bool connectGlobal = false;    /* k_connect reads its tables from global memory (SURF_CONNECT_GLOBAL=1, tuning) */
    bool extStack16 = true;        /* k_extend's stack in 16-bit entries when node indices fit (SURF_EXT_STACK16=0: 32-bit) */
    bool regenCount = true;        /* k_regen_count fills the next pool and counts it for its sort (SURF_REGEN_COUNT=0: k_regen + k_bincount) */
    bool ldsTables = false;        /* instance/material/light tables fit the per-workgroup LDS copy */
    DevScene S{};
    std::vector<void*> sceneAllocs;
    uint32_t stackDepth = 0;
    uint32_t nInstances = 0, nTriangles = 0, nBlasNodes = 0;
    /* what surf_update_instances may change: instance records, TLAS, lights */
    uint32_t nMaterials = 0, nLightsUp = 0, tlasNodeCount = 0, maxBlasDepth = 0;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, std::array<float4, 4>> blasRoots;  /* (node, idx, tri offset) -> root record */
    std::map<uint32_t, std::array<double, 6>> blasBounds;   /* tri offset -> bounds of its BLAS's triangles (v0, v0+e1, v0+e2) */
    std::map<uint32_t, uint32_t> blasSlots;                  /* tri offset -> index slots (triangles) of its BLAS */
    /* issue order: the pixels whose centre ray first hits a heavy instance
     * (long Russian-roulette paths start there) are issued for all frames of a
     * multi-frame stream before the rest (SURF_REORDER=0: frame-major) */
    bool reorder = true;
    bool permValid = false;
    uint32_t* dPerm = nullptr;
    /* first-hit feature buffers (surf_read_aov, k_aov): valid until the camera,
     * the scene or the instances change (dropDerivedPlanes) */
    PassPlanes aov{SURF_AOV_COUNT};
    /* the same four planes traced through mirrors and glass (surf_read_aov_chain,
     * k_aov_chain): valid until then or another max_links */
    PassPlanes aovChain{SURF_AOV_COUNT};
    uint32_t aovChainLinks = 0;    /* the max_links the cached planes were traced with */
    /* which planes surf_denoise and surf_denoise_sampled read (surf_set_filter_guides) */
    int guides = SURF_GUIDES_FIRST_HIT;
    uint32_t guideLinks = 8;
    /* the sampled feature buffers (surf_read_aov_sampled, k_aov_sampled): valid
     * until then or a read with other params */
    PassPlanes aovSampled{SURF_AOVS_COUNT};
    surf_aov_sampled_params aovSampledParams{};   /* the params the cached planes were traced with */
    surf_aov_sampled_params guideSampled{};       /* the params of SURF_GUIDES_SAMPLED (surf_set_filter_guides_sampled) */
    /* ambient occlusion (surf_read_ao, k_ao): valid until then or a read with
     * other params */
    PassPlanes ao{SURF_AO_COUNT};
    surf_ao_params aoParams{};         /* the params the cached planes were traced with */
    bool aoRayMap = true;              /* A/B (SURF_AO_MAP): one lane per ray (1), one lane per pixel (0) */
    /* the a-trous denoiser (surf_denoise*, host/denoise.hip): dn, the scratch
     * every a-trous filter runs in -- the two ping-pong levels, the packed
     * normal and position guides -- and, for surf_denoise_image, the four
     * uploaded planes */
    PlaneGroup<4> dn{"the a-trous scratch"};
    PlaneGroup<4> dnIn{"surf_denoise_image's planes"};
    StageTimer<kDenoiseMaxIterations + 1> dnTime;   /* prepare, then the iterations of the last run (surf_debug_denoise_time) */
    /* largest a-trous step whose tile is staged in LDS (SURF_DENOISE_LDS; 0 =
     * every step reads its taps from global memory).  2: staging takes a third
     * off the launches at steps 1 and 2 and adds 10 % at step 4 (MEASUREMENTS
     * "Denoiser") */
    uint32_t dnLdsMax = 2;
    /* temporal accumulation (surf_temporal*, host/temporal.hip): the state a
     * frame leaves for the next -- history (rgb, n), position and the packed
     * normal + instance id, as two sets of three images used in turn
     * (tp[3 * tpCur ..] is the stored one), tp[6] the blended output -- then
     * the camera and the instance records that frame saw.  surf_temporal_image
     * has images of its own (four current planes, three previous, two
     * outputs). */
    PlaneGroup<7> tp{"the temporal state"};
    int tpCur = 0;
    bool tpHave = false;           /* a previous frame is stored (dropped by surf_upload_scene and surf_temporal_reset) */
    surf_camera_ubo tpCam{};
    std::vector<surf_gpu_instance> tpInst;
    PlaneGroup<9> tpIn{"surf_temporal_image's planes"};
    float* tpMotion = nullptr;     /* the motion table on the device, tpMotionCap records */
    uint32_t tpMotionCap = 0;
    std::vector<float> tpMotionHost;
    StageTimer<1> tpTime;          /* the last k_temporal launch (surf_debug_temporal_time) */
    /* the variance-guided filter (surf_svgf*, host/svgf.hip) shares the
     * temporal state above and the denoiser's scratch (dn) and adds: the
     * luminance moments as a plane pair used in turn (sv[svCur] the stored
     * one; svHave: it belongs to the stored history -- surf_temporal_accumulate
     * clears it) and sv[2], two float planes: the variance entering and leaving
     * the filter.  surf_svgf_image has images of its own beside tpIn: albedo,
     * previous moments, moments out, the two variances. */
    PlaneGroup<3> sv{"the variance-guided filter's moments"};
    int svCur = 0;
    bool svHave = false;
    PlaneGroup<4> svIn{"surf_svgf_image's planes"};
    StageTimer<kDenoiseMaxIterations + 2> svTime;   /* k_temporal, guides + variance, then the iterations of the last run (surf_debug_svgf_time) */
    /* the variance kernel takes its 7 x 7 taps from an LDS copy of the tile
     * (SURF_SVGF_LDS=0: from global memory; MEASUREMENTS "Variance-guided filter") */
    bool svVarStaged = true;
    /* the firefly clamp (surf_svgf_ext.firefly_scale, surf_firefly_image): ff
     * the clamped accumulator A' the frame's other kernels read, ffIn the two
     * planes surf_firefly_image uploads. */
    PlaneGroup<1> ff{"the firefly clamp's image"};
    PlaneGroup<2> ffIn{"surf_firefly_image's planes"};
    StageTimer<1> ffTime;          /* the last k_firefly launch (surf_debug_firefly_time) */
    /* the sample-variance-guided filter and the noise estimate (surf_denoise_sampled*,
     * surf_noise_*, host/svgf.hip) share the denoiser's scratch (dn) and add,
     * each sized to what it stores (the capacities count 16-byte records):
     * sdVar, two float planes (the variance entering and leaving the filter,
     * 8 B per pixel); sdErr, the noise estimate's sums in its first record and
     * behind them the error image (4 B per pixel); sdAQ, the accumulator and
     * squares planes the two image forms upload, and sdIn, the three feature
     * planes surf_denoise_sampled_image uploads. */
    PlaneGroup<1> sdVar{"the sample variances"};
    PlaneGroup<1> sdErr{"the noise estimate's image"};
    PlaneGroup<2> sdAQ{"the accumulator and squares planes of an image call"};
    PlaneGroup<3> sdIn{"surf_denoise_sampled_image's planes"};
    StageTimer<kDenoiseMaxIterations + 1> sdTime;   /* the level-0 kernel, then the iterations of the last run (surf_debug_sampled_time) */
    /* the instance records as last uploaded (surf_upload_scene, surf_update_instances): their transforms move the history */
    std::vector<surf_gpu_instance> instHost;
    /* one-frame render calls may leave up to a pool of their stream unissued
     * (SURF_LOOP_LAG=0: issue each call's frame before returning) */
    bool loopLag = true;
    /* occupancy probes: extra dynamic LDS per k_extend / k_connect workgroup (SURF_EXT_LDS_PAD / SURF_CON_LDS_PAD bytes) */
    size_t extLdsPad = 0, conLdsPad = 0;
    /* k_connect stages the emitters' BLAS node records in LDS when they are
     * few and every BLAS node index fits 16 bits (SURF_LDS_LIGHTBLAS=0: never) */
    bool ldsLightBlas = true;
    /* small BLASes in the compact form k_connect stages (blasAnyStaged): BLAS
     * node offset -> interior records on the device, their count, index offset, triangle slots */
    struct StagedBlas { const float4* rec; uint32_t recN, tri0, triN; };
    std::map<uint32_t, StagedBlas> stagedBlas;
    uint32_t permA = 0, permFrames = 0;
    std::vector<uint32_t> heavyInst;
    /* pool ray-order key (SURF_KEY): 2 heavy-instance mask x quadrant, most
     * heavy instances first (the default: the costliest rays are dealt to the
     * first-dispatched workgroups, DESIGN 4 "Pool sizing"), 1 the same key
     * ascending, 0 start instance x quadrant */
    uint32_t keyMode = 2;
    /* the lane walk takes a single-leaf TLAS's leaf runs (the room's planes) per
     * lane (DevScene::runHead, leafRun; SURF_LEAF_RUN=0: the wave-uniform loop
     * takes every instance) */
    bool leafRun = true;
    /* camera */
    bool hasCamera = false;
    DevCamera cam{};
    surf_camera_ubo camUbo{};

    /* wavefront state */
    bool allocated = false;
    Pool pool[2]{};
    float4* hitTUV = nullptr;
    uint32_t* hitInst = nullptr;
    ShadowQ Q{};
    float4* rad = nullptr;
    float4* acc = nullptr;
    /* the per-sample second moments beside the accumulator (surf_set_sample_squares):
     * npx records (sum r.x^2, sum r.y^2, sum r.z^2, sum lum(r)^2), allocated when
     * first switched on, kept when switched off, freed in surf_destroy */
    float4* sq = nullptr;
    bool sqOn = false;
    /* the sample buckets beside the accumulator (surf_set_sample_buckets): bkM
     * planes of npx records (sum r.x, sum r.y, sum r.z, samples), bucket-major,
     * bkM = 0: off; bkPlanes of them allocated -- when first switched on or to a
     * larger M, kept when switched off or to a smaller one, freed in surf_destroy */
    float4* bk = nullptr;
    uint32_t bkM = 0, bkPlanes = 0;
    /* the robust estimate (surf_robust_*, host/robust.hip): rbOut, the output
     * plane; rbTrim, the striped trimmed-pixel counters (4 KB) and behind them
     * the trim image (1 B per pixel); rbIn, the accumulator and the M bucket
     * planes surf_robust_image uploads (one allocation of (1 + M) * npx records) */
    PlaneGroup<1> rbOut{"the robust estimate's image"};
    PlaneGroup<1> rbTrim{"the robust estimate's trim image"};
    PlaneGroup<1> rbIn{"surf_robust_image's planes"};
    StageTimer<1> rbTime;          /* the last k_robust launch (surf_debug_robust_time) */
    /* the stills filters on the sample buckets' halves (host/nlm.hip's driver).  nl: the two half planes (summed from the
     * buckets or uploaded), the three prepared records (c0 + validity, c1 and V packed), then the output and its error
     * estimate -- one set for both filters.  Their lifetime: a result in nl is good until the next stills filter runs on
     * the context.  Every public entry copies its results out before it returns, and the mask built from the filter's
     * planes (host/error_mask.hip) consumes them before anything else runs.
     * The dual-buffer non-local-means filter (surf_denoise_nlm*, host/nlm.hip): nlStaged: the filter kernel stages its
     * tile in LDS where the layout fits (SURF_NLM_LDS=0: every value from global memory; MEASUREMENTS "Non-local means") */
    PlaneGroup<7> nl{"the non-local-means filter's planes"};
    StageTimer<3> nlTime;          /* halves, prepare, filter of the last run (surf_debug_nlm_time) */
    bool nlStaged = true;
    /* the first-order feature regression filter (surf_denoise_regress*, host/regress.hip): rgIn, the three feature planes
     * the image form uploads; rgStaged: the filter kernel stages its tile in LDS where the layout fits (SURF_REGRESS_LDS=0:
     * every value from global memory; MEASUREMENTS "First-order regression"); rgLdsSet: the staged kernel's dynamic LDS
     * limit has been raised */
    PlaneGroup<3> rgIn{"the regression filter's planes"};
    StageTimer<3> rgTime;          /* halves, prepare, filter of the last run (surf_debug_regress_time) */
    bool rgStaged = true;
    bool rgLdsSet = false;
    /* the mask from the non-local-means filter's error estimate (surf_error_mask_image, surf_mask_from_nlm, surf_render_adaptive_nlm;
     * host/error_mask.hip): em, one record, the loop's summary counters; emIn, the three planes the image form uploads */
    PlaneGroup<1> em{"the error mask's counters"};
    PlaneGroup<3> emIn{"surf_error_mask_image's planes"};
    StageTimer<2> emTime;          /* mask kernel, compaction of the last run (surf_debug_error_mask_time) */
    /* the display stage (surf_display*, host/display.hip): dpRec, the meter record's copies; dpTable: this context has
     * queued the copy of the sRGB table to its device's constant memory; dpIn, the plane surf_display_image uploads; dpHh, the bloom's horizontal pass
     * (allocated only with bloom on); dpOut, the RGBA8 words (4 B per pixel) of the forms that copy to the host */
    PlaneGroup<1> dpRec{"the display stage's meter record"};
    bool dpTable = false;
    PlaneGroup<1> dpIn{"surf_display_image's plane"};
    PlaneGroup<1> dpHh{"the bloom's plane"};
    PlaneGroup<1> dpOut{"the display stage's words"};
    StageTimer<4> dpTime;          /* meter, scale, blur, pack of the last run (surf_debug_display_time) */
    /* the light-map atlas (surf_atlas_*, host/atlas.hip) keeps no buffer on the context: atlasTileMap, the cover kernel's
     * work mapping (SURF_ATLAS_MAP: 1 one wave per (triangle, 8 x 8 tile), 0 one lane per triangle; the planes are the same);
     * atTiles: the last build ran the tile mapping */
    bool atlasTileMap = true;
    bool atTiles = false;
    StageTimer<5> atTime;          /* setup + scan, cover, resolve of the last build; the last finish; the last dilate (surf_debug_atlas_time) */
    /* the active-pixel mask (surf_set_pixel_mask, surf_mask_from_noise; host/adaptive.hip):
     * pmOn: a mask that leaves some pixel out is set (an all-ones mask is "no
     * mask"); then pmMask holds its npx bytes, pmList the pmActive ascending
     * local pixels a masked stream issues and accumulates, pmBlk the
     * compaction's per-block counts.  Allocated on first use, kept, freed in
     * surf_destroy.  adImg*: the same three buffers for surf_adaptive_mask_image's
     * frame, grown when a larger one arrives. */
    bool pmOn = false;
    uint32_t pmActive = 0;
    uint8_t* pmMask = nullptr;
    uint32_t* pmList = nullptr;
    uint32_t* pmBlk = nullptr;
    uint8_t* adImgMask = nullptr;
    uint32_t* adImgList = nullptr;
    uint32_t* adImgBlk = nullptr;
    size_t adImgCap = 0;
    /* the surfel sensor (surf_set_surfel_sensor*; surf_hip.hip): ssOn: samples start at the caller's texels, not at the
     * camera -- the stream's kernels are the SURFEL instantiations (sensorKernels) and take surfelGeom's argument.  ssPlanes:
     * the library's copies of the two planes (position, normal: npx records each), allocated on first use, kept when the
     * sensor is cleared, freed in surf_destroy.  ssValidDev / ssValidHost: a byte per texel, 1 where its normal is not
     * (0, 0, 0), ssValid of them: every mask set or built on the context is ANDed with it before its compaction, and while
     * ssValid < npx "no mask" is the validity mask itself (resetSensorMask). */
    bool ssOn = false;
    PlaneGroup<2> ssPlanes{"the surfel sensor's planes"};
    uint8_t* ssValidDev = nullptr;
    std::vector<uint8_t> ssValidHost;
    uint32_t ssValid = 0;
    hipEvent_t accEv[2] = {};      /* profiling: around each k_accumulate launch (surf_stats.ms_accum), created on first use */
    uint32_t* dRows = nullptr;
    Counters* ctr = nullptr;
    Counters* hctr = nullptr;      /* pinned: the counters as of the last consumed snapshot */
    uint32_t* frameDone = nullptr; /* [kStripes][window] completions per frame slot */
    /* host snapshots of the counters and of the open passes' completion
     * stripes, each taken after a graph replay; a lagged one-frame call may
     * return with up to kSnaps of them (and their replays) in flight, so the
     * GPU keeps working while the application runs its loop (pump) */
    struct Snap { Counters* h = nullptr; uint32_t* fd = nullptr; uint64_t acc = 0, open = 0; int phases = 0; hipEvent_t ev = nullptr; };
    static constexpr int kSnaps = 2;
    Snap snap[kSnaps];
    int snapHead = 0, snapCount = 0;
    uint64_t issuePerPhase = 0;    /* chains a phase issued in the last unstarved snapshot of this stream: what the replays in flight will issue */
    bool pipeline = true;          /* SURF_PIPELINE=0: every replay waited for before the next (and before a call returns) */
    /* issue limits pushed to the device: a ring of pinned sources, so a later
     * push never rewrites the bytes an earlier, still queued copy reads */
    static constexpr uint32_t kLimitRing = 16;
    uint64_t* hLimit = nullptr;
    uint32_t hLimitNext = 0;
    /* device time of calls that return with replays in flight: two event
     * pairs used in turn, read once their end has passed */
    hipEvent_t tev[2][2] = {};
    bool tevPending[2] = {false, false};
    int tevCur = 0;
    uint32_t* dOutRGBA = nullptr;
    std::vector<void*> wfAllocs;
    uint64_t totalSamples = 0;     /* frames rendered since the last clear (samples per pixel) */

    /* sample stream: targetFrames frames of spp samples per pixel requested,
     * i.e. passes (samples per pixel) [0, targetFrames * spp) after the
     * baseFrame samples rendered before the stream; pass q lives in radiance
     * slot q % window (window a multiple of spp) */
    bool streamActive = false;
    uint64_t baseFrame = 0;        /* sample count before the stream (the reference's totalSamples) */
    uint64_t targetFrames = 0;     /* frames requested (chains per pixel) */
    uint64_t accPasses = 0;        /* passes accumulated (in order) */
    uint32_t spp = 1;              /* samples per frame of the stream (a frame's samples chain their RNG state) */
    /* the stream's chains per frame: npx, or the active list's length for a
     * stream opened under a mask (streamMasked: its graphs issue through
     * k_regen<true>, its frames are accumulated by k_accumulate_list) */
    uint32_t streamPx = 0;
    bool streamMasked = false;
    uint32_t streamMaxSeg = 0;
    int zeroCutoff = -1;           /* early end of paths with throughput < FLT_MIN: 1 on, 0 off, -1 automatic (on for 1-sample frames) */
    uint64_t pushedLimit = 0;
    uint32_t tailPaths = 0;        /* drain policy (surf_set_tail_policy), 0 = automatic */
    uint32_t tailBudget = 16;      /* per-stage segment budget of the drain tail (0 = one stage); 16: measured fastest */
    Pool surv[2]{};                /* drain survivors, ping-pong between stages */
    uint32_t survCap = 0;
    uint32_t coopMax = 0;          /* survivors handled by the cooperative tail (one path per wave) */
    uint32_t coopAll = 150000;     /* drain paths left to the cooperative tail (surf_set_tail_coop); C3 drain 176-184 ms at 60000, 172-178 at 150000 */
    int drainReplays = 1;          /* graph replays per host poll while draining (SURF_DRAIN_REPLAYS) */
    bool drainShort = false;       /* short replays once nothing is left to issue (SURF_DRAIN_SHORT=1; measured slower, MEASUREMENTS round 5) */
    bool regenFirst = false;       /* k_regen before the connect fork (SURF_REGEN_FIRST=1; measured equal, MEASUREMENTS round 5) */
    int traceMode = 0;             /* surf_trace_closest/_any: 0 one ray per lane, 1 one ray per wave */
    bool connectStaged = false;    /* the last k_connect launched walked the emitters' BLAS from LDS (surf_debug_connect_staging) */
    bool tailPair = true;          /* cooperative drain on k_tail_pair (partner waves trace the shadow rays; SURF_TAIL_PAIR=0: k_tail_coop) */
    uint32_t cus = 256;            /* compute units of the device */
    bool sortRays = true;          /* order each phase's rays by start instance (SURF_SORT=0: off) */
    bool sortPool = true;
    bool sortShadow = true;        /* ... and the shadow queue by light (SURF_SORT=2: pool only, 3: shadow queue only) */
    uint32_t shKey = 1;            /* the shadow key's layout (shadowKey): 0 = 16 bins, 1 = 32 (default), 2 = 40 (SURF_SH_KEY) */
    uint32_t shRegion = 0;         /* slots per shadow-queue region, 0: by the pool and the layout (SURF_SH_REGION, tests) */
    /* ray order: counts from k_regen_count (or k_bincount), then k_binscatter each phase */
    uint32_t* order = nullptr;
    uint32_t* binHist = nullptr;
    /* connect overlapped with the next phase's regen / pool sort / extend
     * (SURF_OVERLAP=0: one stream): its own stream in the graph capture, its
     * own shadow order and histograms */
    bool overlap = true;
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> capEv;   /* two per phase of a full replay (sized by createCtx) */
    uint32_t tailLanes = 0;
    uint32_t segMaxBase = 0;       /* longest path of finished streams */
    uint64_t tailFirstRays = 0;    /* first extension rays of drained paths: counted by regen, traced by the tail */

    /* graph */
    hipGraphExec_t graphExec = nullptr, graphExecShort = nullptr;
    hipGraph_t graph = nullptr, graphShort = nullptr;
    /* the same two graphs captured for masked streams (k_regen<true> over pmList; built when first needed) */
    hipGraphExec_t graphExecM = nullptr, graphExecShortM = nullptr;
    hipGraph_t graphM = nullptr, graphShortM = nullptr;
    uint32_t gridWork = 0, gridRegen = 0, gridExtend = 0, gridConnect = 0;

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> pev;   /* profiling: kPhaseEvents per phase of a full replay + the end (sized by createCtx) */
    uint32_t* hPhaseN = nullptr;   /* profiling + SURF_PHASE_LOG: paths each phase extends (pinned) */
    FILE* phaseLog = nullptr;      /* SURF_PHASE_LOG=<file>: one line per profiled phase (size, kernel ms) */
    surf_stats stats{};
    unsigned long long evBase[kEvents] = {};   /* event counts of finished streams since the last clear */
};

/* the helpers, and what one host translation unit of the library defines for
 * the others (a namespace of their own: the library's C++ symbols stay clear
 * of an application's) */
namespace surfhost {
/* the last error of any context, for surf_last_error(NULL) */
void setGlobalError(const std::string& e);
/* defined beside the sample stream (surf_hip.hip): whatever replaces scene
 * tables first ends the stream that reads them and drops the captured graphs,
 * whose kernel arguments carry the scene descriptor */
int endStream(surf_ctx* c);
void destroyGraph(surf_ctx* c);
/* ... and for the image-space filters (the .hip files of host/) what a read of the context
 * needs: the sample stream drained, the cached feature planes computed (c->aov.p) */
int drainStream(surf_ctx* c);
int featurePlanes(surf_ctx* c);
/* ... and for the two purely spatial context filters the planes surf_set_filter_guides chose,
 * computed: *planes is the planes of c->aov, c->aovChain or c->aovSampled (whose first three
 * planes are laid out as theirs) */
int guidePlanes(surf_ctx* c, void* const** planes);
/* What follows the camera, the scene and the instances: the pixel classes of the issue order
 * and the cached planes of every plane pass.  Whatever changes one of the three calls this. */
inline void dropDerivedPlanes(surf_ctx* c) {
    c->permValid = false;
    for (PassPlanes* pp : {&c->aov, &c->aovChain, &c->aovSampled, &c->ao}) pp->valid = false;
}
/* defined in host/denoise.hip: PlaneGroup::grow's body -- `count` images of at
 * least npx records each (OOM message: "... of <what> ...") */
int growImages(surf_ctx* c, float4** planes, int count, size_t& cap, size_t npx, const char* what);
/* defined in host/denoise.hip: surf_destroy's part for the denoiser's state */
void freeDenoise(surf_ctx* c);
/* defined in host/temporal.hip: surf_destroy's part for the temporal state */
void freeTemporal(surf_ctx* c);
/* defined in host/svgf.hip: freeTemporal's part for the state of the variance-guided
 * filter, the firefly clamp, the sample-variance-guided filter and the noise estimate */
void freeSvgf(surf_ctx* c);
/* defined in host/adaptive.hip: surf_destroy's part for the mask's buffers */
void freeAdaptive(surf_ctx* c);
/* defined in host/adaptive.hip, for whatever sets the context's mask back to "every pixel": under a surfel sensor with
 * invalid texels that is the validity mask (bytes, list, count), else no mask at all.  Waits for its copies. */
int resetSensorMask(surf_ctx* c);
/* defined in host/robust.hip: surf_destroy's part for the robust estimate's images */
void freeRobust(surf_ctx* c);
/* defined in host/nlm.hip: surf_destroy's part for the stills filters' images */
void freeNlm(surf_ctx* c);
/* defined in host/regress.hip: surf_destroy's part for the regression filter's uploaded planes */
void freeRegress(surf_ctx* c);
/* defined in host/error_mask.hip: surf_destroy's part for the error mask's images */
void freeErrorMask(surf_ctx* c);
/* defined in host/display.hip: surf_destroy's part for the display stage's images */
void freeDisplay(surf_ctx* c);
/* defined in host/atlas.hip: surf_destroy's part for the atlas stage's timer */
void freeAtlas(surf_ctx* c);

#define SURF_CHECK(ctx, call)                                                             \
    do {                                                                                  \
        hipError_t e_ = (call);                                                           \
        if (e_ != hipSuccess) {                                                           \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);               \
            setGlobalError((ctx)->err);                                                   \
            return SURF_ERR_HIP;                                                          \
        }                                                                                 \
    } while (0)

inline int fail(surf_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    setGlobalError(msg);
    return code;
}

template <class T>
int devAlloc(surf_ctx* c, std::vector<void*>& list, T** out, size_t count) {
    *out = nullptr;
    if (count == 0) count = 1;
    void* p = nullptr;
    if (hipMalloc(&p, count * sizeof(T)) != hipSuccess || !p) {
        return fail(c, SURF_ERR_OOM, "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes failed");
    }
    list.push_back(p);
    *out = static_cast<T*>(p);
    return SURF_OK;
}

inline void freeList(std::vector<void*>& list) {
    for (void* p : list) (void)hipFree(p);
    list.clear();
}

template <class T>
int upload(surf_ctx* c, const std::vector<T>& host, const T** devOut) {
    T* d = nullptr;
    int rc = devAlloc(c, c->sceneAllocs, &d, host.size());
    if (rc) return rc;
    if (!host.empty()) SURF_CHECK(c, hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    *devOut = d;
    return SURF_OK;
}

}  // namespace surfhost
using namespace surfhost;

template <int N>
int PlaneGroup<N>::grow(surf_ctx* c, size_t npx) { return growImages(c, p, N, cap, npx, what); }
