/*
 * filter_host.h -- internal: what the image-space filters (host/denoise.hip,
 * temporal.hip, svgf.hip, adaptive.hip, nlm.hip, regress.hip, error_mask.hip) share: the
 * fixed-sigma denoiser's entry points for the other filters, the one driver of the
 * stills filters on the sample buckets' halves with its CPU twin, the non-local-means
 * filter's context run for the mask built from it, the one driver of the a-trous
 * iterations on the device, and the host twins' copy of a caller's plane.  Includes no
 * kernel: a driver is handed the launch of what it drives.
 */
#pragma once
#include "host/surf_ctx.h"

#include <algorithm>
#include <cstring>
#include <functional>

#include "device/denoise_kernels.h"

namespace surfdev { struct NlmConsts; struct NlmSums; struct NlmFetchPlanes; }   /* device/nlm_kernels.h */

namespace surfhost {
/* defined in host/denoise.hip: NULL when the parameters are valid, else what is
 * wrong with them; and the fixed-sigma filter on device planes of a full w x h
 * frame (*result: the scratch image holding the output, valid until the next
 * a-trous run).  Waits for the result. */
const char* denoiseParamsError(const surf_denoise_params* p);
int denoisePlanes(surf_ctx* c, uint32_t w, uint32_t h, const float4* acc, const float4* pos, const float4* nrm, const float4* alb,
                  const surf_denoise_params& P, const float4** result);

/* the grid of 32 x 8 pixel tiles covering a w x h frame */
inline dim3 tileGrid(uint32_t w, uint32_t h) { return dim3((w + kDenoiseTileW - 1) / kDenoiseTileW, (h + kDenoiseTileH - 1) / kDenoiseTileH); }

/* The stills filters -- those that weight the sample buckets' two half images
 * against each other (host/nlm.hip, host/regress.hip) -- have one driver,
 * runStills, defined in host/nlm.hip beside the halves and prepare kernels it
 * launches.  What an entry point tells it: */
struct StillsCall {
    const char* who;                /* the entry point, for a message */
    uint32_t w, h;                  /* the image form: the frame and its two halves on the host; */
    const float *half0, *half1;     /* half0 NULL: the context form, the context's frame and buckets */
    void *out, *outErr;             /* where the two results are copied (outErr may be NULL); out NULL: nowhere */
    hipMemcpyKind kind;
    const char* paramsWhy;          /* what is wrong with the parameters (NULL: nothing), reported where the entry points always did */
    const char* shardAdvice;        /* how the row-shard refusal of the context form ends */
    const char* planesWhat;         /* names c->nl in an out-of-memory message */
    std::function<int()> ready;     /* whatever else the filter reads, put in place after the checks and before the clock starts */
};
/* ... and what it hands the launch of the filter kernel: the grid, the prepared
 * records, the halves, the two result planes, the frame */
struct StillsStep {
    dim3 grid;
    const float4 *C0, *C1, *V, *H0, *H1;
    float4 *out, *err;
    int W, H;
};
/* The checks (parameters, and for the context form buckets on and every row
 * owned; for the image form the frame), the stream drained and the halves of
 * the context's buckets, or the host halves uploaded; prepare; launch(step),
 * which queues the filter kernel; the results copied as the call says.  T's
 * stages: halves (empty for the image form), prepare, filter.  *dOut, *dErr,
 * where asked for: the two result planes on the device.  Waits. */
int runStills(surf_ctx* c, const StillsCall& call, StageTimer<3>& T, const std::function<int(const StillsStep&)>& launch,
              const float4** dOut = nullptr, const float4** dErr = nullptr);
/* what is wrong with an image form's or a host twin's frame and parameters, or NULL */
const char* stillsImageError(uint32_t w, uint32_t h, const char* paramsWhy);
/* The CPU twin of runStills on a checked frame: nlmPrepare over the frame, then
 * per valid pixel pixel(x, y, prepared records), and nlmOutput. */
void stillsTwin(uint32_t w, uint32_t h, const float* half0, const float* half1,
                const std::function<NlmSums(int, int, const NlmFetchPlanes&)>& pixel, float* out, float* outErr);

/* defined in host/nlm.hip: NULL when the parameters are valid, else what is
 * wrong with them; the host constants; and the context form's run without its
 * copies (`who` names the caller in a message).  *out and *err: the scratch
 * images holding the two results, valid until the next stills filter runs on
 * the context (c->nl).  Waits for them. */
const char* nlmParamsError(const surf_nlm_params* p);
NlmConsts nlmConsts(const surf_nlm_params& p);
int nlmContextPlanes(surf_ctx* c, const surf_nlm_params* p, const char* who, const float4** out, const float4** err);

/* what the driver hands the launch of iteration i: the step, whether the tile
 * is staged and the dynamic LDS that takes, the grid, the level read and the
 * level written, and whether this is the last iteration */
struct AtrousStep {
    uint32_t i;
    int s;
    bool staged;
    size_t lds;
    dim3 grid;
    const float4* in;
    float4* out;
    int last;
};

/* Iterations 0 .. n-1 of an a-trous filter over the scratch c->dn, level 0 in
 * dn[0], the levels used in turn: step 2^i, staged up to the step the context
 * allows (SURF_DENOISE_LDS, at most kDenoiseMaxStagedStep) with the tile and
 * its 2 s halo in LDS as three float4 planes.  launch(step) queues the kernel
 * of one iteration; the end of iteration i is event firstStage + i + 1 of T,
 * whose earlier events the caller marked.  Waits for the last iteration, reads
 * the times; *result is the level that holds the output. */
template <int N, class Launch>
int runAtrous(surf_ctx* c, uint32_t w, uint32_t h, uint32_t n, StageTimer<N>& T, int firstStage, const Launch& launch,
              const float4** result) {
    const uint32_t stagedMax = std::min<uint32_t>(c->dnLdsMax, (uint32_t)kDenoiseMaxStagedStep);
    AtrousStep st;
    st.grid = tileGrid(w, h);
    for (st.i = 0; st.i < n; ++st.i) {
        st.s = 1 << st.i;
        st.staged = (uint32_t)st.s <= stagedMax;
        st.lds = st.staged ? (size_t)3 * sizeof(float4) * (kDenoiseTileW + 4 * st.s) * (kDenoiseTileH + 4 * st.s) : 0;
        st.in = c->dn[st.i & 1];
        st.out = c->dn[(st.i & 1) ^ 1];
        st.last = st.i + 1 == n;
        launch(st);
        SURF_CHECK(c, hipGetLastError());
        SURF_CHECK(c, T.mark(firstStage + (int)st.i + 1, c->stream));
    }
    SURF_CHECK(c, T.collect(firstStage + (int)n));
    *result = c->dn[n & 1];
    return SURF_OK;
}

/* a host twin's copy of a caller's plane of npx 16-byte records, which need not
 * be 16-byte aligned as float4 is; NULL: an empty plane */
inline std::vector<float4> hostPlane(const float* src, size_t npx) {
    std::vector<float4> v(src ? npx : 0);
    if (src) std::memcpy(v.data(), src, npx * sizeof(float4));
    return v;
}
}  // namespace surfhost
