/*
 * filter_host.h -- internal: what the image-space filters (host/denoise.hip,
 * temporal.hip, svgf.hip, adaptive.hip, nlm.hip, regress.hip, error_mask.hip) share: the
 * fixed-sigma denoiser's entry points for the other filters, the non-local-means
 * filter's context run for the mask built from it, the one driver of the a-trous
 * iterations on the device, and the host twins' copy of a caller's plane.  Includes no
 * kernel: the driver is handed the launch of an iteration.
 */
#pragma once
#include "host/surf_ctx.h"

#include <algorithm>
#include <cstring>

#include "device/denoise_kernels.h"

namespace surfhost {
/* defined in host/denoise.hip: NULL when the parameters are valid, else what is
 * wrong with them; and the fixed-sigma filter on device planes of a full w x h
 * frame (*result: the scratch image holding the output, valid until the next
 * a-trous run).  Waits for the result. */
const char* denoiseParamsError(const surf_denoise_params* p);
int denoisePlanes(surf_ctx* c, uint32_t w, uint32_t h, const float4* acc, const float4* pos, const float4* nrm, const float4* alb,
                  const surf_denoise_params& P, const float4** result);

/* defined in host/nlm.hip: NULL when the parameters are valid, else what is
 * wrong with them; and the context form's run without its copies -- the checks
 * (`who` names the caller in a message), the drain, the halves of the context's
 * buckets, prepare and filter.  *out and *err: the scratch images holding the
 * two results, valid until the next non-local-means run.  Waits for them. */
const char* nlmParamsError(const surf_nlm_params* p);
int nlmContextPlanes(surf_ctx* c, const surf_nlm_params* p, const char* who, const float4** out, const float4** err);

/* the grid of 32 x 8 pixel tiles covering a w x h frame */
inline dim3 tileGrid(uint32_t w, uint32_t h) { return dim3((w + kDenoiseTileW - 1) / kDenoiseTileW, (h + kDenoiseTileH - 1) / kDenoiseTileH); }

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
