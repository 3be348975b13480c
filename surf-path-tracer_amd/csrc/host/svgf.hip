/*
 * svgf.hip -- the variance-guided filter (surf_svgf*, include/surf_hip.h):
 * parameter checks, the launches of one frame -- the firefly clamp where it
 * is asked for, k_temporal with the moments switched on, the guides and the
 * variance estimate, the variance-guided a-trous iterations (the first of
 * them storing the history where feedback is on) -- the moments a frame
 * leaves on the context beside the temporal state, and the CPU twins.  The
 * arithmetic lives in device/temporal_kernels.h and device/svgf_kernels.h.
 *
 * The file is the one home of k_atrous_var, so it also holds the two readers
 * of the per-sample squares plane, which run the same iterations or none: the
 * sample-variance-guided filter (surf_denoise_sampled*) and the noise estimate
 * (surf_noise_*), their arithmetic in device/sampled_kernels.h.  A file of
 * their own would instantiate k_atrous_var a second time.
 */
#include "host/filter_host.h"
#include "host/temporal_host.h"

#include <cmath>

#include "device/svgf_kernels.h"
#include "device/sampled_kernels.h"

namespace {

/* needSpatial: spatial_below is checked (surf_denoise_sampled* ignores the field) */
const char* svgfParamError(const surf_svgf_params* p, bool needSpatial = true) {
    if (!p) return "svgf params is NULL";
    if (p->iterations < 1 || p->iterations > (uint32_t)kDenoiseMaxIterations) return "iterations outside 1..6";
    for (float s : {p->sigma_lum, p->sigma_normal, p->sigma_plane})
        if (!(std::isfinite(s) && s > 0.0f)) return "a sigma is not finite and > 0";
    if (needSpatial && p->spatial_below == 0) return "spatial_below is 0";
    if (!(std::isfinite(p->variance_eps) && p->variance_eps > 0.0f)) return "variance_eps is not finite and > 0";
    return nullptr;
}

/* the extensions: NULL is all zero */
const char* svgfExtError(const surf_svgf_ext* x) {
    if (!x) return nullptr;
    if (!(x->firefly_scale == 0.0f || (std::isfinite(x->firefly_scale) && x->firefly_scale >= 1.0f))) return "firefly_scale is neither 0 nor finite and >= 1";
    if (x->feedback > 1u) return "feedback is neither 0 nor 1";
    return nullptr;
}
surf_svgf_ext svgfExt(const surf_svgf_ext* x) { return x ? *x : surf_svgf_ext{}; }

/* the constants of a call, computed in f32 on the host as the header states */
SvgfConsts svgfConsts(const surf_svgf_params& p) {
    SvgfConsts k;
    k.kn = 1.0f / (p.sigma_normal * p.sigma_normal);
    k.kp = 1.0f / (p.sigma_plane * p.sigma_plane);
    k.sigmaLum = p.sigma_lum;
    k.varEps = p.variance_eps;
    k.spatialBelow = (float)p.spatial_below;
    return k;
}

/* Kernel selection: k_svgf_variance<STAGED> with its dynamic LDS, and
 * k_atrous_var<STAGED, FEEDBACK> for a step of the a-trous driver
 * (host/filter_host.h), which decides STAGED and the LDS.  FEEDBACK is picked
 * for iteration 0 of a run with surf_svgf_ext.feedback and for no other
 * launch.  k_firefly has one instantiation and static LDS (kFireflyLdsBytes,
 * device/svgf_kernels.h); k_sampled_level0 and the noise estimate's k_noise
 * (device/sampled_kernels.h) have one each and no LDS. */
template <class F>
struct Launch { F fn; size_t lds; };
auto varianceKernel(bool staged) {
    return Launch<decltype(&k_svgf_variance<true>)>{staged ? k_svgf_variance<true> : k_svgf_variance<false>, staged ? kSvgfVarLdsBytes : 0};
}

/* The variance-guided a-trous iterations of both filters over the scratch
 * c->dn (level 0 in dn[0], the guides in dn[2] and dn[3]); var1 takes the
 * variance leaving the filter, hist (not NULL: feedback) the history that
 * iteration 0 rewrites.  T's events up to firstStage are the caller's. */
template <int N>
int runAtrousVar(surf_ctx* c, uint32_t w, uint32_t h, const surf_svgf_params& P, const float4* alb, float* var1, float4* hist,
                 StageTimer<N>& T, int firstStage, const float4** result) {
    const SvgfConsts S = svgfConsts(P);
    const uint32_t demod = P.demodulate ? 1u : 0u;
    const float4* gN = c->dn[2];
    const float4* gP = c->dn[3];
    return runAtrous(c, w, h, P.iterations, T, firstStage, [&](const AtrousStep& st) {
        const bool feedback = hist && st.i == 0;
        const auto fn = feedback ? (st.staged ? k_atrous_var<true, true> : k_atrous_var<false, true>)
                                 : (st.staged ? k_atrous_var<true, false> : k_atrous_var<false, false>);
        hipLaunchKernelGGL(fn, st.grid, dim3(256), st.lds, c->stream, st.in, gN, gP, alb, st.out, var1, (int)w, (int)h, st.s, S, demod,
                           st.last, feedback ? hist : (float4*)nullptr);
    }, result);
}

/* the device planes of one frame: the current frame's, the previous frame's
 * (NULL with K.havePrev 0; pM NULL: no moments stored) and what is written */
struct SvgfPlanes {
    const float4 *A, *P, *N, *alb;
    const uint4* ID;
    const float4 *pH, *pP;
    const TemporalGuide* pG;
    const float4* pM;
    float4 *blend, *hist, *gP;
    TemporalGuide* gN;
    float4* outM;
    float* var;                  /* 2 * npx floats: the variance entering the filter, then leaving it */
    float4* clamped;             /* A' of the firefly clamp; read in A's place when the clamp is on */
};

/* k_firefly over device planes of a full w x h frame, timed (c->ffTime; fireflyTime reads it once the launch has ended) */
int launchFirefly(surf_ctx* c, uint32_t w, uint32_t h, const float4* A, const float4* alb, float scale, uint32_t demod, float4* out) {
    SURF_CHECK(c, c->ffTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_firefly, tileGrid(w, h), dim3(256), 0, c->stream, A, alb, out, (int)w, (int)h, scale, demod);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->ffTime.mark(1, c->stream));
    return SURF_OK;
}
int fireflyTime(surf_ctx* c) {
    SURF_CHECK(c, c->ffTime.collect(1));
    return SURF_OK;
}

/* All launches of a frame on the context's stream over device planes of a
 * full w x h frame; *result is the scratch image that holds the output.
 * Waits for the result. */
int runSvgf(surf_ctx* c, uint32_t w, uint32_t h, const SvgfPlanes& pl, const TemporalConsts& K, const surf_svgf_params& P,
            const surf_svgf_ext& X, const float4** result) {
    const size_t npx = (size_t)w * h;
    int rc = c->dn.grow(c, npx);
    if (rc) return rc;
    if ((rc = temporalMotionUpload(c, K))) return rc;
    const uint32_t demod = P.demodulate ? 1u : 0u;
    float4* gN = c->dn[2];
    float4* gP = c->dn[3];
    const dim3 grid = tileGrid(w, h);
    static_assert(kDenoiseTileW == kTemporalTileW && kDenoiseTileH == kTemporalTileH, "one grid for every kernel of the frame");
    const bool clamp = X.firefly_scale > 0.0f;
    if (clamp && (rc = launchFirefly(c, w, h, pl.A, pl.alb, X.firefly_scale, demod, pl.clamped))) return rc;
    const float4* A = clamp ? pl.clamped : pl.A;
    SURF_CHECK(c, c->svTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_temporal<true>, grid, dim3(256), 0, c->stream, A, pl.P, pl.N, pl.ID, pl.pH, pl.pP, pl.pG, (const float*)c->tpMotion, K,
                       (int)w, (int)h, pl.blend, pl.hist, pl.gP, pl.gN, TemporalMomentPlanes{pl.alb, pl.pM, pl.outM, demod});
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->svTime.mark(1, c->stream));
    hipLaunchKernelGGL(k_svgf_guides, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, pl.P, pl.N, pl.alb, (uint32_t)npx, gN, gP);
    SURF_CHECK(c, hipGetLastError());
    const auto variance = varianceKernel(c->svVarStaged);
    hipLaunchKernelGGL(variance.fn, grid, dim3(256), variance.lds, c->stream, (const float4*)pl.blend, pl.alb, (const float4*)gN, (const float4*)gP,
                       (const float4*)pl.outM, c->dn[0], pl.var, (int)w, (int)h, svgfConsts(P), demod);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->svTime.mark(2, c->stream));
    if ((rc = runAtrousVar(c, w, h, P, pl.alb, pl.var + npx, X.feedback != 0u ? pl.hist : nullptr, c->svTime, 2, result))) return rc;
    return clamp ? fireflyTime(c) : SURF_OK;
}

/* surf_svgf_accumulate / _copy_device: the context's own accumulator and
 * cached feature planes against the stored state, which this frame's replaces */
int svgfContext(surf_ctx* c, const surf_temporal_params* p, const surf_svgf_params* sp, const surf_svgf_ext* ext, void* dst,
                hipMemcpyKind kind) {
    if (!c || !dst) return SURF_ERR_INVALID;
    if (const char* why = temporalParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_accumulate: ") + why);
    if (const char* why = svgfParamError(sp)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_accumulate: ") + why);
    if (const char* why = svgfExtError(ext)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_accumulate: ") + why);
    const surf_svgf_ext X = svgfExt(ext);
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_svgf_accumulate needs a context that owns every row of the frame: a reprojected pixel and "
                                         "a spatial filter read other rows; assemble the shards' accumulators and feature planes and call "
                                         "surf_svgf_image");
    int rc = featurePlanes(c);
    if (rc) return rc;
    if ((rc = drainStream(c))) return rc;
    if ((rc = c->tp.grow(c, c->npx))) { c->tpHave = false; return rc; }
    if ((rc = c->sv.grow(c, c->npx))) { c->svHave = false; return rc; }
    if (X.firefly_scale > 0.0f && (rc = c->ff.grow(c, c->npx))) return rc;
    const bool have = c->tpHave && c->tpInst.size() == c->instHost.size();
    const uint32_t nInst = (uint32_t)c->instHost.size();
    const TemporalConsts K = temporalSetup(*p, have ? &c->tpCam : nullptr, c->instHost.data(), have ? c->tpInst.data() : nullptr, nInst,
                                           c->tpMotionHost);
    float4* const* prev = c->tp.p + 3 * c->tpCur;
    float4* const* next = c->tp.p + 3 * (c->tpCur ^ 1);
    SvgfPlanes pl{};
    pl.A = c->acc;
    pl.P = static_cast<const float4*>(c->aov.p[SURF_AOV_POSITION]);
    pl.N = static_cast<const float4*>(c->aov.p[SURF_AOV_NORMAL]);
    pl.alb = static_cast<const float4*>(c->aov.p[SURF_AOV_ALBEDO]);
    pl.ID = static_cast<const uint4*>(c->aov.p[SURF_AOV_ID]);
    if (have) {
        pl.pH = prev[0];
        pl.pP = prev[1];
        pl.pG = reinterpret_cast<const TemporalGuide*>(prev[2]);
        pl.pM = c->svHave ? c->sv[c->svCur] : nullptr;
    }
    pl.blend = c->tp[6];
    pl.hist = next[0];
    pl.gP = next[1];
    pl.gN = reinterpret_cast<TemporalGuide*>(next[2]);
    pl.outM = c->sv[c->svCur ^ 1];
    pl.var = reinterpret_cast<float*>(c->sv[2]);
    pl.clamped = c->ff[0];
    const float4* res = nullptr;
    if ((rc = runSvgf(c, c->width, c->height, pl, K, *sp, X, &res))) return rc;
    c->tpCur ^= 1;
    c->tpHave = true;
    c->tpCam = c->camUbo;
    c->tpInst = c->instHost;
    c->svCur ^= 1;
    c->svHave = true;
    SURF_CHECK(c, hipMemcpyAsync(dst, res, (size_t)c->npx * sizeof(float4), kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* stage 0 on host planes: fireflyLum's tap value of every pixel, then A' of every pixel */
std::vector<float4> fireflyHost(uint32_t w, uint32_t h, const std::vector<float4>& A, const std::vector<float4>& alb, uint32_t demod, float scale) {
    const size_t npx = (size_t)w * h;
    std::vector<float> tap(npx), l(npx);
    std::vector<V3> c(npx);
    for (size_t q = 0; q < npx; ++q) tap[q] = fireflyLum(A[q], alb[q], demod, c[q], l[q]);
    const FireflyFetchPlane fetch{tap.data(), (int)w};
    std::vector<float4> out(npx);
    for (int y = 0; y < (int)h; ++y)
        for (int x = 0; x < (int)w; ++x) {
            const size_t q = (size_t)y * w + x;
            out[q] = fireflyPixel(x, y, (int)w, (int)h, scale, A[q], c[q], l[q], tap[q], fetch);
        }
    return out;
}

/* what surf_firefly_image and its host twin refuse */
const char* fireflyError(uint32_t w, uint32_t h, const float* acc, const float* albedo, float scale, const float* out) {
    if (!acc || !albedo || !out) return "NULL argument";
    if (w == 0 || h == 0) return "w or h is 0";
    if (!(std::isfinite(scale) && scale >= 1.0f)) return "scale is not finite and >= 1";
    return nullptr;
}

/* the two float planes of variances as the (x, y, 0, 0) image the interface returns */
void interleaveVariance(const std::vector<float>& var, size_t npx, float* out) {
    for (size_t q = 0; q < npx; ++q) {
        out[4 * q] = var[q];
        out[4 * q + 1] = var[npx + q];
        out[4 * q + 2] = out[4 * q + 3] = 0.0f;
    }
}

/* what surf_svgf_image and its host twin refuse, beside the parameters */
const char* svgfFrameError(uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev, const float* out,
                           const float* outHist, const float* outMom, const float* outVar) {
    if (!cur || !outMom || !outVar) return "NULL argument";
    if (!cur->albedo) return "NULL plane in the current frame";
    const surf_temporal_frame tc{cur->acc, cur->position, cur->normal, cur->id, cur->instances, cur->instance_count, 0};
    surf_temporal_prev tq{};
    if (prev) {
        tq.history = prev->history; tq.position = prev->position; tq.normal = prev->normal; tq.id = prev->id;
        tq.instances = prev->instances; tq.instance_count = prev->instance_count;
    }
    return temporalFrameError(w, h, &tc, prev ? &tq : nullptr, out, outHist);
}

/* the guides a tap of either variance-guided filter reads, on host planes, as
 * k_svgf_guides and denoisePrepare pack them */
void packGuidesHost(const std::vector<float4>& Ps, const std::vector<float4>& Ns, const std::vector<float4>& Al, std::vector<float4>& gN,
                    std::vector<float4>& gP) {
    gN.resize(Ps.size());
    gP.resize(Ps.size());
    for (size_t q = 0; q < Ps.size(); ++q) {
        gN[q] = make_float4(Ns[q].x, Ns[q].y, Ns[q].z, Al[q].w != 0.0f ? 1.0f : 0.0f);
        gP[q] = make_float4(Ps[q].x, Ps[q].y, Ps[q].z, 0.0f);
    }
}

/* The variance-guided a-trous iterations on host planes: level 0 in lvl[0],
 * the levels used in turn; var1 takes the variance leaving the filter, Hs (not
 * NULL: feedback) the history that iteration 0 rewrites.  Returns the level
 * that holds the output. */
const std::vector<float4>& atrousVarHost(uint32_t w, uint32_t h, const surf_svgf_params& sp, const std::vector<float4>& Al,
                                         const std::vector<float4>& gN, const std::vector<float4>& gP, std::vector<float4> (&lvl)[2],
                                         float* var1, std::vector<float4>* Hs) {
    const SvgfConsts S = svgfConsts(sp);
    const uint32_t demod = sp.demodulate ? 1u : 0u;
    for (uint32_t i = 0; i < sp.iterations; ++i) {
        const int s = 1 << i;
        const bool last = i + 1 == sp.iterations;
        const std::vector<float4>& I = lvl[i & 1];
        std::vector<float4>& O = lvl[(i & 1) ^ 1];
        const DenoiseFetchPlanes fetch{I.data(), gN.data(), gP.data(), (int)w};
        for (int y = 0; y < (int)h; ++y)
            for (int x = 0; x < (int)w; ++x) {
                const size_t q = (size_t)y * w + x;
                const bool valid = gN[q].w != 0.0f;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (valid) f = denoisePixelVar(x, y, (int)w, (int)h, s, S, I[q], gN[q], gP[q], fetch);
                float v1;
                O[q] = svgfStore(valid, I[q], f, last, Al[q], demod, v1);
                if (last) var1[q] = v1;
                if (Hs && i == 0 && valid) (*Hs)[q] = svgfFeedback(f, Al[q], demod, (*Hs)[q].w);
            }
    }
    return lvl[sp.iterations & 1];
}

/* ---- the sample-variance-guided filter (surf_denoise_sampled*) ---- */

/* The launches of a run on the context's stream over device planes of a full
 * w x h frame: the guides, level 0, the iterations.  *result is the scratch
 * image that holds the output; the two variance planes are left in c->sdVar
 * (2 * npx floats, i.e. (npx + 1) / 2 records).  Waits for the result. */
int runSampled(surf_ctx* c, uint32_t w, uint32_t h, const float4* A, const float4* Q, const float4* P, const float4* N, const float4* alb,
               const surf_svgf_params& sp, const float4** result) {
    const size_t npx = (size_t)w * h;
    int rc = c->dn.grow(c, npx);
    if (rc) return rc;
    if ((rc = c->sdVar.grow(c, (npx + 1) / 2))) return rc;
    float* var = reinterpret_cast<float*>(c->sdVar[0]);
    hipLaunchKernelGGL(k_svgf_guides, dim3((uint32_t)((npx + 255) / 256)), dim3(256), 0, c->stream, P, N, alb, (uint32_t)npx, c->dn[2], c->dn[3]);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->sdTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_sampled_level0, tileGrid(w, h), dim3(256), 0, c->stream, A, Q, alb, c->dn[0], var, (int)w, (int)h, sp.demodulate ? 1u : 0u);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->sdTime.mark(1, c->stream));
    return runAtrousVar(c, w, h, sp, alb, var + npx, nullptr, c->sdTime, 1, result);
}

/* surf_denoise_sampled / _copy_device: the context's own accumulator, squares and cached feature planes */
int sampledContext(surf_ctx* c, const surf_svgf_params* sp, void* dst, hipMemcpyKind kind) {
    if (!c || !dst) return SURF_ERR_INVALID;
    if (const char* why = svgfParamError(sp, false)) return fail(c, SURF_ERR_INVALID, std::string("surf_denoise_sampled: ") + why);
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_denoise_sampled needs a context that owns every row of the frame: a spatial filter reads its "
                                         "neighbours' rows; assemble the shards' accumulators, squares and feature planes and call "
                                         "surf_denoise_sampled_image");
    if (!c->sqOn) return fail(c, SURF_ERR_INVALID, "surf_denoise_sampled: sample squares are off (surf_set_sample_squares)");
    void* const* g = nullptr;     /* the first-hit planes, the chain's or the sampled ones (surf_set_filter_guides*) */
    int rc = guidePlanes(c, &g);
    if (rc) return rc;
    if ((rc = drainStream(c))) return rc;
    const float4* res = nullptr;
    rc = runSampled(c, c->width, c->height, c->acc, c->sq, static_cast<const float4*>(g[SURF_AOV_POSITION]),
                    static_cast<const float4*>(g[SURF_AOV_NORMAL]), static_cast<const float4*>(g[SURF_AOV_ALBEDO]), *sp,
                    &res);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(dst, res, (size_t)c->npx * sizeof(float4), kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* what surf_denoise_sampled_image and its host twin refuse, beside the parameters */
const char* sampledFrameError(uint32_t w, uint32_t h, const float* acc, const float* squares, const float* position, const float* normal,
                              const float* albedo, const float* out, const float* outVar) {
    if (!acc || !squares || !position || !normal || !albedo || !out || !outVar) return "NULL argument";
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return "empty or too large a frame";
    return nullptr;
}

/* ---- the noise estimate (surf_noise_*) ---- */
const char* noiseParamError(const surf_noise_params* p) {
    if (!p) return "noise params is NULL";
    if (!(std::isfinite(p->threshold) && p->threshold > 0.0f)) return "threshold is not finite and > 0";
    if (!(std::isfinite(p->floor) && p->floor > 0.0f)) return "floor is not finite and > 0";
    return nullptr;
}

/* k_noise over device planes of npx pixels; the error image (outErr not NULL)
 * and the summary go to the host.  c->sdErr holds the sums in its first
 * record, then the image: 1 + (npx + 3) / 4 records. */
int runNoise(surf_ctx* c, uint32_t npx, const float4* A, const float4* Q, const surf_noise_params& P, float* outErr, surf_noise_summary* sum) {
    const int rc = c->sdErr.grow(c, 1 + ((size_t)npx + 3) / 4);
    if (rc) return rc;
    NoiseSums* dSums = reinterpret_cast<NoiseSums*>(c->sdErr[0]);
    float* dErr = outErr ? reinterpret_cast<float*>(c->sdErr[0] + 1) : nullptr;
    static_assert(sizeof(NoiseSums) <= sizeof(float4), "the sums fit the first record of their image");
    SURF_CHECK(c, hipMemsetAsync(dSums, 0, sizeof(NoiseSums), c->stream));
    hipLaunchKernelGGL(k_noise, dim3((npx + 255) / 256), dim3(256), 0, c->stream, A, Q, npx, P.threshold, P.floor, dErr, dSums);
    SURF_CHECK(c, hipGetLastError());
    NoiseSums hs{};
    SURF_CHECK(c, hipMemcpyAsync(&hs, dSums, sizeof hs, hipMemcpyDeviceToHost, c->stream));
    if (outErr) SURF_CHECK(c, hipMemcpyAsync(outErr, dErr, (size_t)npx * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    sum->pixels = npx;
    sum->above = hs.above;
    std::memcpy(&sum->max_error, &hs.maxBits, sizeof(float));
    sum->_pad = 0;
    return SURF_OK;
}

}  // namespace

void surfhost::freeSvgf(surf_ctx* c) {
    c->sdVar.free();
    c->sdErr.free();
    c->sdAQ.free();
    c->sdIn.free();
    c->sdTime.destroy();
    c->sv.free();
    c->svIn.free();
    c->ff.free();
    c->ffIn.free();
    c->svTime.destroy();
    c->ffTime.destroy();
    c->svHave = false;
}

extern "C" {

int surf_svgf_default_params(surf_svgf_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->iterations = 5;
    p->sigma_lum = 4.0f;
    p->sigma_normal = 0.3f;
    p->sigma_plane = 0.1f;
    p->demodulate = 1;
    p->spatial_below = 4;
    p->variance_eps = 1e-10f;
    return SURF_OK;
}

int surf_svgf_default_ext(surf_svgf_ext* x) {
    if (!x) return SURF_ERR_INVALID;
    std::memset(x, 0, sizeof *x);
    return SURF_OK;
}

int surf_svgf_accumulate(surf_ctx* c, const surf_temporal_params* p, const surf_svgf_params* sp, float* out) {
    return svgfContext(c, p, sp, nullptr, out, hipMemcpyDeviceToHost);
}

int surf_svgf_copy_device(surf_ctx* c, const surf_temporal_params* p, const surf_svgf_params* sp, void* dst) {
    return svgfContext(c, p, sp, nullptr, dst, hipMemcpyDeviceToDevice);
}

int surf_svgf_accumulate_ex(surf_ctx* c, const surf_temporal_params* p, const surf_svgf_params* sp, const surf_svgf_ext* ext, float* out) {
    return svgfContext(c, p, sp, ext, out, hipMemcpyDeviceToHost);
}

int surf_svgf_copy_device_ex(surf_ctx* c, const surf_temporal_params* p, const surf_svgf_params* sp, const surf_svgf_ext* ext, void* dst) {
    return svgfContext(c, p, sp, ext, dst, hipMemcpyDeviceToDevice);
}

int surf_svgf_moments(surf_ctx* c, float* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    if (!(c->tpHave && c->svHave)) return fail(c, SURF_ERR_INVALID, "surf_svgf_moments: no moments stored (call surf_svgf_accumulate first)");
    SURF_CHECK(c, hipSetDevice(c->device));
    SURF_CHECK(c, hipMemcpyAsync(out, c->sv[c->svCur], (size_t)c->npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_svgf_variance(surf_ctx* c, float* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    if (!(c->tpHave && c->svHave)) return fail(c, SURF_ERR_INVALID, "surf_svgf_variance: no variance stored (call surf_svgf_accumulate first)");
    SURF_CHECK(c, hipSetDevice(c->device));
    std::vector<float> var(2 * (size_t)c->npx);
    SURF_CHECK(c, hipMemcpyAsync(var.data(), c->sv[2], var.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    interleaveVariance(var, c->npx, out);
    return SURF_OK;
}

int surf_svgf_image(surf_ctx* c, uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev, const surf_temporal_params* p,
                    const surf_svgf_params* sp, float* out, float* outHist, float* outMom, float* outVar) {
    return surf_svgf_image_ex(c, w, h, cur, prev, p, sp, nullptr, out, outHist, outMom, outVar);
}

int surf_svgf_image_ex(surf_ctx* c, uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev, const surf_temporal_params* p,
                       const surf_svgf_params* sp, const surf_svgf_ext* ext, float* out, float* outHist, float* outMom, float* outVar) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = svgfFrameError(w, h, cur, prev, out, outHist, outMom, outVar)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_image: ") + why);
    if (const char* why = temporalParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_image: ") + why);
    if (const char* why = svgfParamError(sp)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_image: ") + why);
    if (const char* why = svgfExtError(ext)) return fail(c, SURF_ERR_INVALID, std::string("surf_svgf_image: ") + why);
    const surf_svgf_ext X = svgfExt(ext);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->tpIn.grow(c, npx);
    if (rc) return rc;
    if ((rc = c->svIn.grow(c, npx))) return rc;
    if (X.firefly_scale > 0.0f && (rc = c->ff.grow(c, npx))) return rc;
    const void* curSrc[4] = {cur->acc, cur->position, cur->normal, cur->id};
    for (int k = 0; k < 4; ++k) SURF_CHECK(c, hipMemcpyAsync(c->tpIn[k], curSrc[k], bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->svIn[0], cur->albedo, bytes, hipMemcpyHostToDevice, c->stream));
    std::vector<TemporalGuide> guides;
    if (prev) {
        packGuides(prev->normal, prev->id, npx, guides);
        const void* prevSrc[3] = {prev->history, prev->position, guides.data()};
        for (int k = 0; k < 3; ++k) SURF_CHECK(c, hipMemcpyAsync(c->tpIn[4 + k], prevSrc[k], bytes, hipMemcpyHostToDevice, c->stream));
        if (prev->moments) SURF_CHECK(c, hipMemcpyAsync(c->svIn[1], prev->moments, bytes, hipMemcpyHostToDevice, c->stream));
    }
    const TemporalConsts K = temporalSetup(*p, prev ? &prev->camera : nullptr, cur->instances, prev ? prev->instances : nullptr,
                                           cur->instance_count, c->tpMotionHost);
    SvgfPlanes pl{};
    pl.A = c->tpIn[0];
    pl.P = c->tpIn[1];
    pl.N = c->tpIn[2];
    pl.ID = reinterpret_cast<const uint4*>(c->tpIn[3]);
    pl.alb = c->svIn[0];
    if (prev) {
        pl.pH = c->tpIn[4];
        pl.pP = c->tpIn[5];
        pl.pG = reinterpret_cast<const TemporalGuide*>(c->tpIn[6]);
        pl.pM = prev->moments ? c->svIn[1] : nullptr;
    }
    pl.blend = c->tpIn[7];
    pl.hist = c->tpIn[8];
    pl.outM = c->svIn[2];
    pl.var = reinterpret_cast<float*>(c->svIn[3]);
    pl.clamped = c->ff[0];
    const float4* res = nullptr;
    if ((rc = runSvgf(c, w, h, pl, K, *sp, X, &res))) return rc;
    std::vector<float> var(2 * npx);
    SURF_CHECK(c, hipMemcpyAsync(out, res, bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(outHist, c->tpIn[8], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(outMom, c->svIn[2], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(var.data(), c->svIn[3], var.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    interleaveVariance(var, npx, outVar);
    return SURF_OK;
}

/* The CPU twin: temporalPixel<true>, svgfVariancePixel, denoisePixelVar and
 * their companions compiled for the host, on host arrays. */
int surf_svgf_image_host(uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev, const surf_temporal_params* p,
                         const surf_svgf_params* sp, float* out, float* outHist, float* outMom, float* outVar) {
    return surf_svgf_image_host_ex(w, h, cur, prev, p, sp, nullptr, out, outHist, outMom, outVar);
}

int surf_svgf_image_host_ex(uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev, const surf_temporal_params* p,
                            const surf_svgf_params* sp, const surf_svgf_ext* ext, float* out, float* outHist, float* outMom, float* outVar) {
    if (const char* why = svgfFrameError(w, h, cur, prev, out, outHist, outMom, outVar)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_svgf_image_host: ") + why);
    if (const char* why = temporalParamError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_svgf_image_host: ") + why);
    if (const char* why = svgfParamError(sp)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_svgf_image_host: ") + why);
    if (const char* why = svgfExtError(ext)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_svgf_image_host: ") + why);
    const surf_svgf_ext X = svgfExt(ext);
    const size_t npx = (size_t)w * h;
    std::vector<float> motion;
    const TemporalConsts K = temporalSetup(*p, prev ? &prev->camera : nullptr, cur->instances, prev ? prev->instances : nullptr,
                                           cur->instance_count, motion);
    const SvgfConsts S = svgfConsts(*sp);
    const uint32_t demod = sp->demodulate ? 1u : 0u;
    std::vector<TemporalGuide> guides;
    if (prev) packGuides(prev->normal, prev->id, npx, guides);
    const std::vector<float4> Ps = hostPlane(cur->position, npx), Ns = hostPlane(cur->normal, npx), Al = hostPlane(cur->albedo, npx);
    std::vector<float4> A = hostPlane(cur->acc, npx);
    if (X.firefly_scale > 0.0f) A = fireflyHost(w, h, A, Al, demod, X.firefly_scale);
    const std::vector<float4> prevH = hostPlane(prev ? prev->history : nullptr, npx), prevP = hostPlane(prev ? prev->position : nullptr, npx),
                              prevM = hostPlane(prev ? prev->moments : nullptr, npx);
    const TemporalFetchPlanes tfetch{prevH.data(), prevP.data(), guides.data(), (int)w, prevM.empty() ? nullptr : prevM.data()};
    std::vector<float4> R(npx), Hs(npx), M(npx), gN, gP, lvl[2] = {std::vector<float4>(npx), std::vector<float4>(npx)};
    std::vector<float> var(2 * npx, 0.0f);
    packGuidesHost(Ps, Ns, Al, gN, gP);
    for (size_t q = 0; q < npx; ++q)
        temporalPixel<true>((int)w, (int)h, A[q], Ps[q], Ns[q], cur->id[4 * q], K, motion.data(), tfetch, R[q], Hs[q], denoiseDen(Al[q], demod), M[q]);
    const SvgfFetchPlanes vfetch{gN.data(), gP.data(), M.data(), (int)w};
    for (int y = 0; y < (int)h; ++y)
        for (int x = 0; x < (int)w; ++x) {
            const size_t q = (size_t)y * w + x;
            const float v = gN[q].w != 0.0f ? svgfVariancePixel(x, y, (int)w, (int)h, S, M[q], gN[q], gP[q], vfetch) : 0.0f;
            lvl[0][q] = svgfLevel0(R[q], Al[q], demod, v);
            var[q] = lvl[0][q].w;
        }
    const std::vector<float4>& res = atrousVarHost(w, h, *sp, Al, gN, gP, lvl, var.data() + npx, X.feedback != 0u ? &Hs : nullptr);
    std::memcpy(out, res.data(), npx * sizeof(float4));
    std::memcpy(outHist, Hs.data(), npx * sizeof(float4));
    std::memcpy(outMom, M.data(), npx * sizeof(float4));
    interleaveVariance(var, npx, outVar);
    return SURF_OK;
}

int surf_firefly_image(surf_ctx* c, uint32_t w, uint32_t h, const float* acc, const float* albedo, uint32_t demodulate, float scale, float* out) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = fireflyError(w, h, acc, albedo, scale, out)) return fail(c, SURF_ERR_INVALID, std::string("surf_firefly_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->ffIn.grow(c, npx);
    if (rc) return rc;
    if ((rc = c->ff.grow(c, npx))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->ffIn[0], acc, bytes, hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->ffIn[1], albedo, bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = launchFirefly(c, w, h, c->ffIn[0], c->ffIn[1], scale, demodulate ? 1u : 0u, c->ff[0]))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, c->ff[0], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return fireflyTime(c);
}

/* The CPU twin: fireflyLum and fireflyPixel compiled for the host, on host arrays. */
int surf_firefly_image_host(uint32_t w, uint32_t h, const float* acc, const float* albedo, uint32_t demodulate, float scale, float* out) {
    if (const char* why = fireflyError(w, h, acc, albedo, scale, out)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_firefly_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const std::vector<float4> res = fireflyHost(w, h, hostPlane(acc, npx), hostPlane(albedo, npx), demodulate ? 1u : 0u, scale);
    std::memcpy(out, res.data(), npx * sizeof(float4));
    return SURF_OK;
}

int surf_debug_firefly_time(surf_ctx* c, float* kernel_ms) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->ffTime.read(kernel_ms, 1);
    return SURF_OK;
}

int surf_denoise_sampled(surf_ctx* c, const surf_svgf_params* sp, float* out) { return sampledContext(c, sp, out, hipMemcpyDeviceToHost); }

int surf_denoise_sampled_copy_device(surf_ctx* c, const surf_svgf_params* sp, void* dst) {
    return sampledContext(c, sp, dst, hipMemcpyDeviceToDevice);
}

int surf_denoise_sampled_image(surf_ctx* c, uint32_t w, uint32_t h, const float* acc, const float* squares, const float* position,
                               const float* normal, const float* albedo, const surf_svgf_params* sp, float* out, float* outVar) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = sampledFrameError(w, h, acc, squares, position, normal, albedo, out, outVar))
        return fail(c, SURF_ERR_INVALID, std::string("surf_denoise_sampled_image: ") + why);
    if (const char* why = svgfParamError(sp, false)) return fail(c, SURF_ERR_INVALID, std::string("surf_denoise_sampled_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->sdAQ.grow(c, npx);
    if (rc) return rc;
    if ((rc = c->sdIn.grow(c, npx))) return rc;
    float4* const dst[5] = {c->sdAQ[0], c->sdAQ[1], c->sdIn[0], c->sdIn[1], c->sdIn[2]};
    const float* src[5] = {acc, squares, position, normal, albedo};
    for (int k = 0; k < 5; ++k) SURF_CHECK(c, hipMemcpyAsync(dst[k], src[k], bytes, hipMemcpyHostToDevice, c->stream));
    const float4* res = nullptr;
    if ((rc = runSampled(c, w, h, dst[0], dst[1], dst[2], dst[3], dst[4], *sp, &res))) return rc;
    std::vector<float> var(2 * npx);
    SURF_CHECK(c, hipMemcpyAsync(out, res, bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(var.data(), c->sdVar[0], var.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    interleaveVariance(var, npx, outVar);
    return SURF_OK;
}

/* The CPU twin: sampledLevel0, denoisePixelVar and svgfStore compiled for the host, on host arrays. */
int surf_denoise_sampled_image_host(uint32_t w, uint32_t h, const float* acc, const float* squares, const float* position, const float* normal,
                                    const float* albedo, const surf_svgf_params* sp, float* out, float* outVar) {
    if (const char* why = sampledFrameError(w, h, acc, squares, position, normal, albedo, out, outVar))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_sampled_image_host: ") + why);
    if (const char* why = svgfParamError(sp, false)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_denoise_sampled_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    const uint32_t demod = sp->demodulate ? 1u : 0u;
    const std::vector<float4> A = hostPlane(acc, npx), Q = hostPlane(squares, npx), Ps = hostPlane(position, npx), Ns = hostPlane(normal, npx),
                              Al = hostPlane(albedo, npx);
    std::vector<float4> gN, gP, lvl[2] = {std::vector<float4>(npx), std::vector<float4>(npx)};
    std::vector<float> var(2 * npx, 0.0f);
    packGuidesHost(Ps, Ns, Al, gN, gP);
    for (size_t q = 0; q < npx; ++q) {
        lvl[0][q] = sampledLevel0(A[q], Q[q], Al[q], demod);
        var[q] = lvl[0][q].w;
    }
    const std::vector<float4>& res = atrousVarHost(w, h, *sp, Al, gN, gP, lvl, var.data() + npx, nullptr);
    std::memcpy(out, res.data(), npx * sizeof(float4));
    interleaveVariance(var, npx, outVar);
    return SURF_OK;
}

int surf_debug_sampled_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->sdTime.read(kernel_ms, count);
    return SURF_OK;
}

int surf_noise_default_params(surf_noise_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->threshold = 0.05f;
    p->floor = 0.01f;
    return SURF_OK;
}

int surf_noise_estimate(surf_ctx* c, const surf_noise_params* p, float* outErr, surf_noise_summary* sum) {
    if (!c || !sum) return SURF_ERR_INVALID;
    if (const char* why = noiseParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_noise_estimate: ") + why);
    if (!c->sqOn) return fail(c, SURF_ERR_INVALID, "surf_noise_estimate: sample squares are off (surf_set_sample_squares)");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = drainStream(c);
    if (rc) return rc;
    return runNoise(c, c->npx, c->acc, c->sq, *p, outErr, sum);
}

int surf_noise_image(surf_ctx* c, uint32_t npx, const float* acc, const float* squares, const surf_noise_params* p, float* outErr,
                     surf_noise_summary* sum) {
    if (!c || !acc || !squares || !sum) return SURF_ERR_INVALID;
    if (npx == 0 || npx > (1u << 31)) return fail(c, SURF_ERR_INVALID, "surf_noise_image: no pixels or too many");
    if (const char* why = noiseParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_noise_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = c->sdAQ.grow(c, npx);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(c->sdAQ[0], acc, (size_t)npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(c->sdAQ[1], squares, (size_t)npx * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    return runNoise(c, npx, c->sdAQ[0], c->sdAQ[1], *p, outErr, sum);
}

/* The CPU twin: noiseError, noiseAbove and noiseMax compiled for the host. */
int surf_noise_image_host(uint32_t npx, const float* acc, const float* squares, const surf_noise_params* p, float* outErr,
                          surf_noise_summary* sum) {
    if (!acc || !squares || !sum) return fail(nullptr, SURF_ERR_INVALID, "surf_noise_image_host: NULL argument");
    if (npx == 0 || npx > (1u << 31)) return fail(nullptr, SURF_ERR_INVALID, "surf_noise_image_host: no pixels or too many");
    if (const char* why = noiseParamError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_noise_image_host: ") + why);
    std::memset(sum, 0, sizeof *sum);
    sum->pixels = npx;
    for (size_t q = 0; q < npx; ++q) {
        float4 A, Q;                                             /* the caller's planes need not be 16-byte aligned */
        std::memcpy(&A, acc + 4 * q, sizeof A);
        std::memcpy(&Q, squares + 4 * q, sizeof Q);
        const float e = noiseError(A, Q, p->floor);
        if (outErr) outErr[q] = e;
        if (noiseAbove(e, p->threshold)) ++sum->above;
        sum->max_error = noiseMax(sum->max_error, e);
    }
    return SURF_OK;
}

int surf_debug_svgf_time(surf_ctx* c, float* kernel_ms, uint32_t count) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->svTime.read(kernel_ms, count);
    return SURF_OK;
}

}  // extern "C"
