/*
 * temporal.hip -- temporal accumulation with reprojection (surf_temporal*,
 * include/surf_hip.h): parameter checks, the per-frame constants and motion
 * table, the k_temporal launch, the state a frame leaves on the context for
 * the next, and the CPU twin.  The arithmetic lives in
 * device/temporal_kernels.h.
 */
#include "host/filter_host.h"

#include <cmath>

#include "host/temporal_host.h"

const char* surfhost::temporalParamError(const surf_temporal_params* p) {
    if (!p) return "params is NULL";
    if (!(p->alpha_min >= 0.0f && p->alpha_min <= 1.0f)) return "alpha_min outside [0, 1]";
    if (p->max_history == 0) return "max_history is 0";
    if (!(p->normal_min >= -1.0f && p->normal_min <= 1.0f)) return "normal_min outside [-1, 1]";
    if (!(std::isfinite(p->plane_tol) && p->plane_tol > 0.0f)) return "plane_tol is not finite and > 0";
    if (!(std::isfinite(p->min_weight) && p->min_weight > 0.0f)) return "min_weight is not finite and > 0";
    if (!(p->snap >= 0.0f && p->snap < 0.5f)) return "snap outside [0, 0.5)";
    return nullptr;
}

/* The constants of a frame, in f32 on the host as the header states, and the
 * motion table (kTemporalMotionWords floats per instance).  cam, prevInst
 * NULL: no previous frame. */
TemporalConsts surfhost::temporalSetup(const surf_temporal_params& p, const surf_camera_ubo* cam, const surf_gpu_instance* curInst,
                                       const surf_gpu_instance* prevInst, uint32_t nInst, std::vector<float>& motion) {
    TemporalConsts K{};
    K.alphaMin = p.alpha_min;
    K.maxHistory = (float)p.max_history;
    K.normalMin = p.normal_min;
    K.planeTol = p.plane_tol;
    K.snap = p.snap;
    K.minWeight = p.min_weight;
    motion.clear();
    if (!cam) return K;
    K.havePrev = 1u;
    K.nInst = nInst;
    const float C[3] = {cam->position.x, cam->position.y, cam->position.z};
    const float F0[3] = {cam->first_pixel.x, cam->first_pixel.y, cam->first_pixel.z};
    const float U[3] = {cam->u_vector.x, cam->u_vector.y, cam->u_vector.z};
    const float V[3] = {cam->v_vector.x, cam->v_vector.y, cam->v_vector.z};
    for (int a = 0; a < 3; ++a) {
        K.C[a] = C[a];
        K.G[a] = F0[a] - C[a];
        K.U[a] = U[a];
        K.V[a] = V[a];
    }
    K.n[0] = U[1] * V[2] - U[2] * V[1];
    K.n[1] = U[2] * V[0] - U[0] * V[2];
    K.n[2] = U[0] * V[1] - U[1] * V[0];
    K.g = (K.G[0] * K.n[0] + K.G[1] * K.n[1]) + K.G[2] * K.n[2];
    K.iu = 1.0f / ((U[0] * U[0] + U[1] * U[1]) + U[2] * U[2]);
    K.iv = 1.0f / ((V[0] * V[0] + V[1] * V[1]) + V[2] * V[2]);
    K.resx = cam->resolution[0];
    K.resy = cam->resolution[1];
    motion.resize((size_t)kTemporalMotionWords * nInst);
    for (uint32_t i = 0; i < nInst; ++i)
        temporalMotionRecord(curInst[i].transform, curInst[i].inv_transform, prevInst[i].transform, prevInst[i].inv_transform,
                             &motion[(size_t)kTemporalMotionWords * i]);
    return K;
}

/* the motion table of c->tpMotionHost on the device (c->tpMotion), queued on the context's stream */
int surfhost::temporalMotionUpload(surf_ctx* c, const TemporalConsts& K) {
    if (K.nInst > c->tpMotionCap) {
        if (c->tpMotion) (void)hipFree(c->tpMotion);
        c->tpMotion = nullptr;
        c->tpMotionCap = 0;
        const size_t bytes = (size_t)kTemporalMotionWords * K.nInst * sizeof(float);
        if (hipMalloc(reinterpret_cast<void**>(&c->tpMotion), bytes) != hipSuccess || !c->tpMotion) {
            c->tpMotion = nullptr;
            (void)hipGetLastError();
            return fail(c, SURF_ERR_OOM, "hipMalloc of the motion table (" + std::to_string(bytes) + " bytes) failed");
        }
        c->tpMotionCap = K.nInst;
    }
    if (K.nInst)
        SURF_CHECK(c, hipMemcpyAsync(c->tpMotion, c->tpMotionHost.data(), c->tpMotionHost.size() * sizeof(float), hipMemcpyHostToDevice,
                                     c->stream));
    return SURF_OK;
}

namespace {

/* One launch on the context's stream over device planes of a full w x h
 * frame; pH, pP, pG NULL with K.havePrev 0.  Waits for the result. */
int runTemporal(surf_ctx* c, uint32_t w, uint32_t h, const float4* A, const float4* P, const float4* N, const uint4* ID,
                const float4* pH, const float4* pP, const TemporalGuide* pG, const TemporalConsts& K, float4* out, float4* hist,
                float4* gP, TemporalGuide* gN) {
    if (int rc = temporalMotionUpload(c, K)) return rc;
    const dim3 grid((w + kTemporalTileW - 1) / kTemporalTileW, (h + kTemporalTileH - 1) / kTemporalTileH);
    SURF_CHECK(c, c->tpTime.mark(0, c->stream));
    hipLaunchKernelGGL(k_temporal<false>, grid, dim3(256), 0, c->stream, A, P, N, ID, pH, pP, pG, (const float*)c->tpMotion, K, (int)w, (int)h,
                       out, hist, gP, gN, TemporalMomentPlanes{});
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, c->tpTime.mark(1, c->stream));
    SURF_CHECK(c, c->tpTime.collect(1));
    return SURF_OK;
}

/* surf_temporal_accumulate / _copy_device: the context's own accumulator and
 * cached feature planes against the stored state, which this frame's replaces */
int temporalContext(surf_ctx* c, const surf_temporal_params* p, const surf_denoise_params* spatial, void* dst, hipMemcpyKind kind) {
    if (!c || !dst) return SURF_ERR_INVALID;
    if (const char* why = temporalParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_temporal_accumulate: ") + why);
    if (spatial)
        if (const char* why = denoiseParamsError(spatial)) return fail(c, SURF_ERR_INVALID, std::string("surf_temporal_accumulate: spatial: ") + why);
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, "surf_temporal_accumulate needs a context that owns every row of the frame: a reprojected pixel "
                                         "reads other rows of the previous frame; assemble the shards' accumulators and feature planes "
                                         "and call surf_temporal_image");
    int rc = featurePlanes(c);
    if (rc) return rc;
    if ((rc = drainStream(c))) return rc;
    if ((rc = c->tp.grow(c, c->npx))) { c->tpHave = false; return rc; }
    const bool have = c->tpHave && c->tpInst.size() == c->instHost.size();
    const uint32_t nInst = (uint32_t)c->instHost.size();
    const TemporalConsts K = temporalSetup(*p, have ? &c->tpCam : nullptr, c->instHost.data(), have ? c->tpInst.data() : nullptr, nInst,
                                           c->tpMotionHost);
    float4* const* prev = c->tp.p + 3 * c->tpCur;
    float4* const* next = c->tp.p + 3 * (c->tpCur ^ 1);
    const float4* pos = static_cast<const float4*>(c->aov.p[SURF_AOV_POSITION]);
    const float4* nrm = static_cast<const float4*>(c->aov.p[SURF_AOV_NORMAL]);
    rc = runTemporal(c, c->width, c->height, c->acc, pos, nrm, static_cast<const uint4*>(c->aov.p[SURF_AOV_ID]), have ? prev[0] : nullptr,
                     have ? prev[1] : nullptr, have ? reinterpret_cast<const TemporalGuide*>(prev[2]) : nullptr, K, c->tp[6], next[0],
                     next[1], reinterpret_cast<TemporalGuide*>(next[2]));
    if (rc) return rc;
    c->tpCur ^= 1;
    c->tpHave = true;
    c->tpCam = c->camUbo;
    c->tpInst = c->instHost;
    c->svHave = false;                /* this history carries no moments: the next surf_svgf_accumulate estimates spatially */
    const float4* res = c->tp[6];
    if (spatial) {
        rc = denoisePlanes(c, c->width, c->height, c->tp[6], pos, nrm, static_cast<const float4*>(c->aov.p[SURF_AOV_ALBEDO]), *spatial, &res);
        if (rc) return rc;
    }
    SURF_CHECK(c, hipMemcpyAsync(dst, res, (size_t)c->npx * sizeof(float4), kind, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

}  // namespace

/* what surf_temporal_image and its host twin refuse, beside the parameters */
const char* surfhost::temporalFrameError(uint32_t w, uint32_t h, const surf_temporal_frame* cur, const surf_temporal_prev* prev, const float* out,
                               const float* outHist) {
    if (!cur || !out || !outHist) return "NULL argument";
    if (!cur->acc || !cur->position || !cur->normal || !cur->id || (cur->instance_count && !cur->instances)) return "NULL plane in the current frame";
    if (prev && (!prev->history || !prev->position || !prev->normal || !prev->id || (prev->instance_count && !prev->instances)))
        return "NULL plane in the previous frame";
    if (w == 0 || h == 0 || (uint64_t)w * h > (1ull << 31)) return "empty or too large a frame";
    if (prev && prev->instance_count != cur->instance_count) return "instance counts differ between the two frames";
    return nullptr;
}

/* the previous frame's normal and id planes as the guide a tap reads */
void surfhost::packGuides(const float* normal, const uint32_t* id, size_t npx, std::vector<TemporalGuide>& g) {
    g.resize(npx);
    for (size_t q = 0; q < npx; ++q) {
        g[q].x = normal[4 * q];
        g[q].y = normal[4 * q + 1];
        g[q].z = normal[4 * q + 2];
        g[q].id = id[4 * q];
    }
}

void surfhost::freeTemporal(surf_ctx* c) {
    c->tp.free();
    c->tpIn.free();
    if (c->tpMotion) (void)hipFree(c->tpMotion);
    c->tpMotion = nullptr;
    c->tpTime.destroy();
    c->tpMotionCap = 0;
    c->tpHave = false;
    freeSvgf(c);
}

extern "C" {

int surf_temporal_default_params(surf_temporal_params* p) {
    if (!p) return SURF_ERR_INVALID;
    std::memset(p, 0, sizeof *p);
    p->alpha_min = 0.0f;
    p->max_history = 32;
    p->normal_min = 0.9f;
    p->plane_tol = 0.01f;
    p->snap = 0.015625f;
    p->min_weight = 0.01f;
    return SURF_OK;
}

int surf_temporal_accumulate(surf_ctx* c, const surf_temporal_params* p, const surf_denoise_params* spatial, float* out) {
    return temporalContext(c, p, spatial, out, hipMemcpyDeviceToHost);
}

int surf_temporal_copy_device(surf_ctx* c, const surf_temporal_params* p, const surf_denoise_params* spatial, void* dst) {
    return temporalContext(c, p, spatial, dst, hipMemcpyDeviceToDevice);
}

int surf_temporal_reset(surf_ctx* c) {
    if (!c) return SURF_ERR_INVALID;
    c->tpHave = false;
    c->svHave = false;
    return SURF_OK;
}

int surf_temporal_history(surf_ctx* c, float* out) {
    if (!c || !out) return SURF_ERR_INVALID;
    if (!c->tpHave) return fail(c, SURF_ERR_INVALID, "surf_temporal_history: no history stored (call surf_temporal_accumulate first)");
    SURF_CHECK(c, hipSetDevice(c->device));
    SURF_CHECK(c, hipMemcpyAsync(out, c->tp[3 * c->tpCur], (size_t)c->npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_temporal_image(surf_ctx* c, uint32_t w, uint32_t h, const surf_temporal_frame* cur, const surf_temporal_prev* prev,
                        const surf_temporal_params* p, float* out, float* outHist) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = temporalFrameError(w, h, cur, prev, out, outHist)) return fail(c, SURF_ERR_INVALID, std::string("surf_temporal_image: ") + why);
    if (const char* why = temporalParamError(p)) return fail(c, SURF_ERR_INVALID, std::string("surf_temporal_image: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    const size_t npx = (size_t)w * h, bytes = npx * sizeof(float4);
    int rc = c->tpIn.grow(c, npx);
    if (rc) return rc;
    const void* curSrc[4] = {cur->acc, cur->position, cur->normal, cur->id};
    for (int k = 0; k < 4; ++k) SURF_CHECK(c, hipMemcpyAsync(c->tpIn[k], curSrc[k], bytes, hipMemcpyHostToDevice, c->stream));
    std::vector<TemporalGuide> guides;
    if (prev) {
        packGuides(prev->normal, prev->id, npx, guides);
        const void* prevSrc[3] = {prev->history, prev->position, guides.data()};
        for (int k = 0; k < 3; ++k) SURF_CHECK(c, hipMemcpyAsync(c->tpIn[4 + k], prevSrc[k], bytes, hipMemcpyHostToDevice, c->stream));
    }
    const TemporalConsts K = temporalSetup(*p, prev ? &prev->camera : nullptr, cur->instances, prev ? prev->instances : nullptr,
                                           cur->instance_count, c->tpMotionHost);
    rc = runTemporal(c, w, h, c->tpIn[0], c->tpIn[1], c->tpIn[2], reinterpret_cast<const uint4*>(c->tpIn[3]), prev ? c->tpIn[4] : nullptr,
                     prev ? c->tpIn[5] : nullptr, prev ? reinterpret_cast<const TemporalGuide*>(c->tpIn[6]) : nullptr, K, c->tpIn[7],
                     c->tpIn[8], nullptr, nullptr);
    if (rc) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, c->tpIn[7], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(outHist, c->tpIn[8], bytes, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

/* The CPU twin: temporalPixel of device/temporal_kernels.h compiled for the host, on host arrays. */
int surf_temporal_image_host(uint32_t w, uint32_t h, const surf_temporal_frame* cur, const surf_temporal_prev* prev,
                             const surf_temporal_params* p, float* out, float* outHist) {
    if (const char* why = temporalFrameError(w, h, cur, prev, out, outHist)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_temporal_image_host: ") + why);
    if (const char* why = temporalParamError(p)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_temporal_image_host: ") + why);
    const size_t npx = (size_t)w * h;
    std::vector<float> motion;
    const TemporalConsts K = temporalSetup(*p, prev ? &prev->camera : nullptr, cur->instances, prev ? prev->instances : nullptr,
                                           cur->instance_count, motion);
    std::vector<TemporalGuide> guides;
    if (prev) packGuides(prev->normal, prev->id, npx, guides);
    const std::vector<float4> A = hostPlane(cur->acc, npx), P = hostPlane(cur->position, npx), N = hostPlane(cur->normal, npx);
    const std::vector<float4> prevH = hostPlane(prev ? prev->history : nullptr, npx), prevP = hostPlane(prev ? prev->position : nullptr, npx);
    const TemporalFetchPlanes fetch{prevH.data(), prevP.data(), guides.data(), (int)w, nullptr};
    std::vector<float4> O(npx), Hs(npx);
    for (size_t q = 0; q < npx; ++q) {
        float4 unused;
        temporalPixel<false>((int)w, (int)h, A[q], P[q], N[q], cur->id[4 * q], K, motion.data(), fetch, O[q], Hs[q], mk3(1.0f, 1.0f, 1.0f), unused);
    }
    std::memcpy(out, O.data(), npx * sizeof(float4));
    std::memcpy(outHist, Hs.data(), npx * sizeof(float4));
    return SURF_OK;
}

int surf_debug_temporal_time(surf_ctx* c, float* kernel_ms) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->tpTime.read(kernel_ms, 1);
    return SURF_OK;
}

}  // extern "C"
