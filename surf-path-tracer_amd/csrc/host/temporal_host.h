/*
 * temporal_host.h -- internal: what host/temporal.hip defines for the
 * variance-guided filter (host/svgf.hip), which runs the same reprojection
 * with the moments switched on: the parameter and frame checks, the per-frame
 * constants and motion table, and the previous frame's packed guides.
 */
#pragma once
#include "host/surf_ctx.h"

#include "device/temporal_kernels.h"

namespace surfhost {
/* NULL when valid, else what is wrong */
const char* temporalParamError(const surf_temporal_params* p);
const char* temporalFrameError(uint32_t w, uint32_t h, const surf_temporal_frame* cur, const surf_temporal_prev* prev, const float* out,
                               const float* outHist);
/* the constants of a frame and its motion table; cam, prevInst NULL: no previous frame */
TemporalConsts temporalSetup(const surf_temporal_params& p, const surf_camera_ubo* cam, const surf_gpu_instance* curInst,
                             const surf_gpu_instance* prevInst, uint32_t nInst, std::vector<float>& motion);
int temporalMotionUpload(surf_ctx* c, const TemporalConsts& K);
void packGuides(const float* normal, const uint32_t* id, size_t npx, std::vector<TemporalGuide>& g);
}  // namespace surfhost
