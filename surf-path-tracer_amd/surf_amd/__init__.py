"""ctypes binding of libsurf_hip.so (include/surf_hip.h).

Python is test/bench plumbing here: the product is the C-ABI library (HIP
kernels for gfx950 + C++ host API).  Importing this module never falls back
to anything: if the library is missing, `load()` raises.

Mirrors the reference interface for the hot path:
  Scene.indoor(...)            main.cpp:161-346 scene (Mesh/BvhBLAS/Instance/GPUScene)
  Renderer(...)                WaveFrontRenderer (renderer.h:207-436)
    .render(frames, first, spp=) render loop: frames of spp samples per pixel (Renderer::render)
    .clear_accumulator()       IRenderer::clearAccumulator
    .accumulator()             float RGBA accumulator (rows of this shard)
    .finalize_rgba8()          wavefront_finalize.comp + RgbaToU32
    .trace_closest/.trace_any  ray_extend / ray_connect traversal (tests)
    .aov()                     first-hit feature buffers (no reference counterpart)
    .aov_chain(max_links)      the same planes traced through mirrors and glass; .set_filter_guides("chain") guides
                               denoise() and denoise_sampled() with them (no reference counterpart)
    .ao(samples, radius)       ray-traced ambient occlusion and bent normals from the first-hit or chain planes
    .aov_sampled(samples)      the features of the camera rays render() traces, reduced per pixel: anti-aliased planes and an
                               id coverage matte (matte_coverage); .set_filter_guides("sampled") guides the same filters
    .denoise()                 edge-avoiding a-trous filter on them (no reference counterpart)
    .temporal()                temporal accumulation with reprojection across cleared frames (no reference counterpart)
    .svgf()                    the same with luminance moments, their variance guiding the a-trous filter (no reference counterpart);
                               firefly_scale= and feedback= switch on the firefly clamp and the filtered-history feedback
    .set_sample_squares(on)    per-sample second moments beside the accumulator, .sample_squares() reads them (no reference counterpart)
    .denoise_sampled()         the a-trous filter guided by each pixel's own sample variance, for stills from about 16 spp
    .noise_estimate()          per-pixel relative standard error of the mean luminance and its summary
    .set_pixel_mask(mask)      per-pixel sample mask: render() then traces the active pixels only (no reference counterpart)
    .mask_from_noise()         the mask from the noise estimate; .render_adaptive() the "render until converged" loop around it
    .finalize_weighted()       RGBA8 with each pixel divided by its own sample count
    .set_sample_buckets(M)     M partial accumulators per pixel, .sample_buckets() reads them, bucket_halves() sums the half images
    .robust()                  the median-of-means estimate of the accumulator with a Gini-adaptive trim (no reference counterpart)
    .denoise_nlm()             dual-buffer non-local means on the buckets' two half images: no feature plane, an error estimate beside it
    .denoise_regress()         first-order regression of the two half images on the feature planes with those patch weights
    .render_adaptive_nlm()     the adaptive loop driven by that error estimate (.mask_from_nlm() builds its mask); returns the filtered image
    .display()                 the display stage on the accumulator: metered exposure, bloom, tone curve, sRGB, dither -> RGBA8;
                               .display_image(img) the same on any float RGBA image, display_image_host(img) its CPU twin
    .bake(pos, nrm, frames)    the surfel sensor: path-traced irradiance at the caller's texels
    .atlas_build(scene, charts, W, H)  the light-map atlas: charts' UV layouts rasterized to one surfel per texel;
                               .atlas_finish / .atlas_dilate turn the baked accumulator into the texture and fill its gutters,
                               .bake_atlas(scene, charts, frames) runs all of it on the device; atlas_*_host are the CPU twins
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "lib", "libsurf_hip.so")
MGPU_LIB_PATH = os.path.join(_PKG, "lib", "libsurf_mgpu.so")
REPO_ROOT = os.path.dirname(_PKG)
ASSETS_DIR = os.path.join(REPO_ROOT, "assets")

SURF_OK = 0
_STATUS = {
    -1: "SURF_ERR_INVALID", -2: "SURF_ERR_HIP", -3: "SURF_ERR_NO_DEVICE", -4: "SURF_ERR_NO_SCENE",
    -5: "SURF_ERR_OOM", -6: "SURF_ERR_IO", -7: "SURF_ERR_LIMIT",
}


SENSOR_CAMERA, SENSOR_SURFELS = 0, 1    # surf_get_sensor's kinds


class SurfError(RuntimeError):
    def __init__(self, code: int, what: str, detail: str):
        super().__init__(f"{what} failed: {_STATUS.get(code, code)}: {detail}")
        self.code = code


class SceneDesc(C.Structure):
    _fields_ = [
        ("triangles", C.c_void_p), ("triangle_count", C.c_uint32),
        ("tri_ext", C.c_void_p),
        ("blas_indices", C.c_void_p), ("blas_index_count", C.c_uint32),
        ("blas_nodes", C.c_void_p), ("blas_node_count", C.c_uint32),
        ("materials", C.c_void_p), ("material_count", C.c_uint32),
        ("instances", C.c_void_p), ("instance_count", C.c_uint32),
        ("tlas_indices", C.c_void_p),
        ("tlas_nodes", C.c_void_p), ("tlas_node_count", C.c_uint32),
        ("lights", C.c_void_p), ("light_count", C.c_uint32),
        ("background", C.c_void_p),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("samples", C.c_uint64), ("n_ext", C.c_uint64), ("n_hit", C.c_uint64), ("n_cont", C.c_uint64),
        ("n_shadow", C.c_uint64), ("n_acc", C.c_uint64), ("n_unocc", C.c_uint64), ("iterations", C.c_uint64),
        ("tail_paths", C.c_uint64),
        ("ms_total", C.c_double), ("ms_extend", C.c_double), ("ms_shade", C.c_double), ("ms_connect", C.c_double),
        ("ms_regen", C.c_double), ("ms_tail", C.c_double), ("ms_accum", C.c_double), ("ms_sort", C.c_double),
        ("launches_extend", C.c_uint64), ("n_ext_wavefront", C.c_uint64),
        ("stack_depth", C.c_uint32), ("pool_capacity", C.c_uint32),
        ("energy", C.c_float), ("max_segments", C.c_uint32), ("tail_survivors", C.c_uint64),
        ("frame_window", C.c_uint32), ("n_shadow_overflow", C.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_ if not k.startswith("_")}


class DenoiseParams(C.Structure):
    """surf_denoise_params (include/surf_hip.h gives the filter's arithmetic)."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_plane", C.c_float), ("demodulate", C.c_uint32), ("_pad", C.c_uint32 * 3)]


class TemporalParams(C.Structure):
    """surf_temporal_params (include/surf_hip.h gives the arithmetic)."""
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_uint32), ("normal_min", C.c_float), ("plane_tol", C.c_float),
                ("snap", C.c_float), ("min_weight", C.c_float), ("_pad", C.c_uint32 * 2)]


CameraUBO = C.c_uint8 * 128


class TemporalFrame(C.Structure):
    """surf_temporal_frame: host planes of the current frame."""
    _fields_ = [("acc", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("id", C.c_void_p),
                ("instances", C.c_void_p), ("instance_count", C.c_uint32), ("_pad", C.c_uint32)]


class TemporalPrev(C.Structure):
    """surf_temporal_prev: host planes, instance records and camera of the previous frame."""
    _fields_ = [("history", C.c_void_p), ("position", C.c_void_p), ("normal", C.c_void_p), ("id", C.c_void_p),
                ("instances", C.c_void_p), ("instance_count", C.c_uint32), ("_pad", C.c_uint32), ("camera", CameraUBO)]


class SvgfParams(C.Structure):
    """surf_svgf_params (include/surf_hip.h gives the arithmetic)."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_lum", C.c_float), ("sigma_normal", C.c_float), ("sigma_plane", C.c_float),
                ("demodulate", C.c_uint32), ("spatial_below", C.c_uint32), ("variance_eps", C.c_float), ("_pad", C.c_uint32)]


class SvgfExt(C.Structure):
    """surf_svgf_ext: the firefly clamp (firefly_scale 0 = off, else >= 1) and the filtered-history feedback (0 / 1)."""
    _fields_ = [("firefly_scale", C.c_float), ("feedback", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class SvgfFrame(C.Structure):
    """surf_svgf_frame: surf_temporal_frame plus the albedo plane."""
    _fields_ = TemporalFrame._fields_ + [("albedo", C.c_void_p)]


class SvgfPrev(C.Structure):
    """surf_svgf_prev: surf_temporal_prev plus the moments plane (None: no moments stored)."""
    _fields_ = TemporalPrev._fields_ + [("moments", C.c_void_p)]


class NoiseParams(C.Structure):
    """surf_noise_params: the threshold a pixel's relative standard error is counted against and the floor under its mean luminance."""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float)]


class NoiseSummary(C.Structure):
    """surf_noise_summary: pixels looked at, pixels above the threshold, the largest error."""
    _fields_ = [("pixels", C.c_uint64), ("above", C.c_uint64), ("max_error", C.c_float), ("_pad", C.c_uint32)]

    def as_dict(self) -> dict:
        return {"pixels": int(self.pixels), "above": int(self.above), "max_error": float(self.max_error)}


class RobustParams(C.Structure):
    """surf_robust_params: the factor on the Gini coefficient that decides how many bucket means are dropped."""
    _fields_ = [("trim_scale", C.c_float), ("_pad", C.c_uint32)]


class RobustSummary(C.Structure):
    """surf_robust_summary: pixels looked at, pixels whose extreme bucket means were dropped."""
    _fields_ = [("pixels", C.c_uint64), ("trimmed", C.c_uint64)]

    def as_dict(self) -> dict:
        return {"pixels": int(self.pixels), "trimmed": int(self.trimmed)}


class NlmParams(C.Structure):
    """surf_nlm_params: the search and patch radii, the distance's scale k, the variance cancellation alpha, eps."""
    _fields_ = [("search_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("k", C.c_float), ("alpha", C.c_float), ("eps", C.c_float),
                ("_pad", C.c_uint32)]


class RegressParams(C.Structure):
    """surf_regress_params: surf_nlm_params' radii, k, alpha and eps, and the ridge of the regression."""
    _fields_ = [("search_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("k", C.c_float), ("alpha", C.c_float), ("eps", C.c_float),
                ("ridge", C.c_float)]


class AdaptiveMaskParams(C.Structure):
    """surf_adaptive_mask_params: the noise estimate's threshold and floor, the sample counts a pixel stays active
    below / stops at, and the dilation of the noisy pixels."""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32),
                ("dilate", C.c_uint32), ("_pad", C.c_uint32 * 3)]


class AdaptiveParams(C.Structure):
    """surf_adaptive_params: the mask's parameters and the loop's."""
    _fields_ = [("mask", AdaptiveMaskParams), ("batch", C.c_uint32), ("max_segments", C.c_uint32),
                ("first_sample_index", C.c_uint32), ("_pad", C.c_uint32)]


class AdaptiveSummary(C.Structure):
    """surf_adaptive_summary."""
    _fields_ = [("rounds", C.c_uint32), ("frames", C.c_uint32), ("active_last", C.c_uint32), ("_pad", C.c_uint32),
                ("samples", C.c_uint64), ("noise", NoiseSummary)]


class ErrorMaskParams(C.Structure):
    """surf_error_mask_params: the relative RMS error a filtered pixel may keep and its floor, the sample counts a pixel
    stays active below / stops at, the box radius the estimate is smoothed with, and the dilation of the noisy pixels."""
    _fields_ = [("threshold", C.c_float), ("floor", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32),
                ("smooth", C.c_uint32), ("dilate", C.c_uint32), ("_pad", C.c_uint32 * 2)]


class AdaptiveNlmParams(C.Structure):
    """surf_adaptive_nlm_params: the mask's parameters, the filter's and the loop's."""
    _fields_ = [("mask", ErrorMaskParams), ("nlm", NlmParams), ("batch", C.c_uint32), ("max_segments", C.c_uint32),
                ("first_sample_index", C.c_uint32), ("_pad", C.c_uint32)]


class AdaptiveNlmSummary(C.Structure):
    """surf_adaptive_nlm_summary."""
    _fields_ = [("rounds", C.c_uint32), ("frames", C.c_uint32), ("active_last", C.c_uint32), ("_pad", C.c_uint32),
                ("samples", C.c_uint64), ("above", C.c_uint64), ("max_error", C.c_float), ("_pad2", C.c_uint32)]


class DisplayParams(C.Structure):
    """surf_display_params: exposure (mode, manual scale, the meter's key and limits), bloom, tone curve, transfer, dither."""
    _fields_ = [("exposure_mode", C.c_uint32), ("exposure", C.c_float), ("key", C.c_float), ("min_scale", C.c_float),
                ("max_scale", C.c_float), ("bloom_radius", C.c_uint32), ("bloom_threshold", C.c_float), ("bloom_strength", C.c_float),
                ("curve", C.c_uint32), ("white", C.c_float), ("transfer", C.c_uint32), ("dither", C.c_uint32)]


class DisplayMeterResult(C.Structure):
    """surf_display_meter_result: the luminance histogram (8 bins per octave from 2^-16), the pixels in it, those below it,
    the median's bin and the exposure scale applied."""
    _fields_ = [("hist", C.c_uint32 * 256), ("counted", C.c_uint32), ("black", C.c_uint32), ("median_bin", C.c_uint32),
                ("scale", C.c_float)]

    def as_dict(self) -> dict:
        return {"hist": np.array(self.hist, np.uint32), "counted": int(self.counted), "black": int(self.black),
                "median_bin": int(self.median_bin), "scale": np.float32(self.scale)}


class AovSampledParams(C.Structure):
    """surf_aov_sampled_params: the samples reduced per pixel, the frame index of the first, the matte's key."""
    _fields_ = [("samples", C.c_uint32), ("first_sample", C.c_uint32), ("key", C.c_uint32), ("reserved", C.c_uint32)]


class AoParams(C.Structure):
    """surf_ao_params: the rays per pixel, the index of the first, their length and origin offset, the source planes."""
    _fields_ = [("samples", C.c_uint32), ("first_sample", C.c_uint32), ("radius", C.c_float), ("bias", C.c_float),
                ("source", C.c_uint32), ("max_links", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class AtlasChart(C.Structure):
    """surf_atlas_chart (24 B): the instance whose mesh the chart maps, flags (bit 0: flip the normal), and where the mesh's
    uv lands in the atlas's [0,1]^2: uv * scale + offset."""
    _fields_ = [("instance", C.c_uint32), ("flags", C.c_uint32), ("scale", C.c_float * 2), ("offset", C.c_float * 2)]


class AtlasSummary(C.Structure):
    """surf_atlas_summary: texels with cover >= 1, texels with cover >= 2, the triangles skipped, the triangles of all charts."""
    _fields_ = [("covered", C.c_uint32), ("overlapped", C.c_uint32), ("skipped_triangles", C.c_uint32), ("triangles", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


_lib = None

# Byte sizes of the reference records (include/surf_hip.h static_asserts).
RECORD_BYTES = {"triangles": 64, "tri_ext": 80, "blas_indices": 4, "blas_nodes": 48, "materials": 64,
                "instances": 160, "tlas_indices": 4, "tlas_nodes": 48, "lights": 8, "background": 64}


def load() -> C.CDLL:
    """Loads libsurf_hip.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("SURF_HIP_LIB", LIB_PATH)   # tuning builds (make variants); still the HIP library
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `make -C surf-path-tracer_amd` or __graft_entry__.build()")
    lib = C.CDLL(path)
    P, U32, I32, F = C.c_void_p, C.c_uint32, C.c_int, C.c_float
    sig = {
        "surf_abi_version": ([], I32), "surf_device_count": ([C.POINTER(I32)], I32),
        "surf_create": ([I32, U32, U32, U32, U32, C.POINTER(P)], I32),
        "surf_create_sharded": ([I32, U32, U32, U32, U32, U32, C.POINTER(P)], I32),
        "surf_destroy": ([P], None), "surf_last_error": ([P], C.c_char_p),
        "surf_shard_rows": ([P, P, C.POINTER(U32)], I32), "surf_get_device": ([P, C.POINTER(I32)], I32),
        "surf_shard_row_list": ([U32, U32, U32, U32, P, C.POINTER(U32)], I32),
        "surf_pack_rgba8": ([P, U32, F, I32, P], I32),
        "surf_set_pool_capacity": ([P, U32], I32), "surf_set_frame_batch": ([P, U32], I32),
        "surf_set_profiling": ([P, I32], I32), "surf_set_zero_cutoff": ([P, I32], I32), "surf_set_trace_mode": ([P, I32], I32), "surf_set_tail_policy": ([P, U32, U32, U32], I32), "surf_set_tail_coop": ([P, U32], I32),
        "surf_debug_capped": ([P, P, U32, C.POINTER(C.c_uint64)], I32),
        "surf_debug_issue_order": ([P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], I32),
        "surf_debug_connect_staging": ([P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], I32),
        "surf_debug_kernel_selection": ([P] + [C.POINTER(C.c_uint32)] * 4, I32),
        "surf_debug_segment_cycles": ([P, P, U32, P], I32),
        "surf_debug_shadow_keys": ([P, U32, P, P, P, P, P, C.POINTER(U32), P], I32),
        "surf_debug_math": ([P, I32, U32, P, P], I32),
        "surf_debug_trace_paths": ([P, U32, P, P, P, U32, I32, P, P], I32),
        "surf_upload_scene": ([P, C.POINTER(SceneDesc)], I32),
        "surf_set_camera": ([P, P], I32),
        "surf_render": ([P, U32, U32, U32, U32], I32),
        "surf_clear_accumulator": ([P], I32), "surf_read_accumulator": ([P, P], I32),
        "surf_copy_accumulator_device": ([P, P], I32), "surf_finalize_rgba8": ([P, P], I32),
        "surf_get_stats": ([P, C.POINTER(Stats)], I32), "surf_synchronize": ([P], I32),
        "surf_trace_closest": ([P, U32, P, P, P, P, P, P, P], I32),
        "surf_trace_any": ([P, U32, P, P, P, P], I32),
        "surf_scene_build_indoor": ([C.c_char_p, I32, C.POINTER(P)], I32),
        "surf_scene_desc_get": ([P, C.POINTER(SceneDesc)], I32),
        "surf_scene_update": ([P, F], I32),
        "surf_update_instances": ([P, P, U32, P, P, U32, P, U32], I32),
        "surf_scene_camera": ([P, U32, U32, P], I32),
        "surf_scene_bvh_depths": ([P, C.POINTER(U32), C.POINTER(U32)], I32),
        "surf_scene_destroy": ([P], None),
        "surf_bvh_build": ([P, U32, U32, P, P, C.POINTER(U32)], I32),
        "surf_obj_load": ([C.c_char_p, U32, C.POINTER(P)], I32),
        "surf_write_ppm": ([C.c_char_p, U32, U32, P], I32), "surf_write_png": ([C.c_char_p, U32, U32, P], I32),
        "surf_display_rgba8": ([P, P], I32),
        "surf_read_aov": ([P, I32, P], I32), "surf_copy_aov_device": ([P, I32, P], I32),
        "surf_debug_aov_time": ([P, C.POINTER(F)], I32),
        "surf_read_aov_chain": ([P, I32, U32, P], I32), "surf_copy_aov_chain_device": ([P, I32, U32, P], I32),
        "surf_debug_aov_chain_time": ([P, C.POINTER(F)], I32),
        "surf_set_filter_guides": ([P, I32, U32], I32), "surf_get_filter_guides": ([P, C.POINTER(I32), C.POINTER(U32)], I32),
        "surf_aov_sampled_default_params": ([C.POINTER(AovSampledParams)], I32),
        "surf_read_aov_sampled": ([P, C.POINTER(AovSampledParams), I32, P], I32),
        "surf_copy_aov_sampled_device": ([P, C.POINTER(AovSampledParams), I32, P], I32),
        "surf_debug_aov_sampled_time": ([P, C.POINTER(F)], I32),
        "surf_set_filter_guides_sampled": ([P, C.POINTER(AovSampledParams)], I32),
        "surf_ao_default_params": ([C.POINTER(AoParams)], I32),
        "surf_read_ao": ([P, C.POINTER(AoParams), I32, P], I32),
        "surf_copy_ao_device": ([P, C.POINTER(AoParams), I32, P], I32),
        "surf_debug_ao_time": ([P, C.POINTER(F)], I32),
        "surf_write_pfm": ([C.c_char_p, U32, U32, P], I32),
        "surf_denoise_default_params": ([C.POINTER(DenoiseParams)], I32),
        "surf_denoise": ([P, C.POINTER(DenoiseParams), P], I32),
        "surf_denoise_copy_device": ([P, C.POINTER(DenoiseParams), P], I32),
        "surf_denoise_image": ([P, U32, U32, P, P, P, P, C.POINTER(DenoiseParams), P], I32),
        "surf_denoise_image_host": ([U32, U32, P, P, P, P, C.POINTER(DenoiseParams), P], I32),
        "surf_debug_denoise_time": ([P, C.POINTER(F), U32], I32),
        "surf_temporal_default_params": ([C.POINTER(TemporalParams)], I32),
        "surf_temporal_accumulate": ([P, C.POINTER(TemporalParams), C.POINTER(DenoiseParams), P], I32),
        "surf_temporal_copy_device": ([P, C.POINTER(TemporalParams), C.POINTER(DenoiseParams), P], I32),
        "surf_temporal_reset": ([P], I32), "surf_temporal_history": ([P, P], I32),
        "surf_temporal_image": ([P, U32, U32, C.POINTER(TemporalFrame), C.POINTER(TemporalPrev), C.POINTER(TemporalParams), P, P], I32),
        "surf_temporal_image_host": ([U32, U32, C.POINTER(TemporalFrame), C.POINTER(TemporalPrev), C.POINTER(TemporalParams), P, P], I32),
        "surf_debug_temporal_time": ([P, C.POINTER(F)], I32),
        "surf_svgf_default_params": ([C.POINTER(SvgfParams)], I32),
        "surf_svgf_accumulate": ([P, C.POINTER(TemporalParams), C.POINTER(SvgfParams), P], I32),
        "surf_svgf_copy_device": ([P, C.POINTER(TemporalParams), C.POINTER(SvgfParams), P], I32),
        "surf_svgf_moments": ([P, P], I32), "surf_svgf_variance": ([P, P], I32),
        "surf_svgf_image": ([P, U32, U32, C.POINTER(SvgfFrame), C.POINTER(SvgfPrev), C.POINTER(TemporalParams), C.POINTER(SvgfParams),
                             P, P, P, P], I32),
        "surf_svgf_image_host": ([U32, U32, C.POINTER(SvgfFrame), C.POINTER(SvgfPrev), C.POINTER(TemporalParams), C.POINTER(SvgfParams),
                                  P, P, P, P], I32),
        "surf_debug_svgf_time": ([P, C.POINTER(F), U32], I32),
        "surf_svgf_default_ext": ([C.POINTER(SvgfExt)], I32),
        "surf_svgf_accumulate_ex": ([P, C.POINTER(TemporalParams), C.POINTER(SvgfParams), C.POINTER(SvgfExt), P], I32),
        "surf_svgf_copy_device_ex": ([P, C.POINTER(TemporalParams), C.POINTER(SvgfParams), C.POINTER(SvgfExt), P], I32),
        "surf_svgf_image_ex": ([P, U32, U32, C.POINTER(SvgfFrame), C.POINTER(SvgfPrev), C.POINTER(TemporalParams), C.POINTER(SvgfParams),
                                C.POINTER(SvgfExt), P, P, P, P], I32),
        "surf_svgf_image_host_ex": ([U32, U32, C.POINTER(SvgfFrame), C.POINTER(SvgfPrev), C.POINTER(TemporalParams), C.POINTER(SvgfParams),
                                     C.POINTER(SvgfExt), P, P, P, P], I32),
        "surf_firefly_image": ([P, U32, U32, P, P, U32, F, P], I32),
        "surf_firefly_image_host": ([U32, U32, P, P, U32, F, P], I32),
        "surf_debug_firefly_time": ([P, C.POINTER(F)], I32),
        "surf_set_sample_squares": ([P, I32], I32), "surf_read_sample_squares": ([P, P], I32),
        "surf_copy_sample_squares_device": ([P, P], I32),
        "surf_denoise_sampled": ([P, C.POINTER(SvgfParams), P], I32),
        "surf_denoise_sampled_copy_device": ([P, C.POINTER(SvgfParams), P], I32),
        "surf_denoise_sampled_image": ([P, U32, U32, P, P, P, P, P, C.POINTER(SvgfParams), P, P], I32),
        "surf_denoise_sampled_image_host": ([U32, U32, P, P, P, P, P, C.POINTER(SvgfParams), P, P], I32),
        "surf_debug_sampled_time": ([P, C.POINTER(F), U32], I32),
        "surf_noise_default_params": ([C.POINTER(NoiseParams)], I32),
        "surf_noise_estimate": ([P, C.POINTER(NoiseParams), P, C.POINTER(NoiseSummary)], I32),
        "surf_noise_image": ([P, U32, P, P, C.POINTER(NoiseParams), P, C.POINTER(NoiseSummary)], I32),
        "surf_noise_image_host": ([U32, P, P, C.POINTER(NoiseParams), P, C.POINTER(NoiseSummary)], I32),
        "surf_set_pixel_mask": ([P, P], I32), "surf_get_pixel_mask": ([P, P, C.POINTER(U32)], I32),
        "surf_set_surfel_sensor": ([P, P, P], I32), "surf_set_surfel_sensor_device": ([P, P, P], I32),
        "surf_get_sensor": ([P, C.POINTER(I32), C.POINTER(U32)], I32),
        "surf_adaptive_default_mask_params": ([C.POINTER(AdaptiveMaskParams)], I32),
        "surf_adaptive_default_params": ([C.POINTER(AdaptiveParams)], I32),
        "surf_mask_from_noise": ([P, C.POINTER(AdaptiveMaskParams), C.POINTER(U32)], I32),
        "surf_adaptive_mask_image": ([P, U32, U32, P, P, C.POINTER(AdaptiveMaskParams), P, P, C.POINTER(U32)], I32),
        "surf_adaptive_mask_image_host": ([U32, U32, P, P, C.POINTER(AdaptiveMaskParams), P, P, C.POINTER(U32)], I32),
        "surf_render_adaptive": ([P, C.POINTER(AdaptiveParams), P, U32, C.POINTER(AdaptiveSummary)], I32),
        "surf_finalize_rgba8_weighted": ([P, I32, P], I32), "surf_pack_rgba8_weighted": ([P, U32, I32, P], I32),
        "surf_set_sample_buckets": ([P, U32], I32), "surf_get_sample_buckets": ([P, C.POINTER(U32)], I32),
        "surf_read_sample_buckets": ([P, P], I32), "surf_copy_sample_buckets_device": ([P, P], I32),
        "surf_robust_default_params": ([C.POINTER(RobustParams)], I32),
        "surf_robust_accumulator": ([P, C.POINTER(RobustParams), P, P, C.POINTER(RobustSummary)], I32),
        "surf_robust_copy_device": ([P, C.POINTER(RobustParams), P], I32),
        "surf_robust_image": ([P, U32, U32, P, P, C.POINTER(RobustParams), P, P, C.POINTER(RobustSummary)], I32),
        "surf_robust_image_host": ([U32, U32, P, P, C.POINTER(RobustParams), P, P, C.POINTER(RobustSummary)], I32),
        "surf_debug_robust_time": ([P, C.POINTER(F)], I32),
        "surf_nlm_default_params": ([C.POINTER(NlmParams)], I32),
        "surf_denoise_nlm": ([P, C.POINTER(NlmParams), P, P], I32),
        "surf_denoise_nlm_copy_device": ([P, C.POINTER(NlmParams), P, P], I32),
        "surf_denoise_nlm_image": ([P, U32, U32, P, P, C.POINTER(NlmParams), P, P], I32),
        "surf_denoise_nlm_image_host": ([U32, U32, P, P, C.POINTER(NlmParams), P, P], I32),
        "surf_debug_nlm_time": ([P, C.POINTER(F), U32], I32),
        "surf_regress_default_params": ([C.POINTER(RegressParams)], I32),
        "surf_denoise_regress": ([P, C.POINTER(RegressParams), P, P], I32),
        "surf_denoise_regress_copy_device": ([P, C.POINTER(RegressParams), P, P], I32),
        "surf_denoise_regress_image": ([P, U32, U32, P, P, P, P, P, C.POINTER(RegressParams), P, P], I32),
        "surf_denoise_regress_image_host": ([U32, U32, P, P, P, P, P, C.POINTER(RegressParams), P, P], I32),
        "surf_debug_regress_time": ([P, C.POINTER(F), U32], I32),
        "surf_error_mask_default_params": ([C.POINTER(ErrorMaskParams)], I32),
        "surf_error_mask_image": ([P, U32, U32, P, P, P, C.POINTER(ErrorMaskParams), P, P, C.POINTER(U32)], I32),
        "surf_error_mask_image_host": ([U32, U32, P, P, P, C.POINTER(ErrorMaskParams), P, P, C.POINTER(U32)], I32),
        "surf_mask_from_nlm": ([P, C.POINTER(NlmParams), C.POINTER(ErrorMaskParams), C.POINTER(U32)], I32),
        "surf_debug_error_mask_time": ([P, C.POINTER(F), U32], I32),
        "surf_adaptive_nlm_default_params": ([C.POINTER(AdaptiveNlmParams)], I32),
        "surf_render_adaptive_nlm": ([P, C.POINTER(AdaptiveNlmParams), P, P, P, U32, C.POINTER(AdaptiveNlmSummary)], I32),
        "surf_render_adaptive_nlm_copy_device": ([P, C.POINTER(AdaptiveNlmParams), P, P, P, U32, C.POINTER(AdaptiveNlmSummary)], I32),
        "surf_display_default_params": ([C.POINTER(DisplayParams)], I32),
        "surf_display": ([P, C.POINTER(DisplayParams), P, C.POINTER(DisplayMeterResult)], I32),
        "surf_display_image": ([P, U32, U32, P, C.POINTER(DisplayParams), P, C.POINTER(DisplayMeterResult)], I32),
        "surf_display_image_device": ([P, U32, U32, P, C.POINTER(DisplayParams), P, C.POINTER(DisplayMeterResult)], I32),
        "surf_display_image_host": ([U32, U32, P, C.POINTER(DisplayParams), P, C.POINTER(DisplayMeterResult)], I32),
        "surf_display_srgb_table": ([P], I32), "surf_display_bayer8": ([P], I32),
        "surf_debug_display_time": ([P, C.POINTER(F), U32], I32),
        "surf_atlas_build": ([P, C.POINTER(SceneDesc), P, U32, U32, U32, P, P, P, P, C.POINTER(AtlasSummary)], I32),
        "surf_atlas_build_device": ([P, C.POINTER(SceneDesc), P, U32, U32, U32, P, P, P, P, C.POINTER(AtlasSummary)], I32),
        "surf_atlas_build_host": ([C.POINTER(SceneDesc), P, U32, U32, U32, P, P, P, P, C.POINTER(AtlasSummary)], I32),
        "surf_atlas_grid_charts": ([U32, P, U32, U32, U32, P], I32),
        "surf_atlas_finish": ([P, U32, U32, P, P, P, P], I32), "surf_atlas_finish_device": ([P, U32, U32, P, P, P, P], I32),
        "surf_atlas_finish_host": ([U32, U32, P, P, P, P], I32),
        "surf_atlas_dilate": ([P, U32, U32, P, P, U32, P, P], I32), "surf_atlas_dilate_device": ([P, U32, U32, P, P, U32, P, P], I32),
        "surf_atlas_dilate_host": ([U32, U32, P, P, U32, P, P], I32),
        "surf_atlas_bake": ([P, C.POINTER(SceneDesc), P, U32, U32, U32, U32, U32, U32, P, P, P, C.POINTER(AtlasSummary)], I32),
        "surf_debug_atlas_time": ([P, C.POINTER(F), U32, C.POINTER(U32)], I32),
        "surf_mesh_data": ([P, C.POINTER(P), C.POINTER(P), C.POINTER(U32)], I32),
        "surf_mesh_destroy": ([P], None),
        "surf_ref_sinf": ([F], F), "surf_ref_cosf": ([F], F), "surf_ref_expf": ([F], F),
        "surf_debug_math_host": ([I32, U32, P, P], I32),
    }
    for name, (args, res) in sig.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # a library variant built before a diagnostics entry point existed
            # (tools/ab.sh SURF_HIP_LIB=...); tests/test_abi.py checks the product exports all
            if name.startswith("surf_debug_") and os.environ.get("SURF_HIP_LIB"):
                continue
            raise
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


_mgpu = None


def load_mgpu() -> C.CDLL:
    """Loads libsurf_mgpu.so (include/surf_mgpu.h: the RCCL gather and the row
    un-permute of a multi-GPU render); raises if it has not been built."""
    global _mgpu
    if _mgpu is not None:
        return _mgpu
    load()
    if not os.path.exists(MGPU_LIB_PATH):
        raise FileNotFoundError(f"{MGPU_LIB_PATH} not built: run `make -C surf-path-tracer_amd`")
    lib = C.CDLL(MGPU_LIB_PATH)
    P, U32, I32 = C.c_void_p, C.c_uint32, C.c_int
    sig = {
        "surf_mgpu_unique_id": ([P], I32),
        "surf_mgpu_create": ([P, U32, U32, U32, U32, U32, P, C.POINTER(P)], I32),
        "surf_mgpu_create_all": ([P, U32, U32, U32, U32, P], I32),
        "surf_mgpu_gather": ([P, P], I32), "surf_mgpu_gather_all": ([P, U32, P], I32),
        "surf_mgpu_destroy": ([P], None), "surf_mgpu_last_error": ([], C.c_char_p),
        "surf_mgpu_assemble": ([U32, U32, U32, U32, P, U32, P], I32),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _mgpu = lib
    return lib


def assemble_slabs(width: int, height: int, shards: int, row_block: int, gathered: np.ndarray) -> np.ndarray:
    """The root's row un-permute of a multi-GPU gather, by libsurf_mgpu's native
    code (surf_mgpu_assemble): gathered is (shards, rows_per_slab, W, 4) float32,
    slab k holding shard k's rows in shard order (padding rows ignored)."""
    g = np.ascontiguousarray(gathered, dtype=np.float32)
    if g.ndim != 4 or g.shape[0] != shards or g.shape[2] != width or g.shape[3] != 4:
        raise ValueError(f"gathered shape {g.shape} is not ({shards}, rows, {width}, 4)")
    out = np.zeros((height, width, 4), np.float32)
    try:
        mg = load_mgpu()
    except OSError:
        # libsurf_mgpu.so (it links RCCL) not built or not loadable: the same
        # un-permute on the host in numpy -- a torch.distributed gather does not need RCCL's library
        for k in range(shards):
            rows = shard_rows(height, ShardSpec(k, shards, row_block))
            if len(rows) > g.shape[1]:
                raise ValueError(f"slab smaller than shard {k}")
            out[rows] = g[k, :len(rows)]
        return out
    rc = mg.surf_mgpu_assemble(width, height, shards, row_block, g.ctypes.data, g.shape[1], out.ctypes.data)
    if rc != SURF_OK:
        raise SurfError(rc, "surf_mgpu_assemble", mg.surf_mgpu_last_error().decode())
    return out


def pack_rgba8(acc: np.ndarray, samples: int, display: bool = False) -> np.ndarray:
    """surf_finalize_rgba8 / surf_display_rgba8 of a host accumulator (surf_pack_rgba8)."""
    a = np.ascontiguousarray(acc, dtype=np.float32).reshape(-1, 4)
    out = np.zeros(len(a), np.uint32)
    _check(load().surf_pack_rgba8(a.ctypes.data, len(a), np.float32(1.0) / np.float32(samples), 1 if display else 0,
                                  out.ctypes.data), "surf_pack_rgba8")
    return out


def pack_rgba8_weighted(acc: np.ndarray, display: bool = False) -> np.ndarray:
    """surf_finalize_rgba8_weighted of a host accumulator (surf_pack_rgba8_weighted): each pixel divided by its own w."""
    a = np.ascontiguousarray(acc, dtype=np.float32).reshape(-1, 4)
    out = np.zeros(len(a), np.uint32)
    _check(load().surf_pack_rgba8_weighted(a.ctypes.data, len(a), 1 if display else 0, out.ctypes.data), "surf_pack_rgba8_weighted")
    return out


def _check(rc: int, what: str, ctx=None):
    if rc != SURF_OK:
        detail = load().surf_last_error(ctx)
        raise SurfError(rc, what, detail.decode() if detail else "")


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def device_count() -> int:
    n = C.c_int(0)
    rc = load().surf_device_count(C.byref(n))
    return n.value if rc == SURF_OK else 0


class Scene:
    """Host scene built by the product's C++ host API (OBJ -> BVH -> GPUBatcher layout)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def indoor(cls, assets_dir: str = ASSETS_DIR, variant: int = 0) -> "Scene":
        h = C.c_void_p()
        _check(load().surf_scene_build_indoor(assets_dir.encode(), variant, C.byref(h)), "surf_scene_build_indoor")
        return cls(h)

    @property
    def handle(self):
        return self._h

    def update(self, delta_time: float):
        """GPUScene::update (scene.cpp:267-282): rotate instance 3, refit the TLAS, re-batch."""
        _check(load().surf_scene_update(self._h, delta_time), "surf_scene_update")

    def desc(self) -> SceneDesc:
        d = SceneDesc()
        _check(load().surf_scene_desc_get(self._h, C.byref(d)), "surf_scene_desc_get")
        return d

    def camera(self, width: int, height: int) -> bytes:
        ubo = CameraUBO()
        _check(load().surf_scene_camera(self._h, width, height, ubo), "surf_scene_camera")
        return bytes(ubo)

    def bvh_depths(self) -> tuple[int, int]:
        t, b = C.c_uint32(), C.c_uint32()
        _check(load().surf_scene_bvh_depths(self._h, C.byref(t), C.byref(b)), "surf_scene_bvh_depths")
        return t.value, b.value

    def buffers(self) -> dict[str, bytes]:
        """The ten reference-layout buffers of the GPUScene, as bytes."""
        d = self.desc()
        counts = {"triangles": d.triangle_count, "tri_ext": d.triangle_count, "blas_indices": d.blas_index_count,
                  "blas_nodes": d.blas_node_count, "materials": d.material_count, "instances": d.instance_count,
                  "tlas_indices": d.instance_count, "tlas_nodes": d.tlas_node_count, "lights": d.light_count,
                  "background": 1}
        out = {}
        for k, n in counts.items():
            ptr = getattr(d, k)
            out[k] = C.string_at(ptr, n * RECORD_BYTES[k]) if n else b""
        return out

    def close(self):
        if self._h:
            load().surf_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_image(path: str, rgba8: np.ndarray) -> None:
    """Writes an (H, W) uint32 RGBA8 image (R in the low byte) as PNG or, for a
    .ppm path, binary PPM (alpha dropped)."""
    img = np.ascontiguousarray(rgba8, dtype=np.uint32)
    h, w = img.shape
    fn = load().surf_write_ppm if path.lower().endswith(".ppm") else load().surf_write_png
    _check(fn(path.encode(), w, h, _ptr(img)), "surf_write_image")


def write_pfm(path: str, rgba: np.ndarray) -> None:
    """Writes an (H, W, 4) float32 image, rows top to bottom (the accumulator, a
    float feature plane of Renderer.aov()), as a colour PFM (surf_write_pfm:
    rows bottom to top, RGB as little-endian f32 bit for bit, alpha dropped)."""
    img = np.ascontiguousarray(rgba, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 4:
        raise ValueError(f"rgba shape {img.shape} is not (H, W, 4)")
    h, w = img.shape[:2]
    _check(load().surf_write_pfm(path.encode(), w, h, _ptr(img)), "surf_write_pfm")


AOV_PLANES = ("position", "normal", "albedo", "id")      # surf_aov order
AOV_CHAIN_MAX_LINKS = 16                                 # SURF_AOV_CHAIN_MAX_LINKS
FILTER_GUIDES = ("first_hit", "chain")                   # surf_guides order
FILTER_GUIDES_SAMPLED = "sampled"                        # SURF_GUIDES_SAMPLED (2), set through surf_set_filter_guides_sampled
AOVS_PLANES = ("position", "normal", "albedo", "id", "matte_key", "matte_count")   # surf_aovs order
AOVS_MAX_SAMPLES = 64                                    # SURF_AOVS_MAX_SAMPLES
MATTE_KEYS = ("instance", "material")                    # surf_matte_key order
MATTE_MISS = 0xFFFFFFFF                                  # the key of a sample that missed, and of an empty rank


def aov_sampled_params(samples=16, first_sample=0, key="instance") -> AovSampledParams:
    """surf_aov_sampled_params, checked before the library sees them."""
    if key not in MATTE_KEYS:
        raise ValueError(f"matte key {key!r}: one of {MATTE_KEYS}")
    n, f = int(samples), int(first_sample)
    if n != samples or not 1 <= n <= AOVS_MAX_SAMPLES:
        raise ValueError(f"samples {samples!r}: an integer in 1..{AOVS_MAX_SAMPLES}")
    if f != first_sample or not 0 <= f <= 0xFFFFFFFF:
        raise ValueError(f"first_sample {first_sample!r}: an unsigned 32-bit integer")
    return AovSampledParams(n, f, MATTE_KEYS.index(key), 0)


MATH_OPS = ("expf", "sinf", "cosf", "sincosf")           # surf_math_op order
AO_PLANES = ("openness", "bits")                         # surf_ao_plane order
AO_SOURCES = ("first_hit", "chain")                      # surf_ao_source order
AO_SAMPLES = (1, 2, 4, 8, 16, 32, 64)                    # a pixel's rays fill an aligned lane group of a wave


def ao_params(samples=16, radius=1.0, first_sample=0, bias=1e-5, source="first_hit", max_links=8) -> AoParams:
    """surf_ao_params, checked before the library sees them."""
    if source not in AO_SOURCES:
        raise ValueError(f"source {source!r}: one of {AO_SOURCES}")
    if isinstance(samples, bool) or samples not in AO_SAMPLES:
        raise ValueError(f"samples {samples!r}: one of {AO_SAMPLES}")
    f, links = int(first_sample), int(max_links)
    if f != first_sample or not 0 <= f <= 0xFFFFFFFF:
        raise ValueError(f"first_sample {first_sample!r}: an unsigned 32-bit integer")
    if links != max_links or not 0 <= links <= AOV_CHAIN_MAX_LINKS:
        raise ValueError(f"max_links {max_links!r}: an integer in 0..{AOV_CHAIN_MAX_LINKS}")
    rad, b = np.float32(radius), np.float32(bias)
    if not rad > 0.0:                                    # NaN fails every comparison
        raise ValueError(f"radius {radius!r}: above 0 (inf allowed)")
    if not b >= 0.0:
        raise ValueError(f"bias {bias!r}: 0 or above")
    return AoParams(int(samples), f, float(rad), float(b), AO_SOURCES.index(source), links, (C.c_uint32 * 2)(0, 0))


def matte_coverage(keys, counts, key: int, samples: int) -> np.ndarray:
    """The coverage of one key from Renderer.aov_sampled()'s 'matte_key' and
    'matte_count' planes: (H, W) float32, the key's count / samples where one
    of the pixel's four ranks holds it (with a count above 0: an empty rank is
    MATTE_MISS with count 0), else 0.  key = MATTE_MISS gives the share of the
    samples that missed."""
    keys, counts = np.asarray(keys, np.uint32), np.asarray(counts, np.uint32)
    if keys.ndim != 3 or keys.shape[2] != 4 or counts.shape != keys.shape:
        raise ValueError(f"matte planes {keys.shape} and {counts.shape} are not two (H, W, 4) images of one size")
    if int(samples) < 1:
        raise ValueError(f"samples {samples!r}: at least 1")
    hits = np.where(keys == np.uint32(key), counts, np.uint32(0)).sum(axis=2, dtype=np.uint32)
    return hits.astype(np.float32) / np.float32(samples)


def _chain_links(max_links) -> int:
    """max_links of the chain planes, checked before the library sees it."""
    n = int(max_links)
    if n != max_links or not 0 <= n <= AOV_CHAIN_MAX_LINKS:
        raise ValueError(f"max_links {max_links!r}: an integer in 0..{AOV_CHAIN_MAX_LINKS}")
    return n


def denoise_params(**params) -> DenoiseParams:
    """surf_denoise_default_params (5 iterations, sigma_color 1.0, sigma_normal
    0.3, sigma_plane 0.1, demodulate 1) with the given fields replaced."""
    p = DenoiseParams()
    _check(load().surf_denoise_default_params(C.byref(p)), "surf_denoise_default_params")
    for k, v in params.items():
        if k not in ("iterations", "sigma_color", "sigma_normal", "sigma_plane", "demodulate"):
            raise TypeError(f"unknown denoise parameter {k!r}")
        setattr(p, k, int(v) if k in ("iterations", "demodulate") else float(v))
    return p


def _denoise_planes(acc, planes):
    """(w, h, [acc, position, normal, albedo]) as contiguous (H, W, 4) float32; planes
    is Renderer.aov()'s dict (the id plane is not needed) or a (position, normal, albedo) sequence."""
    if isinstance(planes, dict):
        planes = [planes[k] for k in ("position", "normal", "albedo")]
    arrs = [np.ascontiguousarray(a, dtype=np.float32) for a in (acc, *planes)]
    if len(arrs) != 4 or arrs[0].ndim != 3 or arrs[0].shape[2] != 4 or any(a.shape != arrs[0].shape for a in arrs):
        raise ValueError(f"denoise planes {[a.shape for a in arrs]} are not four (H, W, 4) images of one size")
    h, w = arrs[0].shape[:2]
    return w, h, arrs


def denoise_image_host(acc: np.ndarray, planes, **params) -> np.ndarray:
    """The CPU twin of Renderer.denoise_image (surf_denoise_image_host): the
    same per-pixel functions compiled for the host, bit-identical; no device."""
    w, h, a = _denoise_planes(acc, planes)
    p = denoise_params(**params)
    out = np.zeros((h, w, 4), np.float32)
    _check(load().surf_denoise_image_host(w, h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), C.byref(p), _ptr(out)),
           "surf_denoise_image_host")
    return out


def temporal_params(**params) -> TemporalParams:
    """surf_temporal_default_params (alpha_min 0, max_history 32, normal_min 0.9,
    plane_tol 0.01, snap 1/64, min_weight 0.01) with the given fields replaced."""
    p = TemporalParams()
    _check(load().surf_temporal_default_params(C.byref(p)), "surf_temporal_default_params")
    for k, v in params.items():
        if k not in ("alpha_min", "max_history", "normal_min", "plane_tol", "snap", "min_weight"):
            raise TypeError(f"unknown temporal parameter {k!r}")
        setattr(p, k, int(v) if k == "max_history" else float(v))
    return p


def _spatial_params(spatial):
    """None, True (the denoiser's defaults) or a dict of denoiser parameters -> DenoiseParams or None."""
    if spatial is None or spatial is False:
        return None
    return denoise_params(**({} if spatial is True else spatial))


def _temporal_frames(cur, prev):
    """(w, h, TemporalFrame, TemporalPrev or None, the arrays they point into).  cur: a
    dict with 'acc', 'position', 'normal' ((H, W, 4) float32), 'id' ((H, W, 4) uint32)
    and 'instances' (the surf_gpu_instance records as bytes, Scene.buffers()['instances']);
    prev: None for a first frame, or a dict with 'history', 'position', 'normal',
    'id', 'instances' and 'camera' (the 128-byte camera UBO)."""
    def planes(d, first):
        arrs = [np.ascontiguousarray(d[k], dtype=np.float32) for k in (first, "position", "normal")]
        arrs.append(np.ascontiguousarray(d["id"], dtype=np.uint32))
        inst = np.frombuffer(bytes(d.get("instances", b"")), np.uint8).copy()
        if len(inst) % RECORD_BYTES["instances"]:
            raise ValueError(f"instances: {len(inst)} bytes are no multiple of {RECORD_BYTES['instances']}")
        return arrs, inst
    ca, ci = planes(cur, "acc")
    if ca[0].ndim != 3 or ca[0].shape[2] != 4 or any(a.shape != ca[0].shape for a in ca):
        raise ValueError(f"temporal planes {[a.shape for a in ca]} are not four (H, W, 4) images of one size")
    h, w = ca[0].shape[:2]
    f = TemporalFrame(*[_ptr(a) for a in ca], _ptr(ci) if len(ci) else None, len(ci) // RECORD_BYTES["instances"], 0)
    keep = [ca, ci]
    q = None
    if prev is not None:
        pa, pi = planes(prev, "history")
        if any(a.shape != ca[0].shape for a in pa):
            raise ValueError(f"previous planes {[a.shape for a in pa]} differ from the current frame's {ca[0].shape}")
        if len(prev["camera"]) != C.sizeof(CameraUBO):
            raise ValueError(f"camera UBO is {len(prev['camera'])} bytes, not {C.sizeof(CameraUBO)}")
        q = TemporalPrev(*[_ptr(a) for a in pa], _ptr(pi) if len(pi) else None, len(pi) // RECORD_BYTES["instances"], 0,
                         CameraUBO.from_buffer_copy(prev["camera"]))
        keep += [pa, pi]
    return w, h, f, q, keep


def temporal_image_host(cur, prev, **params):
    """The CPU twin of Renderer.temporal_image (surf_temporal_image_host): the same
    per-pixel function compiled for the host, bit-identical; no device.
    Returns (out, history), each (H, W, 4) float32."""
    w, h, f, q, _keep = _temporal_frames(cur, prev)
    p = temporal_params(**params)
    out, hist = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    _check(load().surf_temporal_image_host(w, h, C.byref(f), C.byref(q) if q is not None else None, C.byref(p), _ptr(out), _ptr(hist)),
           "surf_temporal_image_host")
    return out, hist


_TEMPORAL_FIELDS = ("alpha_min", "max_history", "normal_min", "plane_tol", "snap", "min_weight")
_SVGF_FIELDS = ("iterations", "sigma_lum", "sigma_normal", "sigma_plane", "demodulate", "spatial_below", "variance_eps")


def svgf_params(**params) -> SvgfParams:
    """surf_svgf_default_params (5 iterations, sigma_lum 4.0, sigma_normal 0.3,
    sigma_plane 0.1, demodulate 1, spatial_below 4, variance_eps 1e-10) with the
    given fields replaced."""
    p = SvgfParams()
    _check(load().surf_svgf_default_params(C.byref(p)), "surf_svgf_default_params")
    for k, v in params.items():
        if k not in _SVGF_FIELDS:
            raise TypeError(f"unknown svgf parameter {k!r}")
        setattr(p, k, int(v) if k in ("iterations", "demodulate", "spatial_below") else float(v))
    return p


def _svgf_split(params):
    """One keyword set -> (TemporalParams, SvgfParams): the temporal accumulation's names and the filter's do not overlap."""
    unknown = [k for k in params if k not in _TEMPORAL_FIELDS + _SVGF_FIELDS]
    if unknown:
        raise TypeError(f"unknown svgf parameter {unknown[0]!r}")
    return (temporal_params(**{k: v for k, v in params.items() if k in _TEMPORAL_FIELDS}),
            svgf_params(**{k: v for k, v in params.items() if k in _SVGF_FIELDS}))


def svgf_ext(firefly_scale=0.0, feedback=False) -> SvgfExt:
    """surf_svgf_default_ext (everything off) with the given fields replaced."""
    x = SvgfExt()
    _check(load().surf_svgf_default_ext(C.byref(x)), "surf_svgf_default_ext")
    x.firefly_scale, x.feedback = float(firefly_scale), int(feedback)
    return x


def _svgf_ext(params):
    """Takes 'ext' (a SvgfExt, or None for a NULL ext) or 'firefly_scale' / 'feedback' out of a
    keyword set: (the rest, whether any was given, the ext argument for C).  With none of the
    three given the caller takes the entry point without _ex."""
    rest = {k: v for k, v in params.items() if k not in ("ext", "firefly_scale", "feedback")}
    if len(rest) == len(params):
        return rest, False, None
    if "ext" in params:
        if len(params) - len(rest) > 1:
            raise TypeError("give either ext or firefly_scale / feedback")
        if params["ext"] is not None and not isinstance(params["ext"], SvgfExt):
            raise TypeError("ext is not a SvgfExt")
        return rest, True, C.byref(params["ext"]) if params["ext"] is not None else None
    return rest, True, C.byref(svgf_ext(params.get("firefly_scale", 0.0), params.get("feedback", False)))


def _firefly_planes(acc, albedo):
    a, alb = (np.ascontiguousarray(v, dtype=np.float32) for v in (acc, albedo))
    if a.ndim != 3 or a.shape[2] != 4 or alb.shape != a.shape:
        raise ValueError(f"firefly planes {a.shape}, {alb.shape} are not two (H, W, 4) images of one size")
    return a, alb, np.zeros_like(a)


def firefly_image_host(acc, albedo, scale, demodulate=True) -> np.ndarray:
    """The CPU twin of Renderer.firefly_image (surf_firefly_image_host): the clamped
    accumulator A' = (c', 1), (H, W, 4) float32; bit-identical, no device."""
    a, alb, out = _firefly_planes(acc, albedo)
    _check(load().surf_firefly_image_host(a.shape[1], a.shape[0], _ptr(a), _ptr(alb), int(bool(demodulate)), float(scale), _ptr(out)),
           "surf_firefly_image_host")
    return out


def _svgf_frames(cur, prev):
    """(w, h, SvgfFrame, SvgfPrev or None, the arrays they point into): _temporal_frames' dicts,
    cur with 'albedo' ((H, W, 4) float32) and prev with 'moments' (None or absent: no moments stored)."""
    w, h, f, q, keep = _temporal_frames(cur, prev)
    alb = np.ascontiguousarray(cur["albedo"], dtype=np.float32)
    if alb.shape != (h, w, 4):
        raise ValueError(f"albedo plane {alb.shape} is not ({h}, {w}, 4)")
    sf = SvgfFrame(*[getattr(f, k) for k, _ in TemporalFrame._fields_], _ptr(alb))
    keep.append(alb)
    sq = None
    if q is not None:
        mom = prev.get("moments")
        if mom is not None:
            mom = np.ascontiguousarray(mom, dtype=np.float32)
            if mom.shape != (h, w, 4):
                raise ValueError(f"moments plane {mom.shape} is not ({h}, {w}, 4)")
            keep.append(mom)
        sq = SvgfPrev(*[getattr(q, k) for k, _ in TemporalPrev._fields_], _ptr(mom) if mom is not None else None)
    return w, h, sf, sq, keep


def svgf_image_host(cur, prev, **params):
    """The CPU twin of Renderer.svgf_image (surf_svgf_image_host): the same per-pixel
    functions compiled for the host, bit-identical; no device.  Returns (out,
    history, moments, variance), each (H, W, 4) float32.  firefly_scale=, feedback=
    or ext= (a SvgfExt or None) go through surf_svgf_image_host_ex."""
    params, ex, x = _svgf_ext(params)
    p, sp = _svgf_split(params)
    w, h, f, q, _keep = _svgf_frames(cur, prev)
    res = [np.zeros((h, w, 4), np.float32) for _ in range(4)]
    args = (w, h, C.byref(f), C.byref(q) if q is not None else None, C.byref(p), C.byref(sp))
    if ex:
        _check(load().surf_svgf_image_host_ex(*args, x, *[_ptr(a) for a in res]), "surf_svgf_image_host_ex")
    else:
        _check(load().surf_svgf_image_host(*args, *[_ptr(a) for a in res]), "surf_svgf_image_host")
    return tuple(res)


def _sampled_params(params) -> SvgfParams:
    """svgf_params for the sample-variance-guided filter: spatial_below is ignored there and not accepted."""
    if "spatial_below" in params:
        raise TypeError("the sample-variance-guided filter has no spatial_below")
    return svgf_params(**params)


def _sampled_planes(acc, squares, planes):
    """(w, h, [acc, squares, position, normal, albedo]) as contiguous (H, W, 4) float32; planes as _denoise_planes takes them."""
    w, h, a = _denoise_planes(acc, planes)
    q = np.ascontiguousarray(squares, dtype=np.float32)
    if q.shape != a[0].shape:
        raise ValueError(f"squares plane {q.shape} is not {a[0].shape}")
    return w, h, [a[0], q, a[1], a[2], a[3]]


def denoise_sampled_image_host(acc, squares, planes, **params):
    """The CPU twin of Renderer.denoise_sampled_image (surf_denoise_sampled_image_host):
    bit-identical, no device.  Returns (out, variance), each (H, W, 4) float32."""
    w, h, a = _sampled_planes(acc, squares, planes)
    p = _sampled_params(params)
    out, var = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
    _check(load().surf_denoise_sampled_image_host(w, h, *[_ptr(x) for x in a], C.byref(p), _ptr(out), _ptr(var)),
           "surf_denoise_sampled_image_host")
    return out, var


def noise_params(threshold=None, floor=None) -> NoiseParams:
    """surf_noise_default_params (threshold 0.05, floor 0.01) with the given fields replaced."""
    p = NoiseParams()
    _check(load().surf_noise_default_params(C.byref(p)), "surf_noise_default_params")
    if threshold is not None:
        p.threshold = float(threshold)
    if floor is not None:
        p.floor = float(floor)
    return p


def _noise_planes(acc, squares):
    a, q = (np.ascontiguousarray(v, dtype=np.float32) for v in (acc, squares))
    if a.ndim < 2 or a.shape[-1] != 4 or q.shape != a.shape:
        raise ValueError(f"noise planes {a.shape}, {q.shape} are not two (..., 4) images of one size")
    return a, q, np.zeros(a.shape[:-1], np.float32)


def noise_image_host(acc, squares, threshold=None, floor=None):
    """The CPU twin of Renderer.noise_image (surf_noise_image_host): (error image,
    summary dict) of planes of any shape (..., 4); bit-identical, no device."""
    a, q, err = _noise_planes(acc, squares)
    p, s = noise_params(threshold, floor), NoiseSummary()
    _check(load().surf_noise_image_host(err.size, _ptr(a), _ptr(q), C.byref(p), _ptr(err), C.byref(s)), "surf_noise_image_host")
    return err, s.as_dict()


def robust_params(trim_scale=None) -> RobustParams:
    """surf_robust_default_params (trim_scale 1.0) with the given field replaced."""
    p = RobustParams()
    _check(load().surf_robust_default_params(C.byref(p)), "surf_robust_default_params")
    if trim_scale is not None:
        p.trim_scale = float(trim_scale)
    return p


def _robust_planes(acc, buckets):
    """(npx, M, acc, buckets, out, trim): acc of any shape (..., 4), buckets (M, ..., 4), contiguous float32."""
    a, b = (np.ascontiguousarray(v, dtype=np.float32) for v in (acc, buckets))
    if a.ndim < 2 or a.shape[-1] != 4 or b.shape[1:] != a.shape:
        raise ValueError(f"robust planes {a.shape}, {b.shape} are not an (..., 4) image and its (M, ..., 4) buckets")
    return a.size // 4, b.shape[0], a, b, np.zeros_like(a), np.zeros(a.shape[:-1], np.uint8)


def robust_image_host(acc, buckets, trim_scale=None):
    """The CPU twin of robust_image (surf_robust_image_host): (accumulator plane, trim image, summary dict) of an
    accumulator of any shape (..., 4) and its (M, ..., 4) bucket planes; bit-identical, no device."""
    npx, m, a, b, out, trim = _robust_planes(acc, buckets)
    p, s = robust_params(trim_scale), RobustSummary()
    _check(load().surf_robust_image_host(npx, m, _ptr(a), _ptr(b), C.byref(p), _ptr(out), _ptr(trim), C.byref(s)), "surf_robust_image_host")
    return out, trim, s.as_dict()


def robust_image(renderer, acc, buckets, trim_scale=None):
    """The robust estimate on the renderer's device of host planes (surf_robust_image), e.g. planes assembled from row
    shards: (accumulator plane, trim image, summary dict)."""
    return renderer.robust_image(acc, buckets, trim_scale)


def nlm_params(**params) -> NlmParams:
    """surf_nlm_default_params (search_radius 5, patch_radius 2, k 0.45, alpha 1.0, eps 1e-10) with the given fields replaced."""
    p = NlmParams()
    _check(load().surf_nlm_default_params(C.byref(p)), "surf_nlm_default_params")
    for name, v in params.items():
        if name not in ("search_radius", "patch_radius", "k", "alpha", "eps"):
            raise TypeError(f"surf_nlm_params has no field {name!r}")
        setattr(p, name, int(v) if name.endswith("_radius") else float(v))
    return p


def _nlm_planes(half0, half1):
    """(w, h, half0, half1, out, err): two (H, W, 4) half accumulators as contiguous float32."""
    a, b = (np.ascontiguousarray(v, dtype=np.float32) for v in (half0, half1))
    if a.ndim != 3 or a.shape[-1] != 4 or b.shape != a.shape:
        raise ValueError(f"half planes {a.shape}, {b.shape} are not two (H, W, 4) images of one size")
    return a.shape[1], a.shape[0], a, b, np.zeros_like(a), np.zeros_like(a)


def denoise_nlm_image_host(half0, half1, **params):
    """The CPU twin of Renderer.denoise_nlm_image (surf_denoise_nlm_image_host): (image, err), each (H, W, 4) float32;
    bit-identical, no device."""
    w, h, a, b, out, err = _nlm_planes(half0, half1)
    p = nlm_params(**params)
    _check(load().surf_denoise_nlm_image_host(w, h, _ptr(a), _ptr(b), C.byref(p), _ptr(out), _ptr(err)), "surf_denoise_nlm_image_host")
    return out, err


def display_default_params() -> DisplayParams:
    """surf_display_default_params -- conventions, not measurements: exposure auto (key 0.18, scale within 1/64..64, manual
    exposure 1), bloom off (radius 0, threshold 1, strength 0.1), the ACES curve (white 4), sRGB, dither on."""
    p = DisplayParams()
    _check(load().surf_display_default_params(C.byref(p)), "surf_display_default_params")
    return p


def display_params(**params) -> DisplayParams:
    """display_default_params() with the given fields replaced."""
    p = display_default_params()
    kinds = {name: ctype for name, ctype in DisplayParams._fields_}
    for name, v in params.items():
        if name not in kinds:
            raise TypeError(f"surf_display_params has no field {name!r}")
        setattr(p, name, int(v) if kinds[name] is C.c_uint32 else float(v))
    return p


def _display_plane(img):
    """(w, h, img, words): an (H, W, 4) float RGBA image as contiguous float32 and the (H, W) uint32 image it becomes."""
    a = np.ascontiguousarray(img, dtype=np.float32)
    if a.ndim != 3 or a.shape[-1] != 4:
        raise ValueError(f"image {a.shape} is not (H, W, 4)")
    return a.shape[1], a.shape[0], a, np.zeros(a.shape[:2], np.uint32)


def display_image_host(img, **params):
    """The CPU twin of Renderer.display_image (surf_display_image_host): (RGBA8 words (H, W) uint32, the meter's result
    as a dict); bit-identical, no device."""
    w, h, a, out = _display_plane(img)
    p, m = display_params(**params), DisplayMeterResult()
    _check(load().surf_display_image_host(w, h, _ptr(a), C.byref(p), _ptr(out), C.byref(m)), "surf_display_image_host")
    return out, m.as_dict()


def display_srgb_table() -> np.ndarray:
    """The display stage's sRGB table, indexed by the square root (surf_display_srgb_table): 4096 float32."""
    t = np.zeros(4096, np.float32)
    _check(load().surf_display_srgb_table(_ptr(t)), "surf_display_srgb_table")
    return t


def display_bayer8() -> np.ndarray:
    """The display stage's 8 x 8 Bayer matrix (surf_display_bayer8): (8, 8) uint8, [y, x]."""
    b = np.zeros((8, 8), np.uint8)
    _check(load().surf_display_bayer8(_ptr(b)), "surf_display_bayer8")
    return b


def regress_params(**params) -> RegressParams:
    """surf_regress_default_params (search_radius 5, patch_radius 2, k 0.7, alpha 1.0, eps 1e-10, ridge 0.1) with the
    given fields replaced."""
    p = RegressParams()
    _check(load().surf_regress_default_params(C.byref(p)), "surf_regress_default_params")
    for name, v in params.items():
        if name not in ("search_radius", "patch_radius", "k", "alpha", "eps", "ridge"):
            raise TypeError(f"surf_regress_params has no field {name!r}")
        setattr(p, name, int(v) if name.endswith("_radius") else float(v))
    return p


def _regress_planes(half0, half1, planes):
    """(w, h, [half0, half1, position, normal, albedo], out, err): (H, W, 4) images of one size as contiguous float32;
    planes is Renderer.aov()'s dict or a (position, normal, albedo) sequence."""
    w, h, a, b, out, err = _nlm_planes(half0, half1)
    _, _, f = _denoise_planes(a, planes)
    return w, h, [a, b] + f[1:], out, err


def denoise_regress_image_host(half0, half1, planes, **params):
    """The CPU twin of Renderer.denoise_regress_image (surf_denoise_regress_image_host): (image, err), each (H, W, 4)
    float32; bit-identical, no device."""
    w, h, a, out, err = _regress_planes(half0, half1, planes)
    p = regress_params(**params)
    _check(load().surf_denoise_regress_image_host(w, h, *(_ptr(v) for v in a), C.byref(p), _ptr(out), _ptr(err)),
           "surf_denoise_regress_image_host")
    return out, err


def bucket_halves(buckets) -> tuple:
    """The two half images of (M, ..., 4) bucket planes: the sums of the even and of the odd planes, added in bucket
    order in float32.  Accumulator planes of independent samples (w = the half's sample count)."""
    b = np.asarray(buckets, dtype=np.float32)
    if b.ndim < 3 or b.shape[-1] != 4 or b.shape[0] < 2:
        raise ValueError(f"bucket planes {b.shape} are not (M, ..., 4) with M >= 2")
    halves = []
    for first in (0, 1):
        s = np.zeros(b.shape[1:], np.float32)
        for j in range(first, b.shape[0], 2):
            s = s + b[j]
        halves.append(s)
    return halves[0], halves[1]


_MASK_FIELDS = ("threshold", "floor", "min_samples", "max_samples", "dilate")


def adaptive_mask_params(**params) -> AdaptiveMaskParams:
    """surf_adaptive_default_mask_params (threshold 0.05, floor 0.01, min_samples 16, max_samples 1024, dilate 1)
    with the given fields replaced."""
    p = AdaptiveMaskParams()
    _check(load().surf_adaptive_default_mask_params(C.byref(p)), "surf_adaptive_default_mask_params")
    for k, v in params.items():
        if k not in _MASK_FIELDS:
            raise TypeError(f"unknown mask parameter {k!r}")
        setattr(p, k, float(v) if k in ("threshold", "floor") else int(v))
    return p


def adaptive_params(**params) -> AdaptiveParams:
    """surf_adaptive_default_params (the mask defaults, batch 64, max_segments 0, first_sample_index 0) with the given
    fields replaced; the mask's fields are given by their own names."""
    p = AdaptiveParams()
    _check(load().surf_adaptive_default_params(C.byref(p)), "surf_adaptive_default_params")
    p.mask = adaptive_mask_params(**{k: v for k, v in params.items() if k in _MASK_FIELDS})
    for k, v in params.items():
        if k in _MASK_FIELDS:
            continue
        if k not in ("batch", "max_segments", "first_sample_index"):
            raise TypeError(f"unknown adaptive parameter {k!r}")
        setattr(p, k, int(v))
    return p


def _mask_planes(acc, squares):
    a, q = (np.ascontiguousarray(v, dtype=np.float32) for v in (acc, squares))
    if a.ndim != 3 or a.shape[2] != 4 or q.shape != a.shape:
        raise ValueError(f"mask planes {a.shape}, {q.shape} are not two (H, W, 4) images of one size")
    h, w = a.shape[:2]
    return w, h, a, q, np.zeros((h, w), np.uint8), np.zeros(h * w, np.uint32)


def adaptive_mask_image_host(acc, squares, **params):
    """The CPU twin of Renderer.adaptive_mask_image (surf_adaptive_mask_image_host): (mask (H, W) uint8, the
    ascending list of active pixel indices) of two (H, W, 4) planes; bit-identical, no device."""
    w, h, a, q, mask, lst = _mask_planes(acc, squares)
    p, n = adaptive_mask_params(**params), C.c_uint32()
    _check(load().surf_adaptive_mask_image_host(w, h, _ptr(a), _ptr(q), C.byref(p), _ptr(mask), _ptr(lst), C.byref(n)),
           "surf_adaptive_mask_image_host")
    return mask, lst[:n.value].copy()


_ERROR_MASK_FIELDS = ("threshold", "floor", "min_samples", "max_samples", "smooth", "dilate")
_NLM_FIELDS = ("search_radius", "patch_radius", "k", "alpha", "eps")


def error_mask_params(**params) -> ErrorMaskParams:
    """surf_error_mask_default_params (threshold 0.1, floor 0.01, min_samples 16, max_samples 1024, smooth 3, dilate 1)
    with the given fields replaced."""
    p = ErrorMaskParams()
    _check(load().surf_error_mask_default_params(C.byref(p)), "surf_error_mask_default_params")
    for k, v in params.items():
        if k not in _ERROR_MASK_FIELDS:
            raise TypeError(f"unknown error mask parameter {k!r}")
        setattr(p, k, float(v) if k in ("threshold", "floor") else int(v))
    return p


def adaptive_nlm_params(**params) -> AdaptiveNlmParams:
    """surf_adaptive_nlm_default_params (the mask's and the filter's defaults, batch 64, max_segments 0,
    first_sample_index 0) with the given fields replaced; the mask's and the filter's fields are given by their own names."""
    p = AdaptiveNlmParams()
    _check(load().surf_adaptive_nlm_default_params(C.byref(p)), "surf_adaptive_nlm_default_params")
    p.mask = error_mask_params(**{k: v for k, v in params.items() if k in _ERROR_MASK_FIELDS})
    p.nlm = nlm_params(**{k: v for k, v in params.items() if k in _NLM_FIELDS})
    for k, v in params.items():
        if k in _ERROR_MASK_FIELDS or k in _NLM_FIELDS:
            continue
        if k not in ("batch", "max_segments", "first_sample_index"):
            raise TypeError(f"unknown adaptive parameter {k!r}")
        setattr(p, k, int(v))
    return p


def _error_mask_planes(out, err, acc):
    o, e, a = (np.ascontiguousarray(v, dtype=np.float32) for v in (out, err, acc))
    if o.ndim != 3 or o.shape[2] != 4 or e.shape != o.shape or a.shape != o.shape:
        raise ValueError(f"mask planes {o.shape}, {e.shape}, {a.shape} are not three (H, W, 4) images of one size")
    h, w = o.shape[:2]
    return w, h, o, e, a, np.zeros((h, w), np.uint8), np.zeros(h * w, np.uint32)


def error_mask_image_host(out, err, acc, **params):
    """The CPU twin of Renderer.error_mask_image (surf_error_mask_image_host): (mask (H, W) uint8, the ascending list of
    active pixel indices) of the non-local-means filter's two outputs and the accumulator, each (H, W, 4);
    bit-identical, no device."""
    w, h, o, e, a, mask, lst = _error_mask_planes(out, err, acc)
    p, n = error_mask_params(**params), C.c_uint32()
    _check(load().surf_error_mask_image_host(w, h, _ptr(o), _ptr(e), _ptr(a), C.byref(p), _ptr(mask), _ptr(lst), C.byref(n)),
           "surf_error_mask_image_host")
    return mask, lst[:n.value].copy()


ATLAS_PLANES = ("position", "normal", "albedo", "ids")   # surf_atlas_build's planes
ATLAS_MAX_SIDE = 16384
ATLAS_MAX_ITERATIONS = 64


def atlas_chart(instance: int, scale=(1.0, 1.0), offset=(0.0, 0.0), flip: bool = False) -> AtlasChart:
    """One surf_atlas_chart."""
    ch = AtlasChart()
    ch.instance, ch.flags = int(instance), 1 if flip else 0
    ch.scale[0], ch.scale[1] = float(scale[0]), float(scale[1])
    ch.offset[0], ch.offset[1] = float(offset[0]), float(offset[1])
    return ch


def atlas_chart_array(charts):
    """A ctypes array of the charts (AtlasChart records, or (instance, flags, sx, sy, ox, oy) rows) and their count."""
    rows = list(charts)
    arr = (AtlasChart * max(len(rows), 1))()
    for k, ch in enumerate(rows):
        if isinstance(ch, AtlasChart):
            arr[k] = ch
        else:
            i, f, sx, sy, ox, oy = ch
            arr[k] = atlas_chart(i, (sx, sy), (ox, oy))
            arr[k].flags = int(f)
    return arr, len(rows)


def _atlas_desc(scene_or_desc) -> SceneDesc:
    return scene_or_desc.desc() if isinstance(scene_or_desc, Scene) else scene_or_desc


def _atlas_size(what: str, W: int, H: int):
    if not (isinstance(W, (int, np.integer)) and isinstance(H, (int, np.integer))) or W < 0 or H < 0 or W >= 2 ** 32 or H >= 2 ** 32:
        raise ValueError(f"{what}: W x H = {W!r} x {H!r} is not a pair of 32-bit sizes")


def _atlas_out(W: int, H: int) -> dict:
    out = {k: np.zeros((H, W, 4), np.float32) for k in ATLAS_PLANES[:3]}
    out["ids"] = np.zeros((H, W, 4), np.uint32)
    return out


def atlas_grid_charts(instances, W: int, H: int, margin_texels: int = 0) -> list:
    """Charts on a grid (surf_atlas_grid_charts): `instances` is a list of instance indices, or a count n for instances
    0..n-1; entry i gets cell i of a g x g grid, g = ceil(sqrt(n)), shrunk by margin_texels on every side."""
    _atlas_size("atlas_grid_charts", W, H)
    ids = None if isinstance(instances, (int, np.integer)) else np.ascontiguousarray(instances, dtype=np.uint32)
    n = int(instances) if ids is None else len(ids)
    arr = (AtlasChart * max(n, 1))()
    _check(load().surf_atlas_grid_charts(n, None if ids is None else _ptr(ids), W, H, margin_texels, arr), "surf_atlas_grid_charts")
    return [AtlasChart.from_buffer_copy(arr[k]) for k in range(n)]


def atlas_build_host(scene_or_desc, charts, W: int, H: int) -> dict:
    """The CPU twin of Renderer.atlas_build (surf_atlas_build_host): the four planes (H, W, 4) and the summary."""
    _atlas_size("atlas_build_host", W, H)
    d, (arr, n), s = _atlas_desc(scene_or_desc), atlas_chart_array(charts), AtlasSummary()
    ok = 0 < W <= ATLAS_MAX_SIDE and 0 < H <= ATLAS_MAX_SIDE
    out = _atlas_out(W if ok else 1, H if ok else 1)
    _check(load().surf_atlas_build_host(C.byref(d), arr, n, W, H, *(_ptr(out[k]) for k in ATLAS_PLANES), C.byref(s)), "surf_atlas_build_host")
    out["summary"] = s.as_dict()
    return out


def _atlas_plane(what: str, a, H: int, W: int, dtype=np.float32) -> np.ndarray:
    """A caller's (H, W, 4) plane (or (H, W) bytes) checked before the library sees it."""
    a = np.asarray(a)
    shape = (H, W, 4) if dtype == np.float32 else (H, W)
    if a.dtype != dtype:
        raise ValueError(f"{what} is {a.dtype}, not {np.dtype(dtype).name}")
    if a.shape != shape:
        raise ValueError(f"{what} has shape {a.shape}, not {shape}")
    return np.ascontiguousarray(a)


def _atlas_finish_args(acc, albedo):
    acc = np.asarray(acc)
    if acc.ndim != 3 or acc.shape[2] != 4:
        raise ValueError(f"atlas_finish: acc has shape {acc.shape}, not (H, W, 4)")
    H, W = acc.shape[:2]
    a, b = _atlas_plane("atlas_finish: acc", acc, H, W), _atlas_plane("atlas_finish: albedo", albedo, H, W)
    return W, H, a, b, np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint8)


def atlas_finish_host(acc, albedo):
    """(light map (H, W, 4), valid (H, W) uint8) from an accumulator-form plane and the build's albedo plane
    (surf_atlas_finish_host, the CPU twin of Renderer.atlas_finish)."""
    W, H, a, b, out, valid = _atlas_finish_args(acc, albedo)
    _check(load().surf_atlas_finish_host(W, H, _ptr(a), _ptr(b), _ptr(out), _ptr(valid)), "surf_atlas_finish_host")
    return out, valid


def _atlas_dilate_args(rgba, valid, iterations):
    rgba = np.asarray(rgba)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError(f"atlas_dilate: rgba has shape {rgba.shape}, not (H, W, 4)")
    H, W = rgba.shape[:2]
    a, v = _atlas_plane("atlas_dilate: rgba", rgba, H, W), _atlas_plane("atlas_dilate: valid", valid, H, W, np.uint8)
    if not 0 <= int(iterations) <= ATLAS_MAX_ITERATIONS:
        raise ValueError(f"atlas_dilate: iterations {iterations} outside 0..{ATLAS_MAX_ITERATIONS}")
    return W, H, a, v, np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.uint8)


def atlas_dilate_host(rgba, valid, iterations: int = 2):
    """(rgba, valid) after `iterations` gutter-fill passes (surf_atlas_dilate_host, the CPU twin of Renderer.atlas_dilate)."""
    W, H, a, v, out, ov = _atlas_dilate_args(rgba, valid, iterations)
    _check(load().surf_atlas_dilate_host(W, H, _ptr(a), _ptr(v), int(iterations), _ptr(out), _ptr(ov)), "surf_atlas_dilate_host")
    return out, ov


def obj_load(path: str, threads: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """Mesh(path) (mesh.cpp:69-154): parallel tinyobj-compatible OBJ/OBJ.GZ parse.
    Returns ((n, 16) float32 Triangle records, (n, 20) float32 TriExtension
    records); identical for every thread count."""
    h = C.c_void_p()
    _check(load().surf_obj_load(path.encode(), threads, C.byref(h)), "surf_obj_load")
    try:
        tp, xp, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
        _check(load().surf_mesh_data(h, C.byref(tp), C.byref(xp), C.byref(n)), "surf_mesh_data")
        k = n.value
        tris = np.ctypeslib.as_array(C.cast(tp, C.POINTER(C.c_float)), (k * 16,)).reshape(k, 16).copy() if k else np.zeros((0, 16), np.float32)
        ext = np.ctypeslib.as_array(C.cast(xp, C.POINTER(C.c_float)), (k * 20,)).reshape(k, 20).copy() if k else np.zeros((0, 20), np.float32)
    finally:
        load().surf_mesh_destroy(h)
    return tris, ext


def bvh_build(triangles: np.ndarray, threads: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """BvhBLAS::build (bvh.cpp:255-465) over (n, 16) float32 Triangle records
    (v0, v1, v2, centroid), multi-threaded (0 = default thread count).
    Returns (indices (n,) uint32, nodes (nodes_used, 12) float32 view of the
    48-B BvhNode records); identical for every thread count."""
    tris = np.ascontiguousarray(triangles, dtype=np.float32)
    n = tris.shape[0]
    idx = np.empty(n, np.uint32)
    nodes = np.zeros((2 * n, 12), np.float32)
    used = C.c_uint32()
    _check(load().surf_bvh_build(_ptr(tris), n, threads, _ptr(idx), _ptr(nodes), C.byref(used)), "surf_bvh_build")
    return idx, nodes[: used.value]


@dataclass
class ShardSpec:
    shard: int = 0
    shards: int = 1
    row_block: int = 0      # 0: contiguous rows; N: interleaved blocks of N rows


def shard_rows(height: int, spec: ShardSpec) -> np.ndarray:
    """Rows a shard owns -- same rule as surf_create_sharded."""
    r = np.arange(height, dtype=np.int64)
    if spec.row_block == 0:
        lo = height * spec.shard // spec.shards
        hi = height * (spec.shard + 1) // spec.shards
        return r[lo:hi]
    return r[(r // spec.row_block) % spec.shards == spec.shard]


def assemble_shards(width: int, height: int, parts: list[np.ndarray], specs: list[ShardSpec]) -> np.ndarray:
    """Places per-shard accumulator rows (shard order) into a full (H, W, 4) frame."""
    full = np.zeros((height, width, 4), dtype=np.float32)
    for part, spec in zip(parts, specs):
        rows = shard_rows(height, spec)
        full[rows] = np.asarray(part, dtype=np.float32).reshape(len(rows), width, 4)
    return full


class Renderer:
    """One surf_ctx: a shard of a width x height frame on one HIP device."""

    def __init__(self, scene: Scene, width: int, height: int, device: int = 0, shard: ShardSpec | None = None,
                 pool_capacity: int | None = None, frame_batch: int | None = None, camera: bytes | None = None):
        lib = load()
        self.width, self.height = width, height
        self.shard = shard or ShardSpec()
        h = C.c_void_p()
        _check(lib.surf_create_sharded(device, width, height, self.shard.shard, self.shard.shards,
                                       self.shard.row_block, C.byref(h)), "surf_create_sharded")
        self._h = h
        n = C.c_uint32()
        _check(lib.surf_shard_rows(h, None, C.byref(n)), "surf_shard_rows", h)
        self.rows = np.zeros(n.value, dtype=np.uint32)
        _check(lib.surf_shard_rows(h, _ptr(self.rows), C.byref(n)), "surf_shard_rows", h)
        if pool_capacity:
            _check(lib.surf_set_pool_capacity(h, pool_capacity), "surf_set_pool_capacity", h)
        if frame_batch:
            _check(lib.surf_set_frame_batch(h, frame_batch), "surf_set_frame_batch", h)
        d = scene.desc()
        _check(lib.surf_upload_scene(h, C.byref(d)), "surf_upload_scene", h)
        ubo = camera if camera is not None else scene.camera(width, height)
        buf = CameraUBO.from_buffer_copy(ubo)
        _check(lib.surf_set_camera(h, buf), "surf_set_camera", h)

    @property
    def handle(self):
        return self._h

    def debug_capped(self):
        """(count, sample ids) of paths ended by the segment cap in the current stream."""
        ids = np.zeros(64, np.uint32)
        n = C.c_uint64()
        _check(load().surf_debug_capped(self._h, _ptr(ids), 64, C.byref(n)), "surf_debug_capped", self._h)
        return int(n.value), ids[ids != 0xFFFFFFFF]

    def debug_issue_order(self):
        """(heavy pixels, permuted frames) of the current stream's issue order
        (surf_debug_issue_order); (0, 0) when it is frame-major throughout."""
        a, f = C.c_uint32(), C.c_uint32()
        _check(load().surf_debug_issue_order(self._h, C.byref(a), C.byref(f)), "surf_debug_issue_order", self._h)
        return int(a.value), int(f.value)

    def debug_connect_staging(self):
        """(records, triangles) of the emitters' BLAS the last k_connect launch
        walked from LDS (surf_debug_connect_staging); (0, 0) when none was staged."""
        a, t = C.c_uint32(), C.c_uint32()
        _check(load().surf_debug_connect_staging(self._h, C.byref(a), C.byref(t)), "surf_debug_connect_staging", self._h)
        return int(a.value), int(t.value)

    def debug_kernel_selection(self) -> dict:
        """The kernel variants the uploaded scene selects (surf_debug_kernel_selection):
        lds_tables, stack16, lane_two_level, wave_eligible as booleans."""
        v = [C.c_uint32() for _ in range(4)]
        _check(load().surf_debug_kernel_selection(self._h, *[C.byref(x) for x in v]), "surf_debug_kernel_selection", self._h)
        return dict(zip(("lds_tables", "stack16", "lane_two_level", "wave_eligible"), (bool(x.value) for x in v)))

    def debug_shadow_keys(self, origins, directions, tmax, lights):
        """(keys, bins, layout): the shadow queue's order bin of each of n rays --
        origins and directions (n, 3) float32, tmax (n,) float32, light slots
        (n,) uint32 -- under this context's key layout (SURF_SH_KEY), the
        number of bins in use, and what the key reads of the scene: cell_lo
        (3,), cell_scale (3,), heavy_lo and heavy_hi (n_heavy, 3), the heaviest
        instance first (surf_debug_shadow_keys)."""
        fn = getattr(load(), "surf_debug_shadow_keys", None)
        if fn is None or fn.argtypes is None:
            raise RuntimeError("the loaded library (SURF_HIP_LIB) was built before surf_debug_shadow_keys existed: rebuild it")
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tmax, np.float32).reshape(-1)
        li = np.ascontiguousarray(lights, np.uint32).reshape(-1)
        n = len(o)
        if not (len(d) == len(t) == len(li) == n):
            raise ValueError("debug_shadow_keys: origins, directions, tmax and lights differ in length")
        keys = np.zeros(n, np.uint32)
        bins = C.c_uint32()
        lay = np.zeros(25, np.float32)
        _check(fn(self._h, n, _ptr(o), _ptr(d), _ptr(t), _ptr(li), _ptr(keys), C.byref(bins), _ptr(lay)), "surf_debug_shadow_keys", self._h)
        nh = int(lay[6])
        boxes = lay[7:].reshape(3, 2, 3)[:nh]
        return keys, int(bins.value), {"cell_lo": lay[0:3].copy(), "cell_scale": lay[3:6].copy(),
                                       "heavy_lo": boxes[:, 0].copy(), "heavy_hi": boxes[:, 1].copy()}

    def debug_segment_cycles(self, origin, direction, throughput, seed: int, segment: int = 1, reps: int = 64):
        """Diagnostics: mean shader-clock cycles of one drain segment's pieces on
        a lone wave (surf_debug_segment_cycles): walk, shade, shadow walk,
        cosine sample, light sample, hit normal."""
        rec = np.zeros(12, np.float32)
        rec[0:3] = origin
        rec[4:7] = direction
        rec[8:11] = throughput
        u = rec.view(np.uint32)
        u[3] = 0
        u[7] = (segment << 2)
        u[11] = seed & 0xFFFFFFFF
        out = np.zeros(15, np.uint64)
        _check(load().surf_debug_segment_cycles(self._h, _ptr(rec), reps, _ptr(out)), "surf_debug_segment_cycles", self._h)
        names = ("walk", "shade", "shadow_walk", "cosine", "light_sample", "normal", "checksum", "interior_cycles",
                 "leaf_cycles", "walks", "leaves", "triangles", "visits2", "prologue_cycles", "instance_loop_cycles")
        return {k: float(out[i]) / reps for i, k in enumerate(names) if k != "checksum"}

    def debug_math(self, op: str, x) -> np.ndarray:
        """Diagnostics: the kernels' libm on the device (surf_debug_math), one lane
        per element of the float32 array x.  op: "expf", "sinf", "cosf" (n
        results) or "sincosf" ((n, 2): sin, cos)."""
        if op not in MATH_OPS:
            raise ValueError(f"debug_math: op {op!r} is not one of {MATH_OPS}")
        x = np.ascontiguousarray(x, np.float32).reshape(-1)
        out = np.zeros((len(x), 2) if op == "sincosf" else len(x), np.float32)
        _check(load().surf_debug_math(self._h, MATH_OPS.index(op), len(x), _ptr(x), _ptr(out)), "surf_debug_math", self._h)
        return out

    def debug_trace_paths(self, origins, directions, seeds, max_segments: int, mode: int = 0):
        """Diagnostics: planted paths (surf_debug_trace_paths).  Path i starts at
        origins[i] toward directions[i] ((n, 3) float32) with RNG state seeds[i]
        and runs to its end or max_segments (1..4096) on the device: mode 0 one
        path per lane (the wavefront kernels' device functions), mode 1 one
        path per wave (the cooperative drain's).  Returns (energy (n, 3)
        float32, segments (n,) uint32, final seeds (n,) uint32)."""
        o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(directions, np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        if not (len(o) == len(d) == len(s)):
            raise ValueError("debug_trace_paths: origins, directions and seeds differ in length")
        out = np.zeros((len(o), 4), np.float32)
        end = np.zeros(len(o), np.uint32)
        _check(load().surf_debug_trace_paths(self._h, len(o), _ptr(o), _ptr(d), _ptr(s), max_segments, mode, _ptr(out), _ptr(end)),
               "surf_debug_trace_paths", self._h)
        return out[:, :3].copy(), out[:, 3].copy().view(np.uint32), end

    def set_zero_cutoff(self, on):
        """True / False, or None for the automatic default (on for 1-sample frames, off for multi-sample frames)."""
        _check(load().surf_set_zero_cutoff(self._h, -1 if on is None else (1 if on else 0)), "surf_set_zero_cutoff", self._h)

    def update_instances(self, scene: Scene):
        """Re-uploads the scene's instance records, TLAS and lights (after Scene.update)."""
        d = scene.desc()
        _check(load().surf_update_instances(self._h, d.instances, d.instance_count, d.tlas_indices, d.tlas_nodes,
                                            d.tlas_node_count, d.lights, d.light_count), "surf_update_instances", self._h)

    def set_tail_policy(self, threshold_paths: int = 0, lanes_per_wave: int = 0, stage_segments: int = 0):
        """Drain policy of the tail kernel (0 = automatic); stage_segments is the
        per-stage segment budget before the survivors move on (0 = one stage)."""
        _check(load().surf_set_tail_policy(self._h, threshold_paths, lanes_per_wave, stage_segments), "surf_set_tail_policy",
               self._h)

    def set_tail_coop(self, max_paths: int):
        """Single-stage drain as the cooperative tail when <= max_paths paths remain (0 = never)."""
        _check(load().surf_set_tail_coop(self._h, max_paths), "surf_set_tail_coop", self._h)

    def set_trace_mode(self, mode: int):
        """0: one ray per lane; 1: one ray per wave (lanes as planes, the cooperative tail's traversal),
        for trace_closest/trace_any."""
        _check(load().surf_set_trace_mode(self._h, mode), "surf_set_trace_mode", self._h)

    def set_profiling(self, on: bool):
        _check(load().surf_set_profiling(self._h, 1 if on else 0), "surf_set_profiling", self._h)

    def render(self, frames: int, first_frame: int = 0, max_segments: int = 0, spp: int = 1):
        """`frames` frames of `spp` samples per pixel (Renderer::render with
        samplesPerFrame = spp, renderer.cpp:160-188): first_frame is the sample
        count before the call (the reference's totalSamples; the frame index for
        spp 1); frame k is seeded from first_frame + k * spp and its samples
        chain their RNG state."""
        _check(load().surf_render(self._h, frames, first_frame, max_segments, spp), "surf_render", self._h)

    def synchronize(self):
        _check(load().surf_synchronize(self._h), "surf_synchronize", self._h)

    def clear_accumulator(self):
        _check(load().surf_clear_accumulator(self._h), "surf_clear_accumulator", self._h)

    def accumulator(self) -> np.ndarray:
        out = np.zeros((len(self.rows), self.width, 4), dtype=np.float32)
        _check(load().surf_read_accumulator(self._h, _ptr(out)), "surf_read_accumulator", self._h)
        return out

    def set_camera(self, ubo: bytes):
        """surf_set_camera: a 128-byte CameraUBO (Scene.camera's layout).  A changed
        camera ends the sample stream and drops the cached feature buffers."""
        if len(ubo) != C.sizeof(CameraUBO):
            raise ValueError(f"camera UBO is {len(ubo)} bytes, not {C.sizeof(CameraUBO)}")
        buf = CameraUBO.from_buffer_copy(ubo)
        _check(load().surf_set_camera(self._h, buf), "surf_set_camera", self._h)

    def _read_planes(self, entry: str, names, floats: int, *before, after=()) -> dict:
        """The planes of one plane pass as {name: (rows, width, 4) array}: entry(handle,
        *before, plane index, *after, out) per plane; the first `floats` planes are
        float32, the rest uint32."""
        out = {}
        for k, name in enumerate(names):
            a = np.zeros((len(self.rows), self.width, 4), dtype=np.float32 if k < floats else np.uint32)
            _check(getattr(load(), entry)(self._h, *before, k, *after, _ptr(a)), entry, self._h)
            out[name] = a
        return out

    def _debug_ms(self, entry: str) -> float:
        """The one float a surf_debug_*_time of a single launch hands back."""
        ms = C.c_float()
        _check(getattr(load(), entry)(self._h, C.byref(ms)), entry, self._h)
        return float(ms.value)

    def aov(self) -> dict:
        """First-hit feature buffers of this shard's rows (surf_read_aov; the plane
        definitions are in include/surf_hip.h): 'position', 'normal' and 'albedo'
        as (rows, width, 4) float32, 'id' as (rows, width, 4) uint32 (instance,
        primitive, material, 0; ~0 on a miss).  Computed on the first read, cached
        until the camera, the scene or the instances change; the sample stream is
        not touched.  Row shards assemble like accumulators (assemble_shards
        works on float32: pass it the id plane as .view(np.float32))."""
        return self._read_planes("surf_read_aov", AOV_PLANES, 3)

    def copy_aov_to(self, plane: int, device_ptr: int):
        _check(load().surf_copy_aov_device(self._h, plane, C.c_void_p(device_ptr)), "surf_copy_aov_device", self._h)

    def debug_aov_time(self) -> float:
        """Device milliseconds of the last feature-buffer kernel launch (surf_debug_aov_time)."""
        return self._debug_ms("surf_debug_aov_time")

    def aov_chain(self, max_links: int = 8) -> dict:
        """The feature buffers traced through mirrors and glass (surf_read_aov_chain,
        which defines the chain): aov()'s keys, shapes and dtypes, each pixel's
        record taken at the first surface that is neither mirror nor glass along
        the pixel's unjittered ray, or at link max_links (0..AOV_CHAIN_MAX_LINKS);
        id.w is the number of links followed.  Cached like aov(), per max_links.
        Not for reprojection: the position is the real terminal point."""
        max_links = _chain_links(max_links)
        return self._read_planes("surf_read_aov_chain", AOV_PLANES, 3, after=(max_links,))

    def copy_aov_chain_to(self, plane: int, device_ptr: int, max_links: int = 8):
        max_links = _chain_links(max_links)
        _check(load().surf_copy_aov_chain_device(self._h, plane, max_links, C.c_void_p(device_ptr)), "surf_copy_aov_chain_device", self._h)

    def debug_aov_chain_time(self) -> float:
        """Device milliseconds of the last chain kernel launch (surf_debug_aov_chain_time)."""
        return self._debug_ms("surf_debug_aov_chain_time")

    def aov_sampled(self, samples: int = 16, first_sample: int = 0, key: str = "instance") -> dict:
        """The sampled feature buffers (surf_read_aov_sampled, which states the
        arithmetic): the first-hit features of the camera rays render() traces for
        frames first_sample .. first_sample + samples - 1 at one sample per frame,
        reduced per pixel.  AOVS_PLANES as (rows, width, 4): 'position', 'normal'
        and 'albedo' float32 (albedo.w = the hit coverage), 'id' (sample 0's ids,
        w = the hit count), 'matte_key' and 'matte_count' uint32 (the four best of
        the pixel's instance or material keys and their sample counts; see
        matte_coverage).  Cached like aov(), per parameter set."""
        q = aov_sampled_params(samples, first_sample, key)
        return self._read_planes("surf_read_aov_sampled", AOVS_PLANES, 3, C.byref(q))

    def copy_aov_sampled_to(self, plane: int, device_ptr: int, **params):
        q = aov_sampled_params(**params)
        _check(load().surf_copy_aov_sampled_device(self._h, C.byref(q), plane, C.c_void_p(device_ptr)), "surf_copy_aov_sampled_device", self._h)

    def debug_aov_sampled_time(self) -> float:
        """Device milliseconds of the last sampled-planes kernel launch (surf_debug_aov_sampled_time)."""
        return self._debug_ms("surf_debug_aov_sampled_time")

    def ao(self, samples: int = 16, radius: float = 1.0, first_sample: int = 0, bias: float = 1e-5, source: str = "first_hit",
           max_links: int = 8) -> dict:
        """Ray-traced ambient occlusion and bent normals (surf_read_ao, which
        states the arithmetic): `samples` cosine-weighted any-hit rays of length
        `radius` from every visible point of aov() (source "first_hit") or
        aov_chain(max_links) ("chain").  AO_PLANES as (rows, width, 4):
        'openness' float32 (xyz the mean unoccluded direction, not renormalised;
        w the unoccluded share, 1 on a miss pixel) and 'bits' uint32 (the sample
        mask's two words, the open count, 1 on a valid pixel).  Cached like
        aov(), per parameter set."""
        q = ao_params(samples, radius, first_sample, bias, source, max_links)
        return self._read_planes("surf_read_ao", AO_PLANES, 1, C.byref(q))

    def copy_ao_to(self, plane: int, device_ptr: int, **params):
        """One occlusion plane (index into AO_PLANES) into device memory of rows * width * 16 bytes (surf_copy_ao_device)."""
        q = ao_params(**params)
        _check(load().surf_copy_ao_device(self._h, C.byref(q), plane, C.c_void_p(device_ptr)), "surf_copy_ao_device", self._h)

    def debug_ao_time(self) -> float:
        """Device milliseconds of the last occlusion kernel launch (surf_debug_ao_time)."""
        return self._debug_ms("surf_debug_ao_time")

    def set_filter_guides(self, guides: str = "first_hit", max_links: int = 8, samples: int = 16, first_sample: int = 0):
        """Which planes denoise(), denoise_sampled() and denoise_regress() read
        (surf_set_filter_guides): "first_hit" (the default), "chain",
        aov_chain(max_links)'s, or "sampled", aov_sampled(samples, first_sample)'s
        (surf_set_filter_guides_sampled).  temporal(), svgf(), mask_from_noise()
        and render_adaptive() keep the first-hit planes."""
        if guides == FILTER_GUIDES_SAMPLED:
            q = aov_sampled_params(samples, first_sample)
            _check(load().surf_set_filter_guides_sampled(self._h, C.byref(q)), "surf_set_filter_guides_sampled", self._h)
            return
        if guides not in FILTER_GUIDES:
            raise ValueError(f"filter guides {guides!r}: one of {FILTER_GUIDES + (FILTER_GUIDES_SAMPLED,)}")
        max_links = _chain_links(max_links)
        _check(load().surf_set_filter_guides(self._h, FILTER_GUIDES.index(guides), max_links), "surf_set_filter_guides", self._h)

    def filter_guides(self) -> tuple:
        """(guides, max_links) as set_filter_guides took them (surf_get_filter_guides);
        with "sampled" guides the second member is their sample count."""
        g, n = C.c_int(), C.c_uint32()
        _check(load().surf_get_filter_guides(self._h, C.byref(g), C.byref(n)), "surf_get_filter_guides", self._h)
        return (FILTER_GUIDES + (FILTER_GUIDES_SAMPLED,))[g.value], int(n.value)

    def denoise(self, **params) -> np.ndarray:
        """The accumulated radiance through the edge-avoiding a-trous filter
        (surf_denoise; parameters as denoise_params): (H, W, 4) float32 radiance
        with w = 1 -- pack_rgba8(img, 1, display=True) is the displayable image.
        Reads the accumulator and the cached feature planes on the device and
        leaves both untouched.  Raises SURF_ERR_INVALID on a row shard: assemble
        the shards' accumulators and planes and call denoise_image."""
        p = denoise_params(**params)
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(load().surf_denoise(self._h, C.byref(p), _ptr(out)), "surf_denoise", self._h)
        return out

    def denoise_image(self, acc: np.ndarray, planes, **params) -> np.ndarray:
        """The same filter on host planes of any full frame (surf_denoise_image):
        acc (H, W, 4) with w = the sample count, planes Renderer.aov()'s dict or
        (position, normal, albedo)."""
        w, h, a = _denoise_planes(acc, planes)
        p = denoise_params(**params)
        out = np.zeros((h, w, 4), np.float32)
        _check(load().surf_denoise_image(self._h, w, h, _ptr(a[0]), _ptr(a[1]), _ptr(a[2]), _ptr(a[3]), C.byref(p), _ptr(out)),
               "surf_denoise_image", self._h)
        return out

    def copy_denoised_to(self, device_ptr: int, **params):
        p = denoise_params(**params)
        _check(load().surf_denoise_copy_device(self._h, C.byref(p), C.c_void_p(device_ptr)), "surf_denoise_copy_device", self._h)

    def debug_denoise_time(self) -> list:
        """Device milliseconds of the last denoise run's kernels (surf_debug_denoise_time):
        the prepare kernel, then each iteration (0 past the run's iterations)."""
        ms = (C.c_float * 7)()
        _check(load().surf_debug_denoise_time(self._h, ms, 7), "surf_debug_denoise_time", self._h)
        return [float(v) for v in ms]

    def temporal(self, spatial=None, **params) -> np.ndarray:
        """One frame of temporal accumulation (surf_temporal_accumulate; parameters
        as temporal_params): the accumulator blended with the reprojected result
        of the previous call, (H, W, 4) float32 with w = 1.  The loop per displayed
        frame: move the scene / camera, clear_accumulator(), render(1, first, spp=),
        temporal().  spatial: None, True (the denoiser's defaults) or a dict of
        denoiser parameters -- the returned image then went through the a-trous
        filter; the stored history is always the unfiltered blend.  Raises
        SURF_ERR_INVALID on a row shard (see temporal_image)."""
        p, sp = temporal_params(**params), _spatial_params(spatial)
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(load().surf_temporal_accumulate(self._h, C.byref(p), C.byref(sp) if sp is not None else None, _ptr(out)),
               "surf_temporal_accumulate", self._h)
        return out

    def temporal_reset(self):
        """Drops the stored history: the next temporal() is a first frame."""
        _check(load().surf_temporal_reset(self._h), "surf_temporal_reset", self._h)

    def temporal_history(self) -> np.ndarray:
        """(rgb, n) of the stored history (surf_temporal_history), n the history length."""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(load().surf_temporal_history(self._h, _ptr(out)), "surf_temporal_history", self._h)
        return out

    def temporal_image(self, cur, prev, **params):
        """The same blend on host planes of any two full frames (surf_temporal_image;
        cur and prev as _temporal_frames describes them, prev None for a first
        frame).  Returns (out, history)."""
        w, h, f, q, _keep = _temporal_frames(cur, prev)
        p = temporal_params(**params)
        out, hist = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        _check(load().surf_temporal_image(self._h, w, h, C.byref(f), C.byref(q) if q is not None else None, C.byref(p), _ptr(out),
                                          _ptr(hist)), "surf_temporal_image", self._h)
        return out, hist

    def copy_temporal_to(self, device_ptr: int, spatial=None, **params):
        p, sp = temporal_params(**params), _spatial_params(spatial)
        _check(load().surf_temporal_copy_device(self._h, C.byref(p), C.byref(sp) if sp is not None else None, C.c_void_p(device_ptr)),
               "surf_temporal_copy_device", self._h)

    def debug_temporal_time(self) -> float:
        """Device milliseconds of the last k_temporal launch (surf_debug_temporal_time)."""
        return self._debug_ms("surf_debug_temporal_time")

    def svgf(self, **params) -> np.ndarray:
        """One frame through the variance-guided filter (surf_svgf_accumulate): the
        loop and the stored state are temporal()'s -- the two may be mixed -- with
        the luminance moments carried along, their variance setting the a-trous
        filter's colour width per pixel.  params: temporal_params' and
        svgf_params' names together.  (H, W, 4) float32 with w = 1.  Raises
        SURF_ERR_INVALID on a row shard (see svgf_image).  firefly_scale= (0 = off,
        else >= 1: the firefly clamp in front), feedback= (the first filtered
        iteration becomes the stored history) or ext= (a SvgfExt or None) go
        through surf_svgf_accumulate_ex; all off is the call without them."""
        params, ex, x = _svgf_ext(params)
        p, sp = _svgf_split(params)
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        if ex:
            _check(load().surf_svgf_accumulate_ex(self._h, C.byref(p), C.byref(sp), x, _ptr(out)), "surf_svgf_accumulate_ex", self._h)
        else:
            _check(load().surf_svgf_accumulate(self._h, C.byref(p), C.byref(sp), _ptr(out)), "surf_svgf_accumulate", self._h)
        return out

    def svgf_moments(self) -> np.ndarray:
        """(mu1, mu2, m, 0) of the stored moments (surf_svgf_moments); raises when none are stored."""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(load().surf_svgf_moments(self._h, _ptr(out)), "surf_svgf_moments", self._h)
        return out

    def svgf_variance(self) -> np.ndarray:
        """Of the last svgf(): x the variance entering the filter, y leaving it (surf_svgf_variance)."""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(load().surf_svgf_variance(self._h, _ptr(out)), "surf_svgf_variance", self._h)
        return out

    def svgf_image(self, cur, prev, **params):
        """The same on host planes of any two full frames (surf_svgf_image; cur and
        prev as _svgf_frames describes them).  Returns (out, history, moments, variance).
        firefly_scale=, feedback= or ext= as svgf() (surf_svgf_image_ex)."""
        params, ex, x = _svgf_ext(params)
        p, sp = _svgf_split(params)
        w, h, f, q, _keep = _svgf_frames(cur, prev)
        res = [np.zeros((h, w, 4), np.float32) for _ in range(4)]
        args = (self._h, w, h, C.byref(f), C.byref(q) if q is not None else None, C.byref(p), C.byref(sp))
        if ex:
            _check(load().surf_svgf_image_ex(*args, x, *[_ptr(a) for a in res]), "surf_svgf_image_ex", self._h)
        else:
            _check(load().surf_svgf_image(*args, *[_ptr(a) for a in res]), "surf_svgf_image", self._h)
        return tuple(res)

    def copy_svgf_to(self, device_ptr: int, **params):
        params, ex, x = _svgf_ext(params)
        p, sp = _svgf_split(params)
        if ex:
            _check(load().surf_svgf_copy_device_ex(self._h, C.byref(p), C.byref(sp), x, C.c_void_p(device_ptr)), "surf_svgf_copy_device_ex",
                   self._h)
        else:
            _check(load().surf_svgf_copy_device(self._h, C.byref(p), C.byref(sp), C.c_void_p(device_ptr)), "surf_svgf_copy_device", self._h)

    def firefly_image(self, acc, albedo, scale, demodulate=True) -> np.ndarray:
        """The firefly clamp alone on host planes of any full frame (surf_firefly_image):
        the clamped accumulator A' = (c', 1), (H, W, 4) float32."""
        a, alb, out = _firefly_planes(acc, albedo)
        _check(load().surf_firefly_image(self._h, a.shape[1], a.shape[0], _ptr(a), _ptr(alb), int(bool(demodulate)), float(scale), _ptr(out)),
               "surf_firefly_image", self._h)
        return out

    def debug_firefly_time(self) -> float:
        """Device milliseconds of the last k_firefly launch (surf_debug_firefly_time)."""
        return self._debug_ms("surf_debug_firefly_time")

    def debug_svgf_time(self) -> list:
        """Device milliseconds of the last svgf run's kernels (surf_debug_svgf_time):
        k_temporal, the guides and the variance estimate, then each iteration."""
        ms = (C.c_float * 8)()
        _check(load().surf_debug_svgf_time(self._h, ms, 8), "surf_debug_svgf_time", self._h)
        return [float(v) for v in ms]

    def set_sample_squares(self, on: bool):
        """Switches the per-sample second moments on or off (surf_set_sample_squares): with
        them on every sample's squares are summed beside the accumulator.  Raises
        SURF_ERR_INVALID unless the accumulator is empty (new, or just cleared)."""
        _check(load().surf_set_sample_squares(self._h, 1 if on else 0), "surf_set_sample_squares", self._h)

    def sample_squares(self) -> np.ndarray:
        """The squares plane of this shard's rows (surf_read_sample_squares): (rows, width, 4)
        float32, (sum r^2, sum g^2, sum b^2, sum lum^2) over the samples."""
        out = np.zeros((len(self.rows), self.width, 4), dtype=np.float32)
        _check(load().surf_read_sample_squares(self._h, _ptr(out)), "surf_read_sample_squares", self._h)
        return out

    def copy_sample_squares_to(self, device_ptr: int):
        _check(load().surf_copy_sample_squares_device(self._h, C.c_void_p(device_ptr)), "surf_copy_sample_squares_device", self._h)

    def denoise_sampled(self, **params) -> np.ndarray:
        """The accumulated radiance through the sample-variance-guided filter
        (surf_denoise_sampled; svgf_params' names without spatial_below): the a-trous
        filter whose colour width is each pixel's own sample variance of the mean,
        for stills from about 16 samples per pixel.  (H, W, 4) float32 with w = 1.
        Needs set_sample_squares(True) before the samples; raises SURF_ERR_INVALID
        on a row shard (see denoise_sampled_image)."""
        p = _sampled_params(params)
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        _check(load().surf_denoise_sampled(self._h, C.byref(p), _ptr(out)), "surf_denoise_sampled", self._h)
        return out

    def denoise_sampled_image(self, acc, squares, planes, **params):
        """The same filter on host planes of any full frame (surf_denoise_sampled_image).
        Returns (out, variance): variance x entering the filter, y leaving it."""
        w, h, a = _sampled_planes(acc, squares, planes)
        p = _sampled_params(params)
        out, var = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        _check(load().surf_denoise_sampled_image(self._h, w, h, *[_ptr(x) for x in a], C.byref(p), _ptr(out), _ptr(var)),
               "surf_denoise_sampled_image", self._h)
        return out, var

    def copy_denoise_sampled_to(self, device_ptr: int, **params):
        p = _sampled_params(params)
        _check(load().surf_denoise_sampled_copy_device(self._h, C.byref(p), C.c_void_p(device_ptr)), "surf_denoise_sampled_copy_device",
               self._h)

    def debug_sampled_time(self) -> list:
        """Device milliseconds of the last sampled run's kernels (surf_debug_sampled_time): level 0, then each iteration."""
        ms = (C.c_float * 7)()
        _check(load().surf_debug_sampled_time(self._h, ms, 7), "surf_debug_sampled_time", self._h)
        return [float(v) for v in ms]

    def noise_estimate(self, threshold=None, floor=None, image: bool = True):
        """(error image, summary dict) of this shard's rows (surf_noise_estimate): per pixel the
        relative standard error of its mean luminance (1e30 below two samples), and
        {'pixels', 'above', 'max_error'}.  image=False: no image is written, None returned in its place."""
        p, s = noise_params(threshold, floor), NoiseSummary()
        err = np.zeros((len(self.rows), self.width), np.float32) if image else None
        _check(load().surf_noise_estimate(self._h, C.byref(p), _ptr(err) if image else None, C.byref(s)), "surf_noise_estimate", self._h)
        return err, s.as_dict()

    def noise_image(self, acc, squares, threshold=None, floor=None):
        """The same on host planes of any shape (..., 4) (surf_noise_image)."""
        a, q, err = _noise_planes(acc, squares)
        p, s = noise_params(threshold, floor), NoiseSummary()
        _check(load().surf_noise_image(self._h, err.size, _ptr(a), _ptr(q), C.byref(p), _ptr(err), C.byref(s)), "surf_noise_image", self._h)
        return err, s.as_dict()

    def set_sample_buckets(self, m: int):
        """Switches M sample buckets on (M = 2, 4, 8, 16) or off (0) (surf_set_sample_buckets): each sample is also summed
        into the bucket its pixel's sample count selects.  Raises SURF_ERR_INVALID unless the accumulator is empty."""
        _check(load().surf_set_sample_buckets(self._h, int(m)), "surf_set_sample_buckets", self._h)

    def sample_bucket_count(self) -> int:
        m = C.c_uint32()
        _check(load().surf_get_sample_buckets(self._h, C.byref(m)), "surf_get_sample_buckets", self._h)
        return int(m.value)

    def sample_buckets(self) -> np.ndarray:
        """The bucket planes of this shard's rows (surf_read_sample_buckets): (M, rows, width, 4) float32,
        (sum r, sum g, sum b, samples) of the samples each bucket took."""
        out = np.zeros((self.sample_bucket_count(), len(self.rows), self.width, 4), dtype=np.float32)
        _check(load().surf_read_sample_buckets(self._h, _ptr(out)), "surf_read_sample_buckets", self._h)
        return out

    def copy_sample_buckets_to(self, device_ptr: int):
        _check(load().surf_copy_sample_buckets_device(self._h, C.c_void_p(device_ptr)), "surf_copy_sample_buckets_device", self._h)

    def robust(self, trim_scale=None, image: bool = True):
        """(accumulator plane, trim image, summary dict) of this shard's rows (surf_robust_accumulator): the
        median-of-means estimate from the sample buckets, an accumulator plane (mean = rgb / w); per pixel the bucket
        means dropped at either end; {'pixels', 'trimmed'}.  image=False: no trim image is written, None returned."""
        p, s = robust_params(trim_scale), RobustSummary()
        out = np.zeros((len(self.rows), self.width, 4), np.float32)
        trim = np.zeros((len(self.rows), self.width), np.uint8) if image else None
        _check(load().surf_robust_accumulator(self._h, C.byref(p), _ptr(out), _ptr(trim) if image else None, C.byref(s)),
               "surf_robust_accumulator", self._h)
        return out, trim, s.as_dict()

    def robust_image(self, acc, buckets, trim_scale=None):
        """The same on host planes: acc of any shape (..., 4), buckets (M, ..., 4) (surf_robust_image)."""
        npx, m, a, b, out, trim = _robust_planes(acc, buckets)
        p, s = robust_params(trim_scale), RobustSummary()
        _check(load().surf_robust_image(self._h, npx, m, _ptr(a), _ptr(b), C.byref(p), _ptr(out), _ptr(trim), C.byref(s)),
               "surf_robust_image", self._h)
        return out, trim, s.as_dict()

    def copy_robust_to(self, device_ptr: int, trim_scale=None):
        p = robust_params(trim_scale)
        _check(load().surf_robust_copy_device(self._h, C.byref(p), C.c_void_p(device_ptr)), "surf_robust_copy_device", self._h)

    def denoise_nlm(self, **params):
        """(image, err) of the dual-buffer non-local-means filter on the halves of this context's sample buckets
        (surf_denoise_nlm; nlm_params' names): each half filtered with patch weights from the other, recombined by
        sample count -- (H, W, 4) float32 with w = 1 -- and the per-pixel error estimate from the two filtered halves'
        difference.  Reads no feature plane.  Needs set_sample_buckets; raises SURF_ERR_INVALID on a row shard (see
        denoise_nlm_image)."""
        p = nlm_params(**params)
        out, err = (np.zeros((self.height, self.width, 4), dtype=np.float32) for _ in range(2))
        _check(load().surf_denoise_nlm(self._h, C.byref(p), _ptr(out), _ptr(err)), "surf_denoise_nlm", self._h)
        return out, err

    def denoise_nlm_image(self, half0, half1, **params):
        """The same filter on two host half accumulators of any full frame (surf_denoise_nlm_image), e.g.
        bucket_halves() of planes assembled from row shards: (image, err)."""
        w, h, a, b, out, err = _nlm_planes(half0, half1)
        p = nlm_params(**params)
        _check(load().surf_denoise_nlm_image(self._h, w, h, _ptr(a), _ptr(b), C.byref(p), _ptr(out), _ptr(err)), "surf_denoise_nlm_image",
               self._h)
        return out, err

    def copy_denoise_nlm_to(self, device_ptr: int, err_device_ptr: int = None, **params):
        p = nlm_params(**params)
        _check(load().surf_denoise_nlm_copy_device(self._h, C.byref(p), C.c_void_p(device_ptr), C.c_void_p(err_device_ptr)),
               "surf_denoise_nlm_copy_device", self._h)

    def debug_nlm_time(self) -> list:
        """Device milliseconds of the last non-local-means run's launches (surf_debug_nlm_time): halves, prepare, filter."""
        ms = (C.c_float * 3)()
        _check(load().surf_debug_nlm_time(self._h, ms, 3), "surf_debug_nlm_time", self._h)
        return [float(v) for v in ms]

    def denoise_regress(self, **params):
        """(image, err) of the first-order feature regression filter (surf_denoise_regress; regress_params' names): each
        half of this context's sample buckets fitted around every pixel as a first-order function of normal, albedo and
        relative depth with the non-local-means patch weights of the other half, evaluated at the pixel; recombined
        and with an error estimate as denoise_nlm's.  Reads the planes set_filter_guides selects.  Needs
        set_sample_buckets; raises SURF_ERR_INVALID on a row shard (see denoise_regress_image)."""
        p = regress_params(**params)
        out, err = (np.zeros((self.height, self.width, 4), dtype=np.float32) for _ in range(2))
        _check(load().surf_denoise_regress(self._h, C.byref(p), _ptr(out), _ptr(err)), "surf_denoise_regress", self._h)
        return out, err

    def denoise_regress_image(self, half0, half1, planes, **params):
        """The same filter on host planes of any full frame (surf_denoise_regress_image): two half accumulators, e.g.
        bucket_halves() of planes assembled from row shards, and Renderer.aov()'s dict or (position, normal, albedo):
        (image, err)."""
        w, h, a, out, err = _regress_planes(half0, half1, planes)
        p = regress_params(**params)
        _check(load().surf_denoise_regress_image(self._h, w, h, *(_ptr(v) for v in a), C.byref(p), _ptr(out), _ptr(err)),
               "surf_denoise_regress_image", self._h)
        return out, err

    def copy_denoise_regress_to(self, device_ptr: int, err_device_ptr: int = None, **params):
        p = regress_params(**params)
        _check(load().surf_denoise_regress_copy_device(self._h, C.byref(p), C.c_void_p(device_ptr), C.c_void_p(err_device_ptr)),
               "surf_denoise_regress_copy_device", self._h)

    def debug_regress_time(self) -> list:
        """Device milliseconds of the last regression run's launches (surf_debug_regress_time): halves, prepare, filter."""
        ms = (C.c_float * 3)()
        _check(load().surf_debug_regress_time(self._h, ms, 3), "surf_debug_regress_time", self._h)
        return [float(v) for v in ms]

    def debug_robust_time(self) -> float:
        """Device milliseconds of the last k_robust launch (surf_debug_robust_time)."""
        return self._debug_ms("surf_debug_robust_time")

    def set_pixel_mask(self, mask):
        """The active-pixel mask of this shard (surf_set_pixel_mask): (rows, W) or flat, nonzero = active; None = every
        pixel.  render() then traces the active pixels only; the others' records stay untouched."""
        if mask is None:
            _check(load().surf_set_pixel_mask(self._h, None), "surf_set_pixel_mask", self._h)
            return
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if m.size != len(self.rows) * self.width:
            raise ValueError(f"mask of {m.size} pixels for a shard of {len(self.rows) * self.width}")
        _check(load().surf_set_pixel_mask(self._h, _ptr(m)), "surf_set_pixel_mask", self._h)

    def _surfel_planes(self, position, normal):
        """The two planes of a surfel sensor checked before the library sees them: float32, (rows, W, 4) or flat with
        rows*W*4 values each."""
        n = len(self.rows) * self.width * 4
        planes = []
        for name, a in (("position", position), ("normal", normal)):
            a = np.asarray(a)
            if a.dtype != np.float32:
                raise ValueError(f"set_surfel_sensor: {name} is {a.dtype}, not float32")
            if a.size != n or (a.ndim != 1 and a.shape != (len(self.rows), self.width, 4)):
                raise ValueError(f"set_surfel_sensor: {name} has shape {a.shape}, not ({len(self.rows)}, {self.width}, 4)")
            planes.append(np.ascontiguousarray(a))
        return planes

    def set_surfel_sensor(self, position, normal):
        """Starts this shard's samples at the caller's surface points (surf_set_surfel_sensor, which defines the sensor):
        position and normal (rows, W, 4) float32 (w ignored); a texel whose normal is (0, 0, 0) is invalid and never
        traced.  None, None: back to the camera.  accumulator() / w then estimates irradiance / pi at each texel."""
        if position is None and normal is None:
            _check(load().surf_set_surfel_sensor(self._h, None, None), "surf_set_surfel_sensor", self._h)
            return
        if position is None or normal is None:
            raise ValueError("set_surfel_sensor: one of position and normal is None")
        pos, nrm = self._surfel_planes(position, normal)
        _check(load().surf_set_surfel_sensor(self._h, _ptr(pos), _ptr(nrm)), "surf_set_surfel_sensor", self._h)

    def set_surfel_sensor_device(self, pos_ptr: int, nrm_ptr: int):
        """The same from two device pointers on this context's device (surf_set_surfel_sensor_device), e.g. the planes
        copy_aov_to wrote: rows*W float4 records each.  The library copies them."""
        if not pos_ptr or not nrm_ptr:
            raise ValueError("set_surfel_sensor_device: a device pointer is 0 (set_surfel_sensor(None, None) clears the sensor)")
        _check(load().surf_set_surfel_sensor_device(self._h, C.c_void_p(pos_ptr), C.c_void_p(nrm_ptr)),
               "surf_set_surfel_sensor_device", self._h)

    def sensor(self):
        """(kind, valid): SENSOR_CAMERA or SENSOR_SURFELS, and the valid texels (rows*W for the camera) (surf_get_sensor)."""
        k, v = C.c_int(), C.c_uint32()
        _check(load().surf_get_sensor(self._h, C.byref(k), C.byref(v)), "surf_get_sensor", self._h)
        return int(k.value), int(v.value)

    def bake(self, position, normal, frames: int, spp: int = 1, max_segments: int = 0, first_sample: int = 0) -> np.ndarray:
        """Sets the surfel sensor, clears the accumulator, renders `frames` frames of `spp` samples and returns the
        accumulator ((rows, W, 4): sum of energy, samples); the camera sensor is restored, the accumulator keeps the bake."""
        self.set_surfel_sensor(position, normal)
        try:
            self.clear_accumulator()
            self.render(frames, first_sample, max_segments, spp)
            return self.accumulator()
        finally:
            self.set_surfel_sensor(None, None)

    def pixel_mask(self):
        """(mask (rows, W) uint8, active count) as set (surf_get_pixel_mask)."""
        m, n = np.zeros((len(self.rows), self.width), np.uint8), C.c_uint32()
        _check(load().surf_get_pixel_mask(self._h, _ptr(m), C.byref(n)), "surf_get_pixel_mask", self._h)
        return m, int(n.value)

    def mask_from_noise(self, **params) -> int:
        """Builds the mask from this context's accumulator and squares and sets it (surf_mask_from_noise; parameters as
        adaptive_mask_params); returns the active count.  Refused on a row shard unless dilate=0."""
        p, n = adaptive_mask_params(**params), C.c_uint32()
        _check(load().surf_mask_from_noise(self._h, C.byref(p), C.byref(n)), "surf_mask_from_noise", self._h)
        return int(n.value)

    def adaptive_mask_image(self, acc, squares, **params):
        """The same rule on host planes of any (H, W, 4) frame (surf_adaptive_mask_image): (mask, ascending list)."""
        w, h, a, q, mask, lst = _mask_planes(acc, squares)
        p, n = adaptive_mask_params(**params), C.c_uint32()
        _check(load().surf_adaptive_mask_image(self._h, w, h, _ptr(a), _ptr(q), C.byref(p), _ptr(mask), _ptr(lst), C.byref(n)),
               "surf_adaptive_mask_image", self._h)
        return mask, lst[:n.value].copy()

    def render_adaptive(self, round_cap: int = 4096, **params) -> dict:
        """Renders until converged (surf_render_adaptive; parameters as adaptive_params): needs sample squares on and an
        empty accumulator.  Returns {'rounds', 'frames', 'active_last', 'samples', 'noise', 'round_active'}."""
        p, s = adaptive_params(**params), AdaptiveSummary()
        ra = np.zeros(max(1, round_cap), np.uint32)
        _check(load().surf_render_adaptive(self._h, C.byref(p), _ptr(ra), round_cap, C.byref(s)), "surf_render_adaptive", self._h)
        return {"rounds": int(s.rounds), "frames": int(s.frames), "active_last": int(s.active_last), "samples": int(s.samples),
                "noise": s.noise.as_dict(), "round_active": [int(v) for v in ra[:min(int(s.rounds), round_cap)]]}

    def error_mask_image(self, out, err, acc, **params):
        """The mask from the non-local-means filter's error estimate on host planes of any (H, W, 4) frame
        (surf_error_mask_image; parameters as error_mask_params): (mask, ascending list).  Leaves this context's mask alone."""
        w, h, o, e, a, mask, lst = _error_mask_planes(out, err, acc)
        p, n = error_mask_params(**params), C.c_uint32()
        _check(load().surf_error_mask_image(self._h, w, h, _ptr(o), _ptr(e), _ptr(a), C.byref(p), _ptr(mask), _ptr(lst), C.byref(n)),
               "surf_error_mask_image", self._h)
        return mask, lst[:n.value].copy()

    def mask_from_nlm(self, nlm=None, **params) -> int:
        """Filters the halves of this context's buckets, builds the mask from the filter's error estimate and sets it
        (surf_mask_from_nlm; nlm: a dict of nlm_params' fields, params as error_mask_params); returns the active count.
        Needs set_sample_buckets; refused on a row shard."""
        fp, p, n = nlm_params(**(nlm or {})), error_mask_params(**params), C.c_uint32()
        _check(load().surf_mask_from_nlm(self._h, C.byref(fp), C.byref(p), C.byref(n)), "surf_mask_from_nlm", self._h)
        return int(n.value)

    def render_adaptive_nlm(self, round_cap: int = 4096, **params) -> dict:
        """Renders until the filtered picture has converged (surf_render_adaptive_nlm; parameters as adaptive_nlm_params):
        needs sample buckets on and an empty accumulator.  Returns {'rounds', 'frames', 'active_last', 'samples', 'above',
        'max_error', 'round_active', 'image', 'err'}: image and err are the filter's two outputs of the final state."""
        p, s = adaptive_nlm_params(**params), AdaptiveNlmSummary()
        ra = np.zeros(max(1, round_cap), np.uint32)
        out, err = (np.zeros((self.height, self.width, 4), dtype=np.float32) for _ in range(2))
        _check(load().surf_render_adaptive_nlm(self._h, C.byref(p), _ptr(out), _ptr(err), _ptr(ra), round_cap, C.byref(s)),
               "surf_render_adaptive_nlm", self._h)
        return {"rounds": int(s.rounds), "frames": int(s.frames), "active_last": int(s.active_last), "samples": int(s.samples),
                "above": int(s.above), "max_error": np.float32(s.max_error),
                "round_active": [int(v) for v in ra[:min(int(s.rounds), round_cap)]], "image": out, "err": err}

    def debug_error_mask_time(self) -> list:
        """Device milliseconds of the last error mask's launches (surf_debug_error_mask_time): mask kernel, compaction."""
        ms = (C.c_float * 2)()
        _check(load().surf_debug_error_mask_time(self._h, ms, 2), "surf_debug_error_mask_time", self._h)
        return [float(v) for v in ms]

    def display(self, **params):
        """(RGBA8 words (H, W) uint32, the meter's result) of the display stage on this context's accumulator, each pixel
        divided by its own sample count (surf_display; display_params' names): metered or manual exposure, optional bloom,
        tone curve, transfer function, ordered dither.  Raises SURF_ERR_INVALID on a row shard (see display_image) and on an
        accumulator nothing was rendered into."""
        p, m = display_params(**params), DisplayMeterResult()
        out = np.zeros((self.height, self.width), dtype=np.uint32)
        _check(load().surf_display(self._h, C.byref(p), _ptr(out), C.byref(m)), "surf_display", self._h)
        return out, m.as_dict()

    def display_image(self, img, **params):
        """The same on any host (H, W, 4) float RGBA image (surf_display_image): a filter's output (w = 1), an accumulator
        or a robust accumulator (w = the count), e.g. one assembled from row shards."""
        w, h, a, out = _display_plane(img)
        p, m = display_params(**params), DisplayMeterResult()
        _check(load().surf_display_image(self._h, w, h, _ptr(a), C.byref(p), _ptr(out), C.byref(m)), "surf_display_image", self._h)
        return out, m.as_dict()

    def display_image_device(self, src_device_ptr: int, width: int, height: int, dst_device_ptr: int, **params) -> dict:
        """The same from a plane on this context's device (width*height*16 bytes, e.g. what copy_denoise_nlm_to filled) to
        width*height words there (surf_display_image_device); returns the meter's result."""
        p, m = display_params(**params), DisplayMeterResult()
        _check(load().surf_display_image_device(self._h, width, height, C.c_void_p(src_device_ptr), C.byref(p),
                                                C.c_void_p(dst_device_ptr), C.byref(m)), "surf_display_image_device", self._h)
        return m.as_dict()

    def debug_display_time(self) -> list:
        """Device milliseconds of the last display run's stages (surf_debug_display_time): meter, scale, blur, pack."""
        ms = (C.c_float * 4)()
        _check(load().surf_debug_display_time(self._h, ms, 4), "surf_debug_display_time", self._h)
        return [float(v) for v in ms]

    def atlas_build(self, scene_or_desc, charts, W: int, H: int) -> dict:
        """Rasterizes the charts' UV layouts into one surfel per texel of a W x H atlas (surf_atlas_build, which defines
        it): position, normal, albedo (H, W, 4) float32, ids (H, W, 4) uint32 = (chart, instance, primitive, cover), and
        the summary.  scene_or_desc: a Scene or a SceneDesc (only triangles, tri_ext, instances and materials are read).
        The atlas's size is its own; position and normal are what set_surfel_sensor / bake take."""
        _atlas_size("atlas_build", W, H)
        d, (arr, n), s = _atlas_desc(scene_or_desc), atlas_chart_array(charts), AtlasSummary()
        ok = 0 < W <= ATLAS_MAX_SIDE and 0 < H <= ATLAS_MAX_SIDE
        out = _atlas_out(W if ok else 1, H if ok else 1)
        _check(load().surf_atlas_build(self._h, C.byref(d), arr, n, W, H, *(_ptr(out[k]) for k in ATLAS_PLANES), C.byref(s)),
               "surf_atlas_build", self._h)
        out["summary"] = s.as_dict()
        return out

    def atlas_build_to(self, scene_or_desc, charts, W: int, H: int, position_ptr: int = 0, normal_ptr: int = 0, albedo_ptr: int = 0,
                       ids_ptr: int = 0) -> dict:
        """The same into planes on this context's device, W*H*16 bytes each, 0: not wanted (surf_atlas_build_device);
        returns the summary."""
        _atlas_size("atlas_build_to", W, H)
        d, (arr, n), s = _atlas_desc(scene_or_desc), atlas_chart_array(charts), AtlasSummary()
        ptrs = [C.c_void_p(p or None) for p in (position_ptr, normal_ptr, albedo_ptr, ids_ptr)]
        _check(load().surf_atlas_build_device(self._h, C.byref(d), arr, n, W, H, *ptrs, C.byref(s)), "surf_atlas_build_device", self._h)
        return s.as_dict()

    def atlas_finish(self, acc, albedo):
        """(light map (H, W, 4), valid (H, W) uint8) from an accumulator-form plane -- accumulator(), robust()'s, a filter's
        output with w = 1 -- and the build's albedo plane (surf_atlas_finish)."""
        W, H, a, b, out, valid = _atlas_finish_args(acc, albedo)
        _check(load().surf_atlas_finish(self._h, W, H, _ptr(a), _ptr(b), _ptr(out), _ptr(valid)), "surf_atlas_finish", self._h)
        return out, valid

    def atlas_finish_to(self, W: int, H: int, acc_ptr: int, albedo_ptr: int, out_ptr: int, valid_ptr: int):
        """The same between planes on this context's device (surf_atlas_finish_device); valid is W*H bytes."""
        _atlas_size("atlas_finish_to", W, H)
        _check(load().surf_atlas_finish_device(self._h, W, H, *(C.c_void_p(p or None) for p in (acc_ptr, albedo_ptr, out_ptr, valid_ptr))),
               "surf_atlas_finish_device", self._h)

    def atlas_dilate(self, rgba, valid, iterations: int = 2):
        """(rgba, valid) after `iterations` (0..64) gutter-fill passes: an invalid texel becomes the mean of its valid
        8-neighbours (surf_atlas_dilate)."""
        W, H, a, v, out, ov = _atlas_dilate_args(rgba, valid, iterations)
        _check(load().surf_atlas_dilate(self._h, W, H, _ptr(a), _ptr(v), int(iterations), _ptr(out), _ptr(ov)), "surf_atlas_dilate", self._h)
        return out, ov

    def atlas_dilate_to(self, W: int, H: int, rgba_ptr: int, valid_ptr: int, iterations: int, out_ptr: int, out_valid_ptr: int):
        """The same between planes on this context's device (surf_atlas_dilate_device)."""
        _atlas_size("atlas_dilate_to", W, H)
        _check(load().surf_atlas_dilate_device(self._h, W, H, C.c_void_p(rgba_ptr or None), C.c_void_p(valid_ptr or None), int(iterations),
                                               C.c_void_p(out_ptr or None), C.c_void_p(out_valid_ptr or None)),
               "surf_atlas_dilate_device", self._h)

    def debug_atlas_time(self) -> dict:
        """Device milliseconds of the last atlas runs (surf_debug_atlas_time): the build's setup (with the scan and the
        item count's readback), cover and resolve, the last finish, the last dilate; and whether the build ran the tile mapping."""
        ms, tiles = (C.c_float * 5)(), C.c_uint32()
        _check(load().surf_debug_atlas_time(self._h, ms, 5, C.byref(tiles)), "surf_debug_atlas_time", self._h)
        names = ("setup", "cover", "resolve", "finish", "dilate")
        return {**{k: float(v) for k, v in zip(names, ms)}, "tile_map": bool(tiles.value)}

    def bake_atlas(self, scene, charts, frames: int, iterations: int = 2, spp: int = 1, max_segments: int = 0,
                   first_sample: int = 0) -> dict:
        """A light map of this context's frame size with no host trip between the stages (surf_atlas_bake, in buffers of
        the library's own on this context's device): atlas_build on the device, the surfel sensor set from its planes, the
        accumulator cleared, `frames` frames rendered, finished and dilated `iterations` times.  The context must own every row (no shard); its width x height is the atlas.  Returns
        lightmap (H, W, 4), valid (H, W), accumulator (H, W, 4) and the build's summary; the camera sensor is restored, the
        accumulator keeps the bake."""
        W, H = self.width, self.height
        if len(self.rows) != H:
            raise ValueError("bake_atlas: a row shard cannot bake an atlas: the context must own every row")
        if not 0 <= int(iterations) <= ATLAS_MAX_ITERATIONS:
            raise ValueError(f"bake_atlas: iterations {iterations} outside 0..{ATLAS_MAX_ITERATIONS}")
        if int(frames) < 1 or int(spp) < 1:
            raise ValueError("bake_atlas: frames and spp must be at least 1")
        d, (arr, n), s = _atlas_desc(scene), atlas_chart_array(charts), AtlasSummary()
        out = {"lightmap": np.zeros((H, W, 4), np.float32), "valid": np.zeros((H, W), np.uint8), "accumulator": np.zeros((H, W, 4), np.float32)}
        _check(load().surf_atlas_bake(self._h, C.byref(d), arr, n, int(frames), first_sample, max_segments, int(spp), int(iterations),
                                      _ptr(out["lightmap"]), _ptr(out["valid"]), _ptr(out["accumulator"]), C.byref(s)),
               "surf_atlas_bake", self._h)
        out["summary"] = s.as_dict()
        return out

    def finalize_weighted(self, display: bool = False) -> np.ndarray:
        """RGBA8 with each pixel divided by its own sample count (surf_finalize_rgba8_weighted)."""
        out = np.zeros((len(self.rows), self.width), dtype=np.uint32)
        _check(load().surf_finalize_rgba8_weighted(self._h, 1 if display else 0, _ptr(out)), "surf_finalize_rgba8_weighted", self._h)
        return out

    def copy_accumulator_to(self, device_ptr: int):
        _check(load().surf_copy_accumulator_device(self._h, C.c_void_p(device_ptr)), "surf_copy_accumulator_device", self._h)

    def finalize_rgba8(self) -> np.ndarray:
        out = np.zeros((len(self.rows), self.width), dtype=np.uint32)
        _check(load().surf_finalize_rgba8(self._h, _ptr(out)), "surf_finalize_rgba8", self._h)
        return out

    def display_rgba8(self) -> np.ndarray:
        """The displayed image: fs_quad.frag's sqrt gamma on the RGBA8 finalize image."""
        out = np.zeros((len(self.rows), self.width), dtype=np.uint32)
        _check(load().surf_display_rgba8(self._h, _ptr(out)), "surf_display_rgba8", self._h)
        return out

    def stats(self) -> dict:
        s = Stats()
        _check(load().surf_get_stats(self._h, C.byref(s)), "surf_get_stats", self._h)
        return s.as_dict()

    def trace_closest(self, o: np.ndarray, d: np.ndarray):
        o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
        n = len(o)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        inst, prim = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        _check(load().surf_trace_closest(self._h, n, _ptr(o), _ptr(d), _ptr(t), _ptr(u), _ptr(v), _ptr(inst), _ptr(prim)),
               "surf_trace_closest", self._h)
        return t, u, v, inst, prim

    def trace_any(self, o: np.ndarray, d: np.ndarray, tmax: np.ndarray) -> np.ndarray:
        o = np.ascontiguousarray(o, dtype=np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, dtype=np.float32).reshape(-1, 3)
        tmax = np.ascontiguousarray(tmax, dtype=np.float32)
        occ = np.zeros(len(o), np.uint8)
        _check(load().surf_trace_any(self._h, len(o), _ptr(o), _ptr(d), _ptr(tmax), _ptr(occ)), "surf_trace_any", self._h)
        return occ

    def close(self):
        if self._h:
            load().surf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
