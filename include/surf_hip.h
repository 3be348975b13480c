/*
 * surf_hip.h -- C-ABI of the MI355X-native wavefront path tracer.
 *
 * This is the drop-in boundary for the reference's GPU path
 * (nemjit001/surf-path-tracer).  Each entry point names the reference
 * interface it replaces (paths relative to the reference repository root):
 *
 *   surf_create / surf_destroy      WaveFrontRenderer ctor/dtor (headers/renderer.h:211, sources/renderer.cpp:604-937)
 *   surf_upload_scene               GPUScene ctor: the 9 SSBOs + scene UBO (headers/scene.h:94-122, sources/scene.cpp:159-258)
 *   surf_update_instances           GPUScene::update re-upload (sources/scene.cpp:267-282)
 *   surf_set_camera                 CameraUBO upload (sources/renderer.cpp:971-979, headers/camera.h:12-19)
 *   surf_render                     WaveFrontRenderer::render dispatch loop (sources/renderer.cpp:1029-1118)
 *   surf_clear_accumulator          IRenderer::clearAccumulator (headers/renderer.h:91, sources/renderer.cpp:927-937)
 *   surf_read_accumulator           accumulator SSBO readback (headers/renderer.h:344-350)
 *   surf_finalize_rgba8             wavefront_finalize.comp:15-26 (+ RgbaToU32 rounding, sources/surf_math.cpp:13-29)
 *   surf_get_stats                  FrameInstrumentationData + Lumen energy (headers/renderer.h:30-34, sources/renderer.cpp:955-969)
 *   surf_trace_closest / _any       ray_extend.comp / ray_connect.comp traversal, exposed for hit-record tests
 *   surf_scene_build_indoor ...     host scene build of main.cpp:161-346 (Mesh/BvhBLAS/Instance/GPUBatcher)
 *
 * Conventions: every function returns 0 (SURF_OK) or a negative surf_status;
 * nothing aborts.  A context belongs to one HIP device and is driven from one
 * host thread.  Input records are byte-identical to the reference host structs
 * (sizes asserted below); the library re-lays them out internally (SoA queues,
 * child-box BVH nodes, BVH-ordered triangles).  Host buffers passed in are
 * copied; the caller keeps ownership.
 */
#ifndef SURF_HIP_H
#define SURF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SURF_ABI_VERSION 4

typedef enum {
    SURF_OK = 0,
    SURF_ERR_INVALID = -1,      /* bad argument / inconsistent scene */
    SURF_ERR_HIP = -2,          /* HIP runtime error (see surf_last_error) */
    SURF_ERR_NO_DEVICE = -3,    /* no gfx950 device at that index */
    SURF_ERR_NO_SCENE = -4,     /* render before upload */
    SURF_ERR_OOM = -5,          /* device allocation failed */
    SURF_ERR_IO = -6,           /* asset file unreadable */
    SURF_ERR_LIMIT = -7         /* scene exceeds a compiled limit (stack depth) */
} surf_status;

/* ---- reference record layouts (byte-identical; offsets in comments) ---- */

typedef struct { float x, y, z, _pad; } surf_float3_16;         /* ALIGN(16) Float3 slot */

typedef struct {                                                /* Triangle, mesh.h:14-25 (64 B) */
    surf_float3_16 v0, v1, v2, centroid;                        /* v0 = OBJ vertex 1, v1 = OBJ vertex 0 */
} surf_triangle;

typedef struct {                                                /* TriExtension, mesh.h:26-30 (80 B) */
    surf_float3_16 n0, n1, n2;                                  /* @0 @16 @32 */
    float uv0[2], uv1[2], uv2[2];                               /* @48 @56 @64 */
    float _pad[2];
} surf_tri_extension;

typedef struct {                                                /* BvhNode, bvh.h:36-46 (48 B) */
    uint32_t left_first, count, _pad[2];                        /* leaf iff count != 0 */
    surf_float3_16 bb_min, bb_max;                              /* @16 @32 */
} surf_bvh_node;

typedef struct {                                                /* Material, material.h:6-19 (64 B) */
    float emission_strength, reflectivity, refractivity, index_of_refraction;
    surf_float3_16 emission_color, albedo, absorption;          /* @16 @32 @48 */
} surf_material;

typedef struct {                                                /* GPUInstance, bvh.h:93-102 (160 B) */
    uint32_t tri_offset, bvh_idx_offset, bvh_node_offset, material_offset;
    float area;                                                 /* @16 */
    uint32_t _pad[3];
    float transform[16];                                        /* @32, glm column major */
    float inv_transform[16];                                    /* @96 */
} surf_gpu_instance;

typedef struct {                                                /* GPULightData, scene.h:67-71 (8 B) */
    uint32_t light_instance_idx, primitive_count;
} surf_light;

typedef struct {                                                /* SceneBackground, scene.h:18-26 (64 B) */
    uint32_t type;                                              /* 0 solid, 1 gradient */
    uint32_t _pad[3];
    surf_float3_16 color, gradient_a, gradient_b;               /* @16 @32 @48 */
} surf_background;

typedef struct {                                                /* CameraUBO, camera.h:12-19 (128 B) */
    surf_float3_16 position, up, fwd, right;                    /* @0 @16 @32 @48 */
    surf_float3_16 first_pixel, u_vector, v_vector;             /* @64 @80 @96 */
    float resolution[2];                                        /* @112 */
    float focal_length, defocus_angle;                          /* @120 @124 */
} surf_camera_ubo;

/* GPUScene's nine buffers + scene UBO (scene.h:113-122), host pointers. */
typedef struct {
    const surf_triangle* triangles;       uint32_t triangle_count;
    const surf_tri_extension* tri_ext;    /* triangle_count records */
    const uint32_t* blas_indices;         uint32_t blas_index_count;
    const surf_bvh_node* blas_nodes;      uint32_t blas_node_count;
    const surf_material* materials;       uint32_t material_count;
    const surf_gpu_instance* instances;   uint32_t instance_count;
    const uint32_t* tlas_indices;         /* instance_count records */
    const surf_bvh_node* tlas_nodes;      uint32_t tlas_node_count;
    const surf_light* lights;             uint32_t light_count;
    const surf_background* background;
} surf_scene_desc;

typedef struct {
    uint64_t samples;          /* camera samples rendered since the last clear (Mrays/s numerator, main.cpp:431) */
    uint64_t n_ext;            /* extension rays traced */
    uint64_t n_hit;            /* extension rays that hit geometry */
    uint64_t n_cont;           /* continuation rays */
    uint64_t n_shadow;         /* shadow rays traced */
    uint64_t n_acc;            /* radiance contributions */
    uint64_t n_unocc;          /* unoccluded shadow rays */
    uint64_t iterations;       /* wavefront iterations (extend->shade->connect->regen) */
    uint64_t tail_paths;       /* paths finished by the tail kernel */
    double   ms_total;         /* device time of render + drain calls since the last clear */
    double   ms_extend, ms_shade, ms_connect, ms_regen, ms_tail, ms_accum;  /* per-kernel (surf_set_profiling) */
    double   ms_sort;          /* the pool's ray-order sort (the shadow queue needs none), profiling mode */
    uint64_t launches_extend;  /* k_extend launches timed (profiling mode) */
    uint64_t n_ext_wavefront;  /* extension rays traced by k_extend (n_ext minus the drain's) */
    uint32_t stack_depth;      /* traversal stack entries reserved per ray */
    uint32_t pool_capacity;    /* paths in flight */
    float    energy;           /* sum of acc.rgb / samples over the shard ("Lumen", renderer.cpp:191-201) */
    uint32_t max_segments;     /* longest path seen (extension rays), diagnostics */
    uint64_t tail_survivors;   /* drain paths handed to the cooperative tail */
    uint32_t frame_window;     /* radiance ring slots (passes) of the current stream (surf_set_frame_batch), 0 before the first render */
    uint64_t n_shadow_overflow; /* wavefront shadow rays queued in the overflow region: their order bin's region was full */
} surf_stats;

typedef struct surf_ctx surf_ctx;       /* one per HIP device */
typedef struct surf_scene surf_scene;   /* host-side scene built by this library */

/* ---- version / device ---- */
int surf_abi_version(void);
int surf_device_count(int* count);

/* ---- context ----
 * Renders rows [row_begin, row_end) of a width x height frame (one shard). */
int surf_create(int hip_device, uint32_t width, uint32_t height,
                uint32_t row_begin, uint32_t row_end, surf_ctx** out);
/* Interleaved row blocks: block b = rows [b*row_block, (b+1)*row_block) goes to
 * shard b % shard_count. row_block 0 = contiguous split. */
int surf_create_sharded(int hip_device, uint32_t width, uint32_t height,
                        uint32_t shard_index, uint32_t shard_count, uint32_t row_block,
                        surf_ctx** out);
void surf_destroy(surf_ctx* ctx);
const char* surf_last_error(const surf_ctx* ctx);   /* ctx may be NULL: last global error */
/* Rows of this shard in shard order (row_count from surf_shard_rows(ctx, NULL, &n)). */
int surf_shard_rows(const surf_ctx* ctx, uint32_t* rows, uint32_t* row_count);
/* The HIP device the context was created on (the multi-GPU gather allocates
 * its buffers and streams there, whatever device the calling thread has set). */
int surf_get_device(const surf_ctx* ctx, int* hip_device);
/* The rows shard shard_index of shard_count owns under surf_create_sharded's
 * rule, in shard order (rows may be NULL to get the count).  Host only. */
int surf_shard_row_list(uint32_t height, uint32_t shard_index, uint32_t shard_count, uint32_t row_block, uint32_t* rows,
                        uint32_t* row_count);

/* Paths in flight (default: 5 full frames, W * H * 5, at most 16 M, whatever
 * the shard). Must be called before the first render. */
int surf_set_pool_capacity(surf_ctx* ctx, uint32_t paths);
/* Frame window: passes (samples per pixel; a frame of spp samples takes spp
 * consecutive passes) whose samples may be in flight at once -- a multiple of
 * the stream's samples_per_frame.  Default: the passes the stream being
 * started requests (one render call's frames x spp, rounded to a multiple of spp),
 * at least 256 -- 4096 for a stream opened by a one-frame request (a drop-in
 * loop extends its stream one frame per call) -- at most
 * 4096 and at most what min(64 GiB, a quarter of the free HBM) holds; a later
 * stream that requests more frames grows the ring (C3 at 1280x720: 256 frames
 * = 3.8 GB, a one-frame stream 4096 = 60 GB; C4 at 1920x1080: 1024 frames = 34 GB;
 * 64 GiB hold 2070 slots at 1080p).
 * Sample radiance is held per (frame slot, pixel) until a frame completes and
 * is accumulated in frame order; long Russian-roulette paths of old frames
 * overlap the bulk of newer ones.  A stream longer than the window issues
 * frame f only once frame f - window is accumulated.  Setting it fixes it
 * (must be called before the first render).  Several contexts on one device:
 * each sizes its default ring from the HBM free when its stream starts, so a
 * context started after another gets a smaller window (and, for a drop-in
 * loop, a lower throughput) -- fix the window here on each context for
 * predictable memory and throughput (memory: W * H * 16 B per slot). */
int surf_set_frame_batch(surf_ctx* ctx, uint32_t frames);
/* Throughput cutoff (enabled 1 / 0; -1 = automatic, the default: on for
 * streams of 1-sample frames, off for multi-sample frames, whose next sample
 * starts from the RNG state the reference's path ends with -- an early end
 * would change it, so there the cutoff is a deviation, not a neutral
 * shortcut): a path whose throughput T is below FLT_MIN
 * (1.17549435e-38) in every channel -- zero or denormal -- ends early.  The
 * reference's Russian roulette ends such a path with certainty at its next
 * diffuse bounce (p = max(T) < 2^-32, the smallest positive randomF32).  The
 * terms dropped are those the path would still add before that bounce: the
 * emitter hits along its chain of specular / dielectric bounces up to the next
 * diffuse bounce (any number of them), plus that bounce's NEE term -- each
 * below 1.2e-38 x (emission or light term):
 * radiance-neutral in f32 except for a pixel whose own energy is ~1e-38 (the
 * parity tests compare the GPU with the cutoff against the oracle without it,
 * bit for bit, on every tested image); n_ext/n_cont/... shrink.  It ends the
 * total-internal-reflection orbits in the glass lens that the reference traces
 * for up to millions of segments at a denormal throughput.
 * Stall risk with the cutoff off -- the automatic default for multi-sample
 * frames, e.g. a drop-in Renderer whose samplesPerFrame is above 1: such an
 * orbit runs to its end as in the reference (13,104,648 segments for one C3
 * path, frame 143, pixel 205912 at 1280x720 -- seconds of drain for the frame
 * holding it).  Bound it with max_segments (surf_render; a deviation, the
 * capped paths are counted and listed by surf_debug_capped) or enable the
 * cutoff (a deviation for multi-sample frames, see above). */
int surf_set_zero_cutoff(surf_ctx* ctx, int enabled);
/* Drain policy: when no new sample may be issued and at most `threshold_paths`
 * paths are in flight, the tail kernel finishes them in stages: each stage
 * runs `lanes_per_wave` paths per 64-lane wave for up to `stage_segments`
 * segments and hands the survivors to the next; once at most the
 * surf_set_tail_coop limit remain, the cooperative tail runs each on a whole
 * wave (0 = automatic for the first two; stage_segments 0 = a single lane
 * stage to the end; default 16).  Results do not depend on the policy.
 * Drains the context first. */
int surf_set_tail_policy(surf_ctx* ctx, uint32_t threshold_paths, uint32_t lanes_per_wave, uint32_t stage_segments);
/* Drain paths handed to the cooperative tail (default 150000, 0 = never): one
 * path per 64-lane wave with the lanes-as-planes traversal (any TLAS -- a
 * single-leaf TLAS walks its instances in a wave-uniform loop, any other the
 * TLAS DFS on the wave -- with a BVH stack of <= 64 entries; past 64
 * instances, materials or lights the tables are read from global memory), in
 * two-wave workgroups whose idle wave traces its sibling's shadow rays once
 * the path queue is empty (SURF_TAIL_PAIR=0 in the environment: one-wave
 * workgroups).  Identical results. */
int surf_set_tail_coop(surf_ctx* ctx, uint32_t max_paths);
/* Diagnostics: how many paths the segment cap ended in the current sample
 * stream, and the sample ids (frame slot * shard pixels + pixel) of up to
 * min(count, 64, max) of them (one per workgroup 0..63 that capped a path;
 * unused entries are 0xffffffff). */
int surf_debug_capped(surf_ctx* ctx, uint32_t* sample_ids, uint32_t max, uint64_t* count);
/* Diagnostics: shader-clock cycles of one drain segment's pieces on a lone
 * wave, each repeated `reps` times on the same path record path12 = (origin,
 * sample id bits), (direction, flag bits), (throughput, rng state bits):
 * cycles7[0] closest-hit wave walk, [1] shading, [2] the shadow ray's any-hit
 * walk, [3] the cosine sample alone, [4] the light sample alone, [5] the hit
 * normal alone (sums over reps); [6] a checksum; [7..14] with a walk-profile
 * build (SURF_WALK_PROFILE) the closest and any-hit walks' split: interior
 * cycles, leaf cycles, walks, leaves, triangles, two-level visits, prologue
 * cycles, instance-loop cycles (else 0).  No reference counterpart. */
int surf_debug_segment_cycles(surf_ctx* ctx, const float* path12, uint32_t reps, uint64_t* cycles15);
/* Diagnostics: the current sample stream's issue order.  permuted_frames is
 * the number of leading frames whose chain heads are issued heavy pixels
 * first (0: frame-major order throughout); heavy_pixels the size of that
 * heavy class (0 when permuted_frames is 0).  No reference counterpart. */
int surf_debug_issue_order(surf_ctx* ctx, uint32_t* heavy_pixels, uint32_t* permuted_frames);
/* Diagnostics: the emitters' BLAS staged in k_connect's LDS by the last phase
 * launched (blasAnyStaged): its compact interior records and its triangles,
 * both 0 when k_connect walked every BLAS from global memory.  No reference
 * counterpart. */
int surf_debug_connect_staging(surf_ctx* ctx, uint32_t* records, uint32_t* triangles);
/* Diagnostics: the shadow queue's order bin of n host rays under the context's
 * key layout (SURF_SH_KEY: 16, 32 or 40 bins; 1 bin when the shadow order is
 * off): o and d 3 floats per ray, tmax and the light slot one value per ray;
 * keys[i] < *bins, the number of bins in use.  layout (25 floats, or NULL)
 * receives what the key reads of the scene: the order cells' origin (3) and
 * scale (3), the number of heavy instances (0..3), then each one's padded
 * world box, lo (3) and hi (3), the heaviest first, zeros behind the last.
 * Needs an uploaded scene.  No reference counterpart. */
int surf_debug_shadow_keys(surf_ctx* ctx, uint32_t n, const float* o, const float* d, const float* tmax, const uint32_t* light,
                           uint32_t* keys, uint32_t* bins, float* layout);
/* Diagnostics: the kernel variants the uploaded scene selects (1 or 0 each):
 * trace and shading tables in LDS (at most 64 instances, materials, lights),
 * k_extend's 16-bit traversal stack (fewer than 65,536 BLAS and TLAS nodes, no
 * two-level lane walk, SURF_EXT_STACK16 not 0), the lane walk over the
 * two-level records (SURF_LANEW, or a BVH past 256 MB), and whether the
 * one-ray-per-wave engines may run (stack of at most 64 entries).  No
 * reference counterpart. */
int surf_debug_kernel_selection(surf_ctx* ctx, uint32_t* lds_tables, uint32_t* stack16, uint32_t* lane_two_level,
                                uint32_t* wave_eligible);
/* Diagnostics: the kernels' libm (gExpf, gSinf, gCosf, gSinCosf of
 * csrc/device/surf_math.h, the restatements of glibc's expf / sinf / cosf /
 * sincosf) on the device, compiled as the render kernels use them, one lane
 * per element of `in` (n floats).  out receives n floats, or for
 * SURF_MATH_SINCOSF 2n: (sin, cos) per element.  Needs no scene.  The header
 * states where each equals glibc bit for bit (expf everywhere, the others for
 * |y| < 120).  No reference counterpart. */
typedef enum { SURF_MATH_EXPF = 0, SURF_MATH_SINF = 1, SURF_MATH_COSF = 2, SURF_MATH_SINCOSF = 3 } surf_math_op;
int surf_debug_math(surf_ctx* ctx, int op, uint32_t n, const float* in, float* out);
/* ... and the same ops and output layout through the library's host build of
 * the same source (no context, no device): which side a device mismatch is on. */
int surf_debug_math_host(int op, uint32_t n, const float* in, float* out);
/* Diagnostics: planted paths.  Path i starts at o[3i..] toward d[3i..] with RNG
 * state seed[i] (as Renderer::trace is entered: throughput 1, no medium, the
 * last bounce specular) and is traced to its end on the device with the
 * render kernels' own device functions -- no camera, no seed derivation, no
 * queues:
 *   mode 0  one path per lane: the lane walk, shadePath<false> and the lane
 *           any-hit walk -- what k_extend, k_shade and k_connect run;
 *   mode 1  one path per wave: traceWave, shadePath<true> and the wave any-hit
 *           walk with the context's table staging -- what the cooperative
 *           drains run.  SURF_ERR_INVALID where surf_set_trace_mode(1) is.
 * A path's contributions are added in the reference's order
 * (renderer.cpp:338-444).  The throughput cutoff follows surf_set_zero_cutoff
 * (automatic: on, a planted path being a one-sample frame).  max_segments caps
 * the path as surf_render's does and must be 1..4096 (SURF_ERR_INVALID
 * otherwise), so no planted path can run without end.
 * out_energy_segments: 4 words per path -- the energy (3 floats) and the
 * number of segments (u32 bits); out_seed[i]: the RNG state after the path's
 * last draw.  Needs an uploaded scene.  No reference counterpart. */
int surf_debug_trace_paths(surf_ctx* ctx, uint32_t n, const float* o, const float* d, const uint32_t* seed, uint32_t max_segments,
                           int mode, float* out_energy_segments, uint32_t* out_seed);
/* When enabled, per-kernel device times are measured with HIP events on the
 * render stream (slower: disables the graph replay). */
int surf_set_profiling(surf_ctx* ctx, int enabled);

/* ---- scene / camera ---- */
int surf_upload_scene(surf_ctx* ctx, const surf_scene_desc* desc);
/* GPUScene::update's re-upload (scene.cpp:276-282): new instance records, TLAS
 * indices and nodes and lights for the uploaded BLASes/materials (same counts;
 * each instance must name a (node, index, triangle) offset triple of the
 * upload).  Drains the context first; geometry stays resident. */
int surf_update_instances(surf_ctx* ctx, const surf_gpu_instance* instances, uint32_t instance_count,
                          const uint32_t* tlas_indices, const surf_bvh_node* tlas_nodes, uint32_t tlas_node_count,
                          const surf_light* lights, uint32_t light_count);
int surf_set_camera(surf_ctx* ctx, const surf_camera_ubo* camera);

/* ---- rendering ----
 * Renders `frames` frames of samples_per_frame (spp) samples per pixel each,
 * as Renderer::render does per call (renderer.cpp:160-188): frame k is seeded
 * once per pixel with initSeed(pixel + 1799 * (first_sample_index + k * spp))
 * (renderer.cpp:169; first_sample_index = the accumulator's totalSamples
 * before this call, which is the frame index for spp 1), and its spp samples
 * run in sequence, sample j + 1's jitter, lens sample and path drawing from the
 * RNG state sample j's path left (renderer.cpp:171-181); (rgb, 1) is
 * accumulated per sample in sample order (renderer.cpp:180).  On the device a
 * frame's samples of one pixel form a chain: the kernel that ends sample j's
 * path (k_shade or a drain kernel) issues sample j + 1 in its place.
 * max_segments: 0 = unbounded + Russian roulette (reference semantics);
 * N > 0 caps each path at N extension rays.  Returns once every
 * sample is issued: consecutive calls form one sample stream, so the last long
 * paths of a call overlap the next call; any read (accumulator, stats,
 * finalize, synchronize) drains the stream first.  Scheduling only, identical
 * results (environment at surf_create, for A/B runs): a multi-frame call that
 * starts a stream issues every frame's samples of the pixels whose centre
 * camera ray first hits one of the largest BLASes first (SURF_REORDER=0:
 * frame-major); continuations are traced in the order of the large BLASes
 * they can reach, those reaching the most first (SURF_KEY=1: ascending,
 * 0: by start instance); each phase's shadow rays are
 * traced beside the next phase's extension (SURF_OVERLAP=0: serialized). */
int surf_render(surf_ctx* ctx, uint32_t frames, uint32_t first_sample_index,
                uint32_t max_segments, uint32_t samples_per_frame);
int surf_clear_accumulator(surf_ctx* ctx);
/* Float RGBA accumulator of this shard's rows, shard order, rows*width*4 floats. */
int surf_read_accumulator(surf_ctx* ctx, float* rgba_rows);
/* Device-to-device copy of the accumulator into dst (a device pointer on the
 * same device, rows*width*16 bytes): feeds the RCCL gather. */
int surf_copy_accumulator_device(surf_ctx* ctx, void* dst_device);
/* RGBA8 of acc / total samples with RgbaToU32 rounding, rows*width words. */
int surf_finalize_rgba8(surf_ctx* ctx, uint32_t* out_rgba8);
/* The displayed image: fs_quad.frag:22-24 (sqrt gamma) applied to the RGBA8
 * finalize image, written as 8-bit UNORM (round to nearest even), rows*width words. */
int surf_display_rgba8(surf_ctx* ctx, uint32_t* out_rgba8);
/* surf_finalize_rgba8 (display 0) / surf_display_rgba8 (display 1) of a host
 * accumulator, e.g. a frame assembled from row shards (surf_mgpu.h): n pixels
 * of RGBA floats times inv_samples, the same rounding as the kernels. */
int surf_pack_rgba8(const float* acc, uint32_t n, float inv_samples, int display, uint32_t* out_rgba8);
int surf_get_stats(surf_ctx* ctx, surf_stats* out);
int surf_synchronize(surf_ctx* ctx);

/* ---- first-hit feature buffers (AOVs) ----
 * What a denoiser, compositor or picking tool reads beside the radiance: per
 * pixel, the first hit of the pixel's unjittered camera ray -- from the camera
 * position through the pixel's corner ((x, row) / resolution on the view
 * plane, the ray the issue order's pixel classes use), WITHOUT jitter and
 * WITHOUT a lens sample even when the camera has a defocus angle: the planes
 * are sharp and noise-free.  No reference counterpart.  Four planes of
 * rows*width 16-byte records, shard row order like the accumulator:
 *   SURF_AOV_POSITION float4  hit (o + t*d, t)                 miss (0, 0, 0, 1e30)
 *   SURF_AOV_NORMAL   float4  hit (N, 0): the shading normal the path tracer
 *                             uses -- M * (u*n0 + v*n2 + w*n1, 0) normalized as a
 *                             vec4 (M, not its inverse transpose: Instance::normal),
 *                             turned against the ray; emitters too -- miss 0
 *   SURF_AOV_ALBEDO   float4  hit (albedo, 1); emitter (emission_strength *
 *                             emission_color, 1); miss (background along d, 0)
 *   SURF_AOV_ID       uint4   hit (instance, primitive, material index, 0)
 *                             miss (~0, ~0, ~0, 0)
 * All four are computed by one kernel on the first read and cached until
 * surf_set_camera changes the camera, surf_upload_scene or
 * surf_update_instances; the device buffers are allocated on first use
 * (SURF_ERR_OOM when that fails, SURF_ERR_NO_SCENE before a scene and a camera
 * are set, SURF_ERR_INVALID for a NULL argument or a plane outside 0..3).
 * A read never changes the sample stream: the accumulator and the event
 * counters after further renders are what they would be without it. */
typedef enum {
    SURF_AOV_POSITION = 0, SURF_AOV_NORMAL = 1, SURF_AOV_ALBEDO = 2, SURF_AOV_ID = 3, SURF_AOV_COUNT = 4
} surf_aov;
int surf_read_aov(surf_ctx* ctx, int plane, void* out);     /* host buffer, rows*width*16 bytes */
/* Device-to-device copy of a plane (dst on the same device, rows*width*16 bytes). */
int surf_copy_aov_device(surf_ctx* ctx, int plane, void* dst_device);
/* Diagnostics: device time (HIP events) of the last feature-buffer kernel
 * launch, 0 before the first.  No reference counterpart. */
int surf_debug_aov_time(surf_ctx* ctx, float* kernel_ms);

/* ---- feature buffers through mirrors and glass (the chain) ----
 * On a mirror or a glass pixel the first-hit planes describe the smooth
 * surface, not what is seen in it.  These planes follow the same unjittered
 * ray through the delta interactions -- a material with
 * reflectivity + refractivity >= 0.5 -- to the first surface that is not one,
 * or to the max_links-th link (0..SURF_AOV_CHAIN_MAX_LINKS).  No RNG anywhere;
 * all arithmetic f32 and uncontracted, in the path tracer's operand order, so
 * a host restatement reproduces every plane bit for bit.  No reference
 * counterpart.  State: tint = (1,1,1), L = 0.0f, inMedium = false, k = 0; then
 *   1. closest hit of (o, d) from depth 1e30; a miss is a terminal miss
 *   2. an emitter (emission_strength > 0 and a positive emission channel) is a
 *      terminal surface with a = emission_strength * emission_color and
 *      medium = (1,1,1) even inside a medium (the path tracer absorbs nothing
 *      on the segment that reaches an emitter); L, P, N as in 3
 *   3. L = L + t; medium_c = inMedium ? expf(absorption_c * (-t)) : 1;
 *      P = o + t*d; N = the shading normal of SURF_AOV_NORMAL, turned against d
 *   4. delta = (reflectivity + refractivity) >= 0.5f; if !delta or
 *      k == max_links: a terminal surface with a = albedo
 *   5. tint = tint * (albedo * medium).  reflectivity >= refractivity:
 *      R = d - (2*dot(N,d))*N.  Otherwise n1 = inMedium ? ior : 1,
 *      n2 = inMedium ? 1 : ior, ratio = n1 / n2, cosI = -dot(d,N),
 *      cos2 = 1 - (ratio*ratio) * (1 - cosI*cosI); cos2 > 0:
 *      R = ratio*d + (ratio*cosI - sqrtf(fabsf(cos2)))*N and inMedium toggles;
 *      else the mirror R and inMedium stays (total internal reflection).  There
 *      is no Fresnel draw: a dielectric transmits whenever it can
 *   6. o = P + 1e-5f*R, d = R, k = k + 1
 * The planes, laid out as surf_read_aov's:
 *   SURF_AOV_POSITION  surface (P, L): the terminal point ITSELF in world
 *                      space -- not a virtual point unfolded behind the mirror --
 *                      and the path length summed along the chain;
 *                      miss (0, 0, 0, 1e30)
 *   SURF_AOV_NORMAL    surface (N, 0), turned against the last d; miss 0
 *   SURF_AOV_ALBEDO    surface ((tint * medium) * a, 1);
 *                      miss (tint * background along the last d, 0)
 *   SURF_AOV_ID        surface (instance, primitive, material index, k);
 *                      miss (~0, ~0, ~0, k) -- k = the links followed
 * With max_links = 0 every plane equals surf_read_aov's bit for bit, and at
 * any max_links so does a pixel whose first hit is not delta.  The real
 * position keeps the a-trous filter's plane term dot(Pq - Pp, Np) consistent
 * inside a reflection; it makes the planes UNSUITABLE FOR REPROJECTION (a
 * reflected point does not move with the instance it lies on as the camera
 * sees it), so the temporal and the variance-guided filters keep the first-hit
 * planes.  Device planes of their own, computed by one kernel on the first
 * read and cached until what drops surf_read_aov's planes or a read with
 * another max_links; status codes as surf_read_aov, and SURF_ERR_INVALID for
 * max_links > SURF_AOV_CHAIN_MAX_LINKS.  A read never changes the sample
 * stream. */
#define SURF_AOV_CHAIN_MAX_LINKS 16
int surf_read_aov_chain(surf_ctx* ctx, int plane, uint32_t max_links, void* out);
int surf_copy_aov_chain_device(surf_ctx* ctx, int plane, uint32_t max_links, void* dst_device);
/* Diagnostics: device time (HIP events) of the last chain kernel launch, 0 before the first. */
int surf_debug_aov_chain_time(surf_ctx* ctx, float* kernel_ms);
/* Which planes the two purely spatial context filters read -- surf_denoise and
 * surf_denoise_sampled with their _copy_device forms: the first-hit planes (the
 * default) or the chain's at max_links.  No other filter is affected: the
 * temporal and variance-guided filters, surf_mask_from_noise and the adaptive
 * loop need reprojectable planes.  SURF_ERR_INVALID for an unknown mode or
 * max_links > SURF_AOV_CHAIN_MAX_LINKS (checked in either mode). */
typedef enum { SURF_GUIDES_FIRST_HIT = 0, SURF_GUIDES_CHAIN = 1 } surf_guides;
int surf_set_filter_guides(surf_ctx* ctx, int guides, uint32_t max_links);
int surf_get_filter_guides(const surf_ctx* ctx, int* guides, uint32_t* max_links);

/* ---- sampled feature buffers: anti-aliased AOVs and id coverage mattes ----
 * The first-hit planes come from one ray through the pixel's corner; the
 * radiance in the accumulator is the mean over the jitter box and the lens.
 * These planes reduce, per pixel, the first-hit features of the very camera
 * rays the render traces at one sample per frame, so with samples = the frames
 * rendered and first_sample = the first frame's index they describe the
 * samples that sit in the accumulator.  No reference counterpart.  All
 * arithmetic f32 and uncontracted, divisions IEEE, so a host restatement
 * reproduces every plane bit for bit.  Per shard pixel, p = x + row * width
 * over the whole frame (u32 wrap-around, as the render seeds), for
 * s = 0 .. samples-1 in order:
 *   1. seed = initSeed(p + 1799u * (first_sample + s))            (u32 wrap-around)
 *   2. jy = rndRange(seed, -0.5, 0.5), then jx likewise; with a defocus angle
 *      the lens disk: repeat sy = rndRange(seed, -1, 1), sx likewise, until
 *      sx*sx + sy*sy <= 1; origin = position + (sx*diskU + sy*diskV);
 *      u = ((float)x + jx) / width, v = ((float)row + jy) / height (as
 *      multiplications by the reciprocals); d = normalize(((first_pixel +
 *      u*u_vector) + v*v_vector) - origin): the render's primary ray
 *   3. closest hit of (o, d) from depth 1e30
 *   4. the sample's features are SURF_AOV_*'s expressions term for term:
 *      P = o + t*d and t; the shading normal N turned against d; a = albedo,
 *      or emission_strength * emission_color on an emitter, or the background
 *      along d for a miss; the ids
 * Running sums, f32 from 0.0f, ONE ADD PER SAMPLE IN SAMPLE ORDER (part of the
 * interface): nHit (u32); sum P (xyz), sum t and sum N (xyz) over the hit
 * samples; sum a (rgb) over ALL samples -- a miss adds the background.  Six
 * planes of rows*width 16-byte records, shard row order like surf_read_aov's:
 *   SURF_AOVS_POSITION    float4  nHit > 0: (sum P / (float)nHit, sum t / (float)nHit)
 *                                 else (0, 0, 0, 1e30)
 *   SURF_AOVS_NORMAL      float4  nHit > 0: (sum N / (float)nHit, 0) -- NOT renormalised:
 *                                 a pixel that straddles a crease gets a short normal; else 0
 *   SURF_AOVS_ALBEDO      float4  (sum a / (float)samples, (float)nHit / (float)samples):
 *                                 w is the hit coverage, 0 exactly when every sample missed
 *   SURF_AOVS_ID          uint4   sample 0's hit (instance, primitive, material index, nHit);
 *                                 sample 0 missed: (~0, ~0, ~0, nHit)
 *   SURF_AOVS_MATTE_KEY   uint4   the four highest-ranked keys
 *   SURF_AOVS_MATTE_COUNT uint4   their sample counts (integers; coverage is
 *                                 count / samples, left to the caller so it stays exact)
 * The first three keep the first-hit planes' layout and their "albedo.w != 0
 * means valid" convention: every filter reads them without change.
 * The matte: a sample's key is its instance index (SURF_MATTE_INSTANCE) or its
 * material index (SURF_MATTE_MATERIAL); a miss has key ~0 and is counted like
 * any key.  A table keeps the first 8 distinct keys in order of first
 * appearance, with their counts; a sample whose key is new once the table is
 * full is not counted (its share is samples - sum of counts).  Ranks are
 * ordered by count descending, ties by first appearance ascending; the four
 * best go out, empty ranks are key ~0 with count 0.  With samples = 1 the
 * matte is sample 0's key with count 1.
 * Device buffers of their own, computed by one launch on the first read and
 * cached until what drops surf_read_aov's planes (surf_set_camera,
 * surf_upload_scene, surf_update_instances) or a read with other params.  A
 * read never drains or changes the sample stream.  Row shards assemble to the
 * frame (the seed uses the whole-frame pixel index).  Frames of more than one
 * sample (samples_per_frame > 1) chain their RNG and are not described.
 * Status codes as surf_read_aov; SURF_ERR_INVALID for a NULL pointer, a plane
 * outside 0..5, samples 0 or above SURF_AOVS_MAX_SAMPLES, an unknown key or
 * reserved != 0. */
#define SURF_AOVS_MAX_SAMPLES 64
typedef enum {
    SURF_AOVS_POSITION = 0, SURF_AOVS_NORMAL = 1, SURF_AOVS_ALBEDO = 2, SURF_AOVS_ID = 3,
    SURF_AOVS_MATTE_KEY = 4, SURF_AOVS_MATTE_COUNT = 5, SURF_AOVS_COUNT = 6
} surf_aovs;
typedef enum { SURF_MATTE_INSTANCE = 0, SURF_MATTE_MATERIAL = 1 } surf_matte_key;
typedef struct {
    uint32_t samples;       /* 1..SURF_AOVS_MAX_SAMPLES */
    uint32_t first_sample;  /* frame index of sample 0 */
    uint32_t key;           /* SURF_MATTE_INSTANCE or SURF_MATTE_MATERIAL */
    uint32_t reserved;      /* 0 */
} surf_aov_sampled_params;
int surf_aov_sampled_default_params(surf_aov_sampled_params* p);   /* 16, 0, SURF_MATTE_INSTANCE, 0 */
int surf_read_aov_sampled(surf_ctx* ctx, const surf_aov_sampled_params* p, int plane, void* out);
int surf_copy_aov_sampled_device(surf_ctx* ctx, const surf_aov_sampled_params* p, int plane, void* dst_device);
/* Diagnostics: device time (HIP events) of the last sampled-planes kernel launch, 0 before the first. */
int surf_debug_aov_sampled_time(surf_ctx* ctx, float* kernel_ms);
/* Makes the filters that honour surf_set_filter_guides -- surf_denoise,
 * surf_denoise_sampled, surf_denoise_regress and their _copy_device forms --
 * read POSITION / NORMAL / ALBEDO of these planes at *p (computed if need be,
 * as a read computes them).  surf_get_filter_guides then reports
 * SURF_GUIDES_SAMPLED (2) and p->samples in max_links;
 * surf_set_filter_guides(ctx, 0 or 1, ...) switches back, and mode 2 stays
 * unknown to it.  The temporal and variance-guided filters and the two mask
 * builders keep the first-hit planes: they need reprojectable,
 * per-pixel-exact planes.  The default stays first hit.  SURF_ERR_INVALID as
 * surf_read_aov_sampled for the params. */
#define SURF_GUIDES_SAMPLED 2
int surf_set_filter_guides_sampled(surf_ctx* ctx, const surf_aov_sampled_params* p);

/* ---- ray-traced ambient occlusion and bent normals ----
 * The utility pass next to depth, normal, albedo and the mattes: from every
 * visible point, cosine-weighted any-hit rays of a given length; the share
 * that escapes is the openness, their mean direction the bent normal.  No
 * reference counterpart.  All arithmetic f32 and uncontracted, divisions IEEE,
 * so a host restatement reproduces both planes bit for bit.
 * The source planes of a shard pixel are the first-hit planes
 * (SURF_AO_FIRST_HIT) or the chain's at max_links (SURF_AO_CHAIN), computed
 * and cached exactly as a read of them would: P = position.xyz,
 * N = normal.xyz, valid = (albedo.w != 0); p = x + row * width over the whole
 * frame (u32 wrap-around, as the render seeds).  For a valid pixel, for
 * s = 0 .. samples-1:
 *   1. seed = initSeed((p + 1799u * (first_sample + s)) ^ SURF_AO_SEED_SALT)
 *      (u32 wrap-around; the salt keeps the draws off the render's own streams)
 *   2. R = the render's cosine-weighted direction about N from that seed: two
 *      draws r0, r1 per try, r = sqrtf(r0), theta = 2pi * r1, the glibc-exact
 *      sinf / cosf, dir = (r cos, r sin, sqrtf(1 - r0)) in the frame
 *      B = normalize(cross(N, |N.x| > 1 - 1e-5 ? (0,1,0) : (1,0,0))),
 *      T = cross(B, N): R = ((dir.x*T + dir.y*B) + dir.z*N); retried while
 *      R.N == 0
 *   3. O = P + bias * R (the render's continuation offset, bias in place of 1e-5)
 *   4. occluded = any hit of (O, R) within depth `radius`: the shadow rays' walk
 * nOpen = the number of unoccluded samples; S = the sum of the unoccluded R,
 * f32 from 0.0f, ONE ADD PER UNOCCLUDED SAMPLE IN SAMPLE ORDER (part of the
 * interface).  Two planes of rows*width 16-byte records, shard row order:
 *   SURF_AO_OPENNESS  float4  valid: (S / (float)nOpen, (float)nOpen / (float)samples);
 *                             xyz is 0 when nOpen == 0; the bent normal is NOT
 *                             renormalised: its length tells how tight the open
 *                             cone is.  invalid: (0, 0, 0, 1) -- the sky is open
 *   SURF_AO_BITS      uint4   valid: (mask bits 0-31, bits 32-63, nOpen, 1), bit s
 *                             set when sample s was unoccluded; invalid: (0, 0, 0, 0)
 * samples is one of 1, 2, 4, 8, 16, 32, 64, deliberately: a pixel's rays then
 * sit in one aligned lane group of a wave, and nOpen / samples is exact.
 * Occlusion is binary: the any-hit walk returns no distance, and that is what
 * makes it the fast walk; a distance falloff is not offered.  Shading normals
 * are used, as the render uses them, so on smooth meshes a few rays start
 * below the geometric surface and report the mesh itself; that is left as it
 * is.  radius and bias are finite or +inf, radius > 0, bias >= 0.
 * Device buffers of their own, computed by one launch on the first read and
 * cached until what drops surf_read_aov's planes (surf_set_camera,
 * surf_upload_scene, surf_update_instances) or a read with other params.  A
 * read never drains or changes the sample stream.  Row shards assemble to the
 * frame.  Status codes as surf_read_aov_sampled; SURF_ERR_INVALID for a NULL
 * pointer, a plane outside 0..1, samples not one of the seven, a radius or
 * bias outside its range, an unknown source, max_links above
 * SURF_AOV_CHAIN_MAX_LINKS or reserved != 0. */
#define SURF_AO_SEED_SALT 0x5AD0CC1Du
#define SURF_AO_MAX_SAMPLES 64
typedef enum { SURF_AO_OPENNESS = 0, SURF_AO_BITS = 1, SURF_AO_COUNT = 2 } surf_ao_plane;
typedef enum { SURF_AO_FIRST_HIT = 0, SURF_AO_CHAIN = 1 } surf_ao_source;
typedef struct {
    uint32_t samples;       /* 1, 2, 4, 8, 16, 32 or 64 */
    uint32_t first_sample;  /* index of sample 0 */
    float radius;           /* the rays' length, > 0 */
    float bias;             /* the origin's offset along the ray, >= 0 */
    uint32_t source;        /* SURF_AO_FIRST_HIT or SURF_AO_CHAIN */
    uint32_t max_links;     /* of the chain planes; ignored with SURF_AO_FIRST_HIT */
    uint32_t reserved[2];   /* 0 */
} surf_ao_params;
int surf_ao_default_params(surf_ao_params* p);   /* 16, 0, 1.0f, 1e-5f, SURF_AO_FIRST_HIT, 8, 0, 0 */
int surf_read_ao(surf_ctx* ctx, const surf_ao_params* p, int plane, void* out);
int surf_copy_ao_device(surf_ctx* ctx, const surf_ao_params* p, int plane, void* dst_device);
/* Diagnostics: device time (HIP events) of the last occlusion kernel launch, 0 before the first. */
int surf_debug_ao_time(surf_ctx* ctx, float* kernel_ms);

/* ---- denoiser: edge-avoiding a-trous wavelet filter on the feature buffers ----
 * A pure post-process of the radiance (Dammertz et al. 2010, with albedo
 * demodulation): it reads the accumulator and the first-hit feature planes
 * and writes a new image; the accumulator, the sample stream and the event
 * counters are what they would be without it.  No reference counterpart.
 *
 * The arithmetic is part of the interface: every operation is f32 and
 * uncontracted, in exactly the order written here, so a host restatement
 * reproduces the image bit for bit (surf_denoise_image_host is one).
 *
 * Inputs: a FULL frame of W x H pixels, rows top to bottom, as four float4
 * planes: acc (radiance sum, w = the sample count), position, normal, albedo
 * as surf_read_aov defines them (albedo.w == 0 marks a miss).  Parameters:
 * iterations n in 1..6, sigma_color, sigma_normal, sigma_plane (each finite
 * and > 0), demodulate (0 / 1).
 *
 * Prepare, per pixel p (k = x, y, z):
 *   valid = albedo.w != 0
 *   inv   = acc.w > 0 ? 1.0f / acc.w : 0.0f
 *   c_k   = acc_k * inv
 *   den_k = (valid && demodulate) ? (albedo_k > 0.01f ? albedo_k : 0.01f) : 1.0f
 *   I0_k  = c_k / den_k
 * Iteration i = 0..n-1, step s = 1 << i, with the f32 constants (host)
 *   sc = sigma_color * ldexpf(1.0f, -i)      kc = 1.0f / (sc * sc)
 *   kn = 1.0f / (sigma_normal * sigma_normal)
 *   kp = 1.0f / (sigma_plane * sigma_plane)
 * An invalid p copies I_i(p) to the next level unchanged.  A valid p starts
 * from sumW = 0, sum = (0, 0, 0) and visits the 25 taps q = (x + dx*s,
 * y + dy*s), dy = -2..2 the outer loop, dx = -2..2 the inner; a q outside the
 * frame or invalid is skipped; for every other q, the centre included:
 *   dC = Iq - Ip     dc = (dCx*dCx + dCy*dCy) + dCz*dCz
 *   dN = Nq - Np     dn = (dNx*dNx + dNy*dNy) + dNz*dNz
 *   dP = Pq - Pp     pl = (dPx*Npx + dPy*Npy) + dPz*Npz     dp = pl*pl
 *   e  = (dc*kc + dn*kn) + dp*kp
 *   e  = e < 100.0f ? e : 100.0f     (a NaN becomes 100; keeps the argument in
 *                                     the range the expf restatement is verified on)
 *   w  = (h[dy+2] * h[dx+2]) * expf(-e)     h = {0.0625, 0.25, 0.375, 0.25, 0.0625}
 *                                           expf: glibc 2.35's, as the path tracer's
 *   sumW  = sumW + w
 *   sum_k = sum_k + w * Iq_k
 * and then I_{i+1}(p)_k = sum_k / sumW (the centre tap makes sumW > 0).
 * Output: (I_n * den, 1.0f) for a valid pixel, (c, 1.0f) for a miss; with
 * w = 1, surf_pack_rgba8(out, n, 1.0f, display, ...) gives the displayable image.
 *
 * Known limit: the guides are the first hit of the sharp centre ray.  What is
 * seen THROUGH the lens blur or in a mirror has no guide edges, only the
 * colour term protects it; fireflies survive as well (surf_firefly_image
 * below clamps them in the accumulator beforehand).
 *
 * One launch per iteration (the last fuses the remodulation) on a 32 x 8
 * pixel tile per 256-thread block, in two variants with identical bits: taps
 * from an LDS copy of the tile and its 2*s halo, or straight from global
 * memory.  SURF_DENOISE_LDS=<largest step staged> (read at surf_create*; 0 =
 * never; steps above 4 are never staged, their halo outgrows its reuse).
 * Scratch images are allocated on first use and kept (no allocation in
 * steady state), freed by surf_destroy. */
typedef struct {
    uint32_t iterations;
    float sigma_color, sigma_normal, sigma_plane;
    uint32_t demodulate;
    uint32_t _pad[3];
} surf_denoise_params;
/* 5 iterations, sigma_color 1.0, sigma_normal 0.3, sigma_plane 0.1, demodulate 1 */
int surf_denoise_default_params(surf_denoise_params* params);
/* The context's accumulator filtered with its own (cached) feature planes, to
 * a host buffer of width*height*4 floats.  Drains the stream, as every read
 * does; leaves the accumulator untouched.  The context must own every row
 * 0..height-1: on a row shard SURF_ERR_INVALID (surf_last_error points to
 * surf_denoise_image -- a spatial filter needs its neighbours' rows).
 * SURF_ERR_NO_SCENE before a scene and a camera are set, SURF_ERR_OOM when a
 * scratch image cannot be allocated, SURF_ERR_INVALID for a NULL argument,
 * iterations outside 1..6 or a sigma that is not finite and > 0. */
int surf_denoise(surf_ctx* ctx, const surf_denoise_params* params, float* out_rgba);
/* The same, to a buffer on the context's device (width*height*16 bytes). */
int surf_denoise_copy_device(surf_ctx* ctx, const surf_denoise_params* params, void* dst_device);
/* Host planes of any full frame (w*h*4 floats each), e.g. one assembled from
 * row shards; needs no scene on the context.  SURF_ERR_INVALID also for w or
 * h of 0. */
int surf_denoise_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* acc, const float* position, const float* normal,
                       const float* albedo, const surf_denoise_params* params, float* out);
/* The CPU twin: the same per-pixel functions compiled for the host; needs no
 * device.  Bit-identical to surf_denoise_image. */
int surf_denoise_image_host(uint32_t w, uint32_t h, const float* acc, const float* position, const float* normal,
                            const float* albedo, const surf_denoise_params* params, float* out);
/* Diagnostics: device time (HIP events) of each kernel of the last denoise run
 * on this context: kernel_ms[0] the prepare kernel, kernel_ms[1 + i]
 * iteration i; entries past the run's iterations (and past 7) are 0. */
int surf_debug_denoise_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);

/* ---- temporal accumulation with reprojection ----
 * The temporal half of SVGF (Schied et al. 2017), the partner of the a-trous
 * filter above: when the camera or an instance moves and the application
 * clears the accumulator, last frame's result is reprojected onto this
 * frame's pixels through the first-hit feature buffers and blended with this
 * frame's samples, instead of starting again from one noisy sample set.  A
 * pure post-process: the accumulator, the sample stream and the event
 * counters are what they would be without it.  No reference counterpart.
 * Per displayed frame: update the scene and the camera, surf_clear_accumulator,
 * surf_render(1, first_sample_index, 0, spp), surf_temporal_accumulate.
 *
 * The arithmetic is part of the interface: every operation is f32 and
 * uncontracted, / and sqrtf are IEEE, rintf (to nearest even) and floorf are
 * exact, in exactly the order written here (surf_temporal_image_host is a
 * host restatement).  dot(a, b) below is (ax*bx + ay*by) + az*bz.
 *
 * Inputs, per pixel p = (x, y) of a FULL frame of W x H pixels, rows top to
 * bottom: A the accumulator (rgb sum, w = samples), P the position plane
 * (xyz, w = the ray depth t), N the normal plane, ID the id plane (x = the
 * instance, ~0 on a miss), as surf_read_aov defines them.  Of the previous
 * frame: the history Hq = (rgb, n) with n the history length as a float, its
 * position plane Pq, normal plane Nq and instance ids, its camera, and both
 * frames' instance records (the same count).
 * Host, per instance i: moved_i = its transform or its inv_transform differs
 * bytewise between the two frames; V = this frame's inv_transform, T = the
 * previous frame's transform (16 floats, column-major).  An id that is not
 * below the instance count counts as not moved.
 * Host, from the previous camera (C = position, F0 = first_pixel, U =
 * u_vector, V = v_vector, res = resolution):
 *   G  = F0 - C                 n = U x V  (nx = Uy*Vz - Uz*Vy, ny = Uz*Vx - Ux*Vz, nz = Ux*Vy - Uy*Vx)
 *   g  = dot(G, n)              iu = 1.0f / dot(U, U)      iv = 1.0f / dot(V, V)
 * Parameters: alpha_min in [0, 1], max_history >= 1, normal_min in [-1, 1],
 * plane_tol and min_weight finite and > 0, snap in [0, 0.5).
 *
 * 1. Colour: inv = A.w > 0 ? 1.0f / A.w : 0.0f, c = A.rgb * inv.
 * 2. Miss (ID.x == ~0): out = (c, 1), hist = (c, 0); nothing else.
 * 3. Previous position and normal.  Not moved: Pprev = P.xyz, Nprev = N.xyz.
 *    Moved, k = 0..2:
 *      q_k     = ((V[k]*Px + V[4+k]*Py) + V[8+k]*Pz) + V[12+k]
 *      Pprev_k = ((T[k]*qx + T[4+k]*qy) + T[8+k]*qz) + T[12+k]
 *      qn_k    = (V[k]*Nx + V[4+k]*Ny) + V[8+k]*Nz
 *      m_k     = (T[k]*qnx + T[4+k]*qny) + T[8+k]*qnz
 *      il      = 1.0f / sqrtf((mx*mx + my*my) + mz*mz)       Nprev_k = m_k * il
 * 4. Projection into the previous frame:
 *      D = Pprev - C      dn = dot(D, n)      s = g / dn      H_k = D_k*s - G_k
 *      fx = (dot(H, U) * iu) * res.x          fy = (dot(H, V) * iv) * res.y
 *    No history unless s > 0, -1 < fx < W and -1 < fy < H (a NaN fails).
 * 5. Snap: rx = rintf(fx); if fabsf(fx - rx) <= snap then fx = rx; fy alike.
 *    (An unmoved pixel under an unmoved camera lands within 1e-4 px of itself:
 *    the snap makes its history a single tap of weight 1, so a still image
 *    does not blur a little more every frame.)
 * 6. Taps: ix = (int)floorf(fx), tx = fx - floorf(fx); iy, ty alike.  From
 *    sumW = sumN = 0, sumC = 0 the texels (ix, iy), (ix+1, iy), (ix, iy+1),
 *    (ix+1, iy+1) in this order, with the weights w = (1-tx)*(1-ty),
 *    tx*(1-ty), (1-tx)*ty, tx*ty.  A tap q is used when it is inside the
 *    frame, w > 0, its previous instance id equals ID.x, Hq.w > 0,
 *    dot(Nq, Nprev) >= normal_min and
 *    fabsf(dot(Pprev - Pq, Nq)) <= plane_tol * P.w; then
 *      sumW = sumW + w     sumC_k = sumC_k + w*Hq_k     sumN = sumN + w*Hq.w
 * 7. Blend, with have = sumW > min_weight, hc = sumC / sumW, hn = sumN / sumW:
 *      have, A.w > 0:   n' = hn + 1.0f, at most (float)max_history;
 *                       a = 1.0f / n', at least alpha_min;
 *                       r_k = hc_k + (c_k - hc_k) * a
 *      have, A.w == 0:  r = hc, n' = hn
 *      not have:        r = c,  n' = A.w > 0 ? 1 : 0
 *    Without a previous frame every hit pixel takes "not have".
 * 8. out = (r, 1), hist = (r, n').
 *
 * Known limits: shadows and reflections OF a moving object lag behind it
 * until max_history or alpha_min ages them out; the guides are the sharp
 * first hit, so what is seen through the lens or in a mirror reprojects by
 * its glass or mirror surface; misses keep no history.
 *
 * One launch per frame, 256 threads on a 32 x 8 pixel tile; taps are read
 * straight from global memory (three 16-byte loads each), and so is the
 * motion table (25 floats per instance) whatever the instance count: an LDS
 * copy of it was measured and is slower. */
typedef struct {
    float alpha_min;
    uint32_t max_history;
    float normal_min, plane_tol, snap, min_weight;
    uint32_t _pad[2];
} surf_temporal_params;
/* alpha_min 0.0, max_history 32, normal_min 0.9, plane_tol 0.01, snap 1/64, min_weight 0.01 */
int surf_temporal_default_params(surf_temporal_params* params);
/* One frame of the loop above: the context's accumulator and (cached) feature
 * planes blended with the state the previous call stored, to a host buffer of
 * width*height*4 floats; then this frame's history (the unfiltered blend,
 * whatever `spatial` is), copies of its guides, its camera and its instance records are
 * stored on the context for the next call.  With `spatial` non-NULL the
 * returned image is surf_denoise's filter applied to the blend as the
 * accumulator (w = 1) with this frame's planes; NULL: the blend itself.
 * Drains the stream, as every read does.  The stored state survives
 * surf_clear_accumulator, surf_set_camera and surf_update_instances (that is
 * the point); surf_upload_scene and surf_temporal_reset drop it.  Buffers
 * are allocated on first use and kept, freed by surf_destroy.
 * SURF_ERR_INVALID on a row shard (surf_last_error points to
 * surf_temporal_image), for a NULL argument, alpha_min outside [0, 1],
 * max_history 0, normal_min outside [-1, 1], plane_tol or min_weight not
 * finite and > 0, snap outside [0, 0.5), invalid spatial parameters;
 * SURF_ERR_NO_SCENE before a scene and a camera are set; SURF_ERR_OOM. */
int surf_temporal_accumulate(surf_ctx* ctx, const surf_temporal_params* params, const surf_denoise_params* spatial, float* out_rgba);
/* The same, to a buffer on the context's device (width*height*16 bytes). */
int surf_temporal_copy_device(surf_ctx* ctx, const surf_temporal_params* params, const surf_denoise_params* spatial, void* dst_device);
/* Drops the stored state: the next surf_temporal_accumulate is a first frame. */
int surf_temporal_reset(surf_ctx* ctx);
/* (rgb, n) of the stored history, width*height*4 floats; SURF_ERR_INVALID before the first accumulate. */
int surf_temporal_history(surf_ctx* ctx, float* out_rgbn);
/* Host planes of any two full frames (w*h*16 bytes each), e.g. assembled from
 * row shards; needs no scene on the context and neither reads nor changes its
 * stored state.  instances: surf_gpu_instance records (their transforms are
 * what is read; NULL with a count of 0). */
typedef struct {
    const float* acc;
    const float* position;
    const float* normal;
    const uint32_t* id;
    const surf_gpu_instance* instances;
    uint32_t instance_count;
    uint32_t _pad;
} surf_temporal_frame;
typedef struct {
    const float* history;
    const float* position;
    const float* normal;
    const uint32_t* id;
    const surf_gpu_instance* instances;
    uint32_t instance_count;
    uint32_t _pad;
    surf_camera_ubo camera;
} surf_temporal_prev;
/* prev NULL: a first frame.  out_rgba and out_history: w*h*4 floats each.
 * SURF_ERR_INVALID also for w or h of 0, a NULL plane and instance counts
 * that differ between the two frames. */
int surf_temporal_image(surf_ctx* ctx, uint32_t w, uint32_t h, const surf_temporal_frame* cur, const surf_temporal_prev* prev,
                        const surf_temporal_params* params, float* out_rgba, float* out_history);
/* The CPU twin: the same per-pixel function compiled for the host; needs no
 * device.  Bit-identical to surf_temporal_image. */
int surf_temporal_image_host(uint32_t w, uint32_t h, const surf_temporal_frame* cur, const surf_temporal_prev* prev,
                             const surf_temporal_params* params, float* out_rgba, float* out_history);
/* Diagnostics: device time (HIP events) of the last k_temporal launch on this context, 0 before the first. */
int surf_debug_temporal_time(surf_ctx* ctx, float* kernel_ms);

/* ---- variance-guided filter ----
 * The piece of SVGF that joins the two halves above: the first and second
 * moment of luminance ride the temporal accumulation's reprojection, become a
 * per-pixel variance (estimated spatially where the history is too short to
 * trust), and that variance -- not one global sigma_color -- sets the a-trous
 * filter's colour edge-stopping width and is filtered along with the colour.
 * A pixel disoccluded this frame, or every pixel after a cut or a
 * surf_temporal_reset, gets a wide filter; a pixel with a long history a
 * narrow one.  A pure post-process, like the two above; no reference
 * counterpart.  The loop is surf_temporal_accumulate's with
 * surf_svgf_accumulate in its place.
 *
 * The arithmetic is part of the interface (f32, uncontracted, / and sqrtf
 * IEEE, expf glibc 2.35's, in exactly this order; surf_svgf_image_host is a
 * host restatement).  lum(v) = (0.2126f*vx + 0.7152f*vy) + 0.0722f*vz.
 * Inputs: those of the temporal accumulation and the albedo plane (albedo.w
 * == 0 marks an invalid pixel, as for the denoiser), and of the previous
 * frame its moments plane Mq = (mu1, mu2, m, 0): the running first and second
 * moment of luminance and the moments' own history length (none: every m = 0).
 * Parameters: surf_temporal_params, and iterations n in 1..6, sigma_lum,
 * sigma_normal, sigma_plane and variance_eps finite and > 0, demodulate
 * 0 / 1, spatial_below >= 1.  den is the denoiser's (Prepare above) with this
 * call's demodulate; kn, kp are the denoiser's from sigma_normal, sigma_plane.
 *
 * A. Moments through time.  Steps 1 - 8 of the temporal accumulation run
 *    unchanged: out = (r, 1) and hist = (r, n') are bit for bit what
 *    surf_temporal_accumulate gives.  Beside them, from sumWm = 0, sumM = 0:
 *    for every tap q that step 6 uses, when Mq.z > 0:
 *      sumWm = sumWm + w     sumM_k = sumM_k + w*Mq_k   (k = x, y, z)
 *    With the quotients taken first, d_k = c_k / den_k and l = lum(d); with
 *    haveM = have && sumWm > min_weight and hm = sumM / sumWm:
 *      haveM, A.w > 0:   m' = hm.z + 1.0f, at most (float)max_history;
 *                        am = 1.0f / m', at least alpha_min;
 *                        mu1' = hm.x + (l - hm.x) * am
 *                        mu2' = hm.y + (l*l - hm.y) * am
 *      haveM, A.w == 0:  M' = (hm.x, hm.y, hm.z, 0)
 *      not haveM:        M' = A.w > 0 ? (l, l*l, 1, 0) : (0, 0, 0, 0)
 *      a miss (step 2):  M' = (0, 0, 0, 0)
 * B. Variance.  An invalid pixel: v = 0.  A valid pixel p with m' = M'(p).z
 *    and sb = (float)spatial_below:
 *      m' >= sb:  t = mu2' - mu1'*mu1';  v = t > 0 ? t : 0
 *      m' <  sb:  from sw = s1 = s2 = 0 the 49 taps q = (x + dx, y + dy),
 *                 dy = -3..3 the outer loop, dx = -3..3 the inner; a q outside
 *                 the frame, invalid or with M'(q).z == 0 is skipped; for
 *                 every other q, the centre included, dn and dp as the
 *                 denoiser's (dN = Nq - Np, dP = Pq - Pp, pl = dot(dP, Np)):
 *                   e = dn*kn + dp*kp;  e = e < 100.0f ? e : 100.0f
 *                   wq = expf(-e)
 *                   sw = sw + wq   s1 = s1 + wq*M'(q).x   s2 = s2 + wq*M'(q).y
 *                 sw > 0:  a1 = s1 / sw, a2 = s2 / sw, t = a2 - a1*a1,
 *                          t = t > 0 ? t : 0, b = sb / (m' > 1.0f ? m' : 1.0f)
 *                          (the quotient first), v = t * b
 *                 else     v = 0
 *    Level 0 of the filtered image is I0 = (r / den, v): the variance rides in
 *    the image's w.  (An invalid pixel has den = 1: (r, 0).)
 * C. Iteration i = 0..n-1, step s = 1 << i.  An invalid p copies I_i(p) to the
 *    next level.  A valid p first takes, from gs = gw = 0, the 3 x 3 taps
 *    q = (x + dx, y + dy), dy = -1..1 outer, dx = -1..1 inner, inside the frame
 *    and valid, with g = {1/16, 1/8, 1/16;  1/8, 1/4, 1/8;  1/16, 1/8, 1/16}:
 *      gs = gs + g*Iq.w     gw = gw + g
 *    then gv = gs / gw and kl = 1.0f / (sigma_lum * sqrtf(gv) + variance_eps)
 *    (sigma_lum is not halved per iteration: the shrinking variance does that),
 *    then the denoiser's 25 taps with its skips, dn, dp and h, and
 *      dl = fabsf(lum(Iq) - lum(Ip))
 *      e  = (dl*kl + dn*kn) + dp*kp;  e = e < 100.0f ? e : 100.0f
 *      w  = (h[dy+2] * h[dx+2]) * expf(-e)
 *      sumW = sumW + w   sum_k = sum_k + w*Iq_k   sumV = sumV + (w*w)*Iq.w
 *    and I_{i+1}(p) = (sum / sumW, sumV / (sumW*sumW)).
 *    Output: (I_n.rgb * den, 1) for a valid pixel, (I_n.rgb, 1) otherwise.
 *
 * Off by default, see "extensions" below: the paper feeds the first filtered
 * iteration back into the history -- here the history stays the unfiltered
 * blend unless surf_svgf_ext.feedback asks for it; and without the firefly
 * clamp (surf_svgf_ext.firefly_scale) one very bright sample in a short
 * history means a large variance and a wide filter around it.  The guides'
 * limits are the denoiser's.
 *
 * Launches per frame, 256 threads on a 32 x 8 pixel tile each: k_temporal's
 * moments instantiation (a fourth 16-byte load per used tap), the packed
 * guides, the variance estimate, n iterations.  The variance kernel exists
 * in two variants with identical bits: the tile and its halo of 3 -- 38 x 14
 * texels of normal, position and moments, 25 536 bytes -- staged in LDS
 * (the default), or its taps straight from global memory (SURF_SVGF_LDS=0,
 * read at surf_create*).  SURF_DENOISE_LDS governs the iterations as it does
 * the denoiser's; their staged tile has the same layout, the image's w now
 * carrying the variance.  Buffers are allocated on first use and kept. */
typedef struct {
    uint32_t iterations;
    float sigma_lum;
    float sigma_normal, sigma_plane;
    uint32_t demodulate;
    uint32_t spatial_below;
    float variance_eps;
    uint32_t _pad;
} surf_svgf_params;
/* 5 iterations, sigma_lum 4.0, sigma_normal 0.3, sigma_plane 0.1, demodulate 1, spatial_below 4, variance_eps 1e-10 */
int surf_svgf_default_params(surf_svgf_params* params);
/* One frame of the loop, as surf_temporal_accumulate: the context's
 * accumulator and (cached) feature planes against the stored state, the
 * filtered image to a host buffer of width*height*4 floats.  It shares the
 * stored temporal state with surf_temporal_accumulate -- history (the
 * unfiltered blend; surf_svgf_accumulate_ex can store the filtered one), guide copies, camera, instance records, with the same
 * lifetime -- and adds the moments.  The two calls may be mixed:
 * surf_temporal_accumulate leaves the stored moments marked absent, so the
 * next surf_svgf_accumulate sees m = 0 everywhere and estimates spatially
 * until the moments have a history again.  surf_temporal_reset and
 * surf_upload_scene drop the moments with the history.  Status codes as
 * surf_temporal_accumulate (on a row shard surf_last_error points to
 * surf_svgf_image); SURF_ERR_INVALID also for iterations outside 1..6,
 * spatial_below 0, and a sigma or variance_eps that is not finite and > 0. */
int surf_svgf_accumulate(surf_ctx* ctx, const surf_temporal_params* params, const surf_svgf_params* svgf, float* out_rgba);
/* The same, to a buffer on the context's device (width*height*16 bytes). */
int surf_svgf_copy_device(surf_ctx* ctx, const surf_temporal_params* params, const surf_svgf_params* svgf, void* dst_device);
/* The stored moments (mu1, mu2, m, 0), width*height*4 floats; SURF_ERR_INVALID
 * when none are stored (before the first surf_svgf_accumulate, after a
 * surf_temporal_accumulate, a reset or a scene upload). */
int surf_svgf_moments(surf_ctx* ctx, float* out);
/* Of the last surf_svgf_accumulate, per pixel: x = the variance entering the
 * filter (I0.w), y = the variance leaving it (I_n.w, 0 for an invalid pixel),
 * z = w = 0.  SURF_ERR_INVALID as surf_svgf_moments. */
int surf_svgf_variance(surf_ctx* ctx, float* out);
/* Host planes of any two full frames, as surf_temporal_image: the temporal
 * structs plus the albedo plane and the previous moments (NULL: every m = 0). */
typedef struct {
    const float* acc;
    const float* position;
    const float* normal;
    const uint32_t* id;
    const surf_gpu_instance* instances;
    uint32_t instance_count;
    uint32_t _pad;
    const float* albedo;
} surf_svgf_frame;
typedef struct {
    const float* history;
    const float* position;
    const float* normal;
    const uint32_t* id;
    const surf_gpu_instance* instances;
    uint32_t instance_count;
    uint32_t _pad;
    surf_camera_ubo camera;
    const float* moments;
} surf_svgf_prev;
/* prev NULL: a first frame.  Four outputs of w*h*4 floats each: the filtered
 * image, the history (rgb, n'), the moments M' and the variances as
 * surf_svgf_variance returns them.  Needs no scene on the context and neither
 * reads nor changes its stored state. */
int surf_svgf_image(surf_ctx* ctx, uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev,
                    const surf_temporal_params* params, const surf_svgf_params* svgf, float* out_rgba, float* out_history,
                    float* out_moments, float* out_variance);
/* The CPU twin: the same per-pixel functions compiled for the host; needs no
 * device.  Bit-identical to surf_svgf_image. */
int surf_svgf_image_host(uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev,
                         const surf_temporal_params* params, const surf_svgf_params* svgf, float* out_rgba, float* out_history,
                         float* out_moments, float* out_variance);
/* Diagnostics: device time (HIP events) of the kernels of the last svgf run on
 * this context: [0] k_temporal, [1] the guides and the variance estimate,
 * [2 + i] iteration i; entries past the run's iterations (and past 8) are 0. */
int surf_debug_svgf_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);

/* ---- variance-guided filter, extensions: firefly clamp and filtered-history feedback ----
 * Two optional stages of the filter above, both off by default: with ext NULL
 * or all zero every _ex call below IS its namesake without _ex, bit for bit --
 * the image, the history, the moments, the variances and the stored state.
 * The arithmetic is part of the interface, as above (f32, uncontracted, IEEE
 * /, in exactly this order).
 *
 * Stage 0, the firefly clamp, runs when firefly_scale > 0, before step A.  At
 * 1 sample per pixel a few pixels per thousand carry a sample tens to
 * thousands of times their converged value; one sets a huge variance, so a
 * wide filter around it, and stays in the history for max_history frames.
 * For every pixel p of the full frame, with valid, inv, c and den the
 * denoiser's Prepare with this call's demodulate:
 *   l = lum(c / den), the quotients first.
 *   From mx = 0, cnt = 0 the 8 neighbours q = (x + dx, y + dy), dy = -1..1 the
 *   outer loop, dx = -1..1 the inner, the centre skipped; a q that is inside
 *   the frame, valid and has A(q).w > 0 is used:
 *     cnt = cnt + 1     mx = l_q > mx ? l_q : mx
 *   lim = firefly_scale * mx
 *   p valid, A.w > 0, cnt > 0 and l > lim:  f = lim / l,  c'_k = c_k * f
 *   otherwise:                              c' = c      (a NaN l fails the comparison and stays)
 *   A'(p) = A.w > 0 ? (c', 1) : (0, 0, 0, 0)
 * Steps A - C then read A' wherever they read A (c' * (1.0f / 1.0f) is exact).
 * Known bias: the clamp removes energy -- MEASUREMENTS "Firefly clamp and
 * feedback" gives the fraction -- and a lone lit pixel among black usable
 * neighbours (mx = 0) is clamped to black.
 *
 * Feedback, when feedback == 1: after iteration 0 of step C the stored and
 * returned history of a valid pixel becomes (I_1.rgb * den, n'), n' unchanged;
 * an invalid pixel keeps (r, n').  Moments, variances and the returned image
 * are defined exactly as above; their values change from the second frame on
 * only because the history did.  surf_temporal_history returns the fed-back
 * history.
 *
 * Launches: k_firefly, one launch of 256 threads per 32 x 8 tile before
 * k_temporal -- every thread loads its pixel's accumulator and albedo and
 * puts l (or a sentinel for "not usable") in a 34 x 10 tile of floats in LDS,
 * 1 360 bytes, the first 84 threads also one texel each of the halo of 1,
 * and the 8 taps come from there; 48 bytes of memory traffic per pixel, one
 * variant, no knob.  Feedback launches nothing more: iteration 0 runs an
 * instantiation of its kernel that also stores the history. */
typedef struct {
    float    firefly_scale;   /* 0: off; else finite and >= 1 */
    uint32_t feedback;        /* 0 / 1 */
    uint32_t _pad[2];
} surf_svgf_ext;
/* all zero: the filter as it is without extensions */
int surf_svgf_default_ext(surf_svgf_ext* ext);
/* surf_svgf_accumulate, _copy_device, _image and _image_host with the
 * extensions; ext may be NULL.  Status codes as theirs; SURF_ERR_INVALID also
 * for a firefly_scale that is neither 0 nor finite and >= 1, and for feedback
 * > 1.  The stored temporal state is the one surf_temporal_accumulate and
 * surf_svgf_accumulate share, and the three calls may be mixed: whichever
 * runs next reads the history the last one stored, filtered or not. */
int surf_svgf_accumulate_ex(surf_ctx* ctx, const surf_temporal_params* params, const surf_svgf_params* svgf, const surf_svgf_ext* ext,
                            float* out_rgba);
int surf_svgf_copy_device_ex(surf_ctx* ctx, const surf_temporal_params* params, const surf_svgf_params* svgf, const surf_svgf_ext* ext,
                             void* dst_device);
int surf_svgf_image_ex(surf_ctx* ctx, uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev,
                       const surf_temporal_params* params, const surf_svgf_params* svgf, const surf_svgf_ext* ext, float* out_rgba,
                       float* out_history, float* out_moments, float* out_variance);
int surf_svgf_image_host_ex(uint32_t w, uint32_t h, const surf_svgf_frame* cur, const surf_svgf_prev* prev,
                            const surf_temporal_params* params, const surf_svgf_params* svgf, const surf_svgf_ext* ext, float* out_rgba,
                            float* out_history, float* out_moments, float* out_variance);
/* The clamp alone on host planes of a full frame (w*h*4 floats each): out_acc
 * = A' as stage 0 defines it, e.g. to put in front of surf_denoise_image,
 * whose fixed-sigma filter has the same hole.  Needs no scene on the context.
 * SURF_ERR_INVALID for a NULL argument, w or h of 0, and a scale that is not
 * finite and >= 1 (0 included: there is nothing to switch off here). */
int surf_firefly_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* acc, const float* albedo, uint32_t demodulate, float scale,
                       float* out_acc);
/* The CPU twin: the same per-pixel function compiled for the host.  Bit-identical to surf_firefly_image. */
int surf_firefly_image_host(uint32_t w, uint32_t h, const float* acc, const float* albedo, uint32_t demodulate, float scale, float* out_acc);
/* Diagnostics: device time (HIP events) of the last k_firefly launch on this context, 0 before the first. */
int surf_debug_firefly_time(surf_ctx* ctx, float* kernel_ms);

/* ---- per-sample second moments, the sample-variance-guided filter, the noise estimate ----
 * For stills of many samples per pixel (from about 16; below that the
 * filters above are the better ones, INTEGRATION 9 has the measured table).
 * Everything here is opt-in: until surf_set_sample_squares switches it on,
 * no kernel, no result bit and no allocation differs.  The arithmetic is part
 * of the interface, as above (f32, uncontracted, / and sqrtf IEEE, in exactly
 * this order); lum is the variance-guided filter's.  No reference counterpart.
 *
 * The squares plane: rows*width float4 records in shard order, like the
 * accumulator.  With the plane on, the kernel that adds each pass's radiance
 * r -- one sample per pixel, whatever samples_per_frame is, so the moments
 * are per sample for multi-sample frames too -- to the accumulator also adds,
 * in pass order:
 *   Q.x = Q.x + r.x*r.x    Q.y = Q.y + r.y*r.y    Q.z = Q.z + r.z*r.z
 *   l   = (0.2126f*r.x + 0.7152f*r.y) + 0.0722f*r.z
 *   Q.w = Q.w + l*l
 * The accumulator, the sample stream and the event counters are bit for bit
 * what they are with the plane off.  surf_clear_accumulator zeroes the plane
 * with the accumulator; surf_destroy frees it.  Pointwise, so row shards work
 * as they are and assemble like accumulators; gathering the plane through
 * libsurf_mgpu.so is not provided.
 *
 * The sample-variance-guided filter.  Inputs: full-frame planes A (the
 * accumulator, n = A.w), Q (the squares), position, normal and albedo as
 * surf_read_aov defines them.  Parameters: surf_svgf_params, checked as for
 * surf_svgf_accumulate except that spatial_below is ignored.  Level 0, per
 * pixel, with valid, inv, c and den the denoiser's Prepare with this call's
 * demodulate:
 *   !valid or !(n >= 2.0f):   v = 0
 *   else, k = x, y, z:  m_k = Q_k * inv;  t_k = m_k - c_k*c_k;  t_k = t_k > 0 ? t_k : 0   (a NaN becomes 0)
 *                       s_k = sqrtf(t_k) / den_k
 *         sd = (0.2126f*s_x + 0.7152f*s_y) + 0.0722f*s_z
 *         v  = (sd*sd) / (n - 1.0f)
 *   I0 = (c / den, v)
 * -- the unbiased sample variance of the pixel mean, the channels' deviations
 * taken as fully correlated.  Then step C of the variance-guided filter runs
 * unchanged, with its output rule and its variance image (x = I0.w, y = I_n.w,
 * 0 for an invalid pixel, z = w = 0).  The variance falls as 1/n, so the
 * filter narrows as the render converges.  A frame with n < 2 everywhere is
 * valid: v = 0 everywhere, the colour term then rejects every tap whose
 * luminance differs (kl = 1 / variance_eps) and the filter all but returns
 * its input.
 * Launches: the packed guides, one level-0 kernel (256 threads per 32 x 8
 * tile; three 16-byte loads, a 16-byte and a 4-byte store per pixel), then the
 * variance-guided filter's own iteration kernels under SURF_DENOISE_LDS.
 *
 * The noise estimate: the relative standard error of a pixel's mean
 * luminance, from A and Q alone.  Parameters threshold and floor, both finite
 * and > 0.  Per pixel:
 *   n = A.w;  !(n >= 2.0f):  e = 1e30f
 *   else inv = 1.0f/n;  lb = lum(A.rgb*inv);  t = Q.w*inv - lb*lb;  t = t > 0 ? t : 0
 *        e = sqrtf(t / (n - 1.0f)) / (lb + floor)
 * The summary: pixels, the pixels looked at; above, those with !(e <=
 * threshold) (a NaN counts); max_error, the largest e, starting from 0 -- a NaN
 * or a negative e (a negative mean luminance) leaves it alone.  One kernel
 * writes the image where one is asked for and reduces the summary: per wave a
 * ballot and popcount and six lane shuffles, then one integer add and one
 * unsigned max on the float's bits -- exact, whatever order the waves arrive in. */
/* Switches the squares plane on (enabled != 0) or off.  Drains the stream.
 * SURF_ERR_INVALID unless the accumulator is empty -- no sample since
 * surf_create* or the last surf_clear_accumulator: the moments of samples
 * already absorbed cannot be recovered; SURF_ERR_OOM when the plane cannot be
 * allocated.  Switching off keeps the allocation. */
int surf_set_sample_squares(surf_ctx* ctx, int enabled);
/* The plane, to a host buffer of rows*width*4 floats / a buffer on the
 * context's device (rows*width*16 bytes).  Drain the stream, as every read
 * does; SURF_ERR_INVALID while the plane is off. */
int surf_read_sample_squares(surf_ctx* ctx, float* out);
int surf_copy_sample_squares_device(surf_ctx* ctx, void* dst_device);
/* The context's accumulator and squares filtered with its own (cached)
 * feature planes, as surf_denoise; status codes as surf_denoise's (on a row
 * shard surf_last_error points to surf_denoise_sampled_image), and
 * SURF_ERR_INVALID while the plane is off. */
int surf_denoise_sampled(surf_ctx* ctx, const surf_svgf_params* params, float* out_rgba);
int surf_denoise_sampled_copy_device(surf_ctx* ctx, const surf_svgf_params* params, void* dst_device);
/* Host planes of any full frame (w*h*4 floats each), e.g. one assembled from
 * row shards; two outputs of w*h*4 floats: the image and the variances.
 * Needs no scene on the context and no squares plane. */
int surf_denoise_sampled_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* acc, const float* squares, const float* position,
                               const float* normal, const float* albedo, const surf_svgf_params* params, float* out_rgba,
                               float* out_variance);
/* The CPU twin: the same per-pixel functions compiled for the host; needs no
 * device.  Bit-identical to surf_denoise_sampled_image. */
int surf_denoise_sampled_image_host(uint32_t w, uint32_t h, const float* acc, const float* squares, const float* position,
                                    const float* normal, const float* albedo, const surf_svgf_params* params, float* out_rgba,
                                    float* out_variance);
/* Diagnostics: device time (HIP events) of the last sampled run on this
 * context: kernel_ms[0] the level-0 kernel (the guide packing in front of it is
 * not counted), kernel_ms[1 + i] iteration i; entries past the run's iterations
 * (and past 7) are 0. */
int surf_debug_sampled_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);
typedef struct {
    float threshold;
    float floor;
} surf_noise_params;
typedef struct {
    uint64_t pixels, above;
    float max_error;
    uint32_t _pad;
} surf_noise_summary;
/* threshold 0.05, floor 0.01 */
int surf_noise_default_params(surf_noise_params* params);
/* The estimate of the context's own rows: out_error (rows*width floats) may be
 * NULL.  Works per shard: counts add across shards, the frame's max_error is
 * the largest of the shards'.  Drains the stream; SURF_ERR_INVALID for a NULL
 * context, params or summary, a threshold or floor that is not finite and > 0,
 * and while the plane is off; SURF_ERR_OOM when a scratch image cannot be
 * allocated. */
int surf_noise_estimate(surf_ctx* ctx, const surf_noise_params* params, float* out_error, surf_noise_summary* summary);
/* Host planes of npx pixels (npx*4 floats each), npx in 1..2^31; out_error
 * (npx floats) may be NULL.  Needs no scene and no squares plane. */
int surf_noise_image(surf_ctx* ctx, uint32_t npx, const float* acc, const float* squares, const surf_noise_params* params,
                     float* out_error, surf_noise_summary* summary);
/* The CPU twin; needs no device.  Bit-identical to surf_noise_image. */
int surf_noise_image_host(uint32_t npx, const float* acc, const float* squares, const surf_noise_params* params, float* out_error,
                          surf_noise_summary* summary);

/* ---- sample buckets and the robust (median-of-means) estimate (no reference counterpart) ----
 * For stills whose pixels have heavy-tailed sample distributions (caustics,
 * paths that survive Russian roulette with probability 1): there the plain
 * mean stops converging, and every filter and estimate above works from it.
 * Everything here is opt-in: until surf_set_sample_buckets switches it on, no
 * kernel, no launch, no allocation and no result bit differs.  The arithmetic
 * is part of the interface (f32, uncontracted, / IEEE, in exactly this order);
 * lum is the variance-guided filter's.
 *
 * The bucket planes: M planes (M = 2, 4, 8 or 16), bucket-major, each
 * rows*width float4 records in shard order like the accumulator: 16 M bytes
 * per pixel.  With the planes on, the kernel that adds a pass's radiance r --
 * one sample per pixel, whatever samples_per_frame is -- to pixel p's
 * accumulator record A takes, before that add,
 *   s = (uint32_t)A.w;   j = s & (M - 1)
 * and adds, plain f32 adds in pass order, to p's record of plane j:
 *   B_j.x = B_j.x + r.x    B_j.y = B_j.y + r.y    B_j.z = B_j.z + r.z    B_j.w = B_j.w + 1.0f
 * The bucket follows the pixel's own sample count, not the stream's pass
 * number: the buckets stay balanced (counts differ by at most one) under a
 * pixel mask, under the adaptive loop and across surf_render calls.  A.w is
 * exact up to 2^24 samples.  The buckets with B_j.w > 0 partition the pixel's
 * samples.  The accumulator, the squares plane, the sample stream, surf_stats
 * and the event counters are bit for bit what they are with buckets off.
 * surf_clear_accumulator zeroes the planes; surf_destroy frees them; a masked
 * stream leaves an inactive pixel's bucket records untouched.  Pointwise, so
 * row shards work as they are and the planes assemble like accumulators, plane
 * by plane; gathering them through libsurf_mgpu.so is not provided.
 * The sums of the even and of the odd planes are two half images of
 * independent samples: what a dual-buffer error estimate of a filtered picture
 * needs.
 * Cost: while a pixel's passes arrive one at a time each is a read-modify-write
 * of one bucket record (32 B beside the pass's 16 B of radiance); from a
 * sample count that is a multiple of M, with M or more passes at hand, the M
 * records are kept in registers for as many whole groups of M passes as there
 * are and written once (32 M bytes a launch).  MEASUREMENTS "Sample buckets".
 *
 * The robust estimate.  Inputs: A, the M bucket records B_0 .. B_{M-1} of the
 * pixel, trim_scale (finite and >= 0, default 1).  Per pixel; every sum starts
 * from 0.0f and adds in the order given:
 *   1. n_j = B_j.w; some n_j not > 0:                          out = A
 *   2. m_j = (B_j.x / n_j, B_j.y / n_j, B_j.z / n_j);  l_j = lum(m_j)
 *      some l_j not finite:                                    out = A
 *   3. order the buckets ascending by (l_j, j): a precedes b iff
 *      l_a < l_b || (l_a == l_b && a < b); call them (1) .. (M)
 *   4. T  = sum over i = 1 .. M of l_(i)
 *      Gn = sum over i = 1 .. M of (float)(2i - M - 1) * l_(i)
 *      !(T > 0):                                               out = A
 *   5. G = Gn / ((float)M * T)            -- the Gini coefficient of the bucket luminances
 *      f = floorf((G * trim_scale) * ((float)M * 0.5f))
 *      c = !(f >= 1) ? 0 : f >= (M-1)/2 ? (M-1)/2 : (uint32_t)f   (a NaN gives 0)
 *   6. c == 0:                                                 out = A, bit for bit
 *   7. e_k = (sum over i = c+1 .. M-c of m_(i).k) / (float)(M - 2c),  k = x, y, z
 *      out = (e.x * A.w, e.y * A.w, e.z * A.w, A.w)
 *   8. trim image byte = c (0 wherever out = A); summary: pixels, the pixels
 *      looked at; trimmed, those with c > 0
 * The output is an accumulator plane -- the mean is out.rgb / out.w -- so it
 * goes straight into surf_denoise_image, surf_denoise_sampled_image,
 * surf_firefly_image and surf_pack_rgba8_weighted.  With M = 2 the cap is 0
 * and the estimate is the accumulator: two buckets only give the half images.
 * The estimate is biased low by design: it removes energy.  On the bundled
 * scene at 256 samples per pixel, M = 8, the image mean falls by about 0.0025
 * (radiance units) against the plain mean; MEASUREMENTS "Robust estimate" has
 * the errors.  It wants about 32 samples per bucket: at 64 samples and M = 8
 * three quarters of the pixels are trimmed by plain noise and nothing is
 * gained, at 256 samples one pixel in nine is.
 * One kernel, one thread per pixel in blocks of 256: M + 1 16-byte loads, one
 * 16-byte store and one byte per pixel; the buckets are ordered by counting
 * ranks (M^2 compares) and taken by rank, nothing is indexed at run time; the
 * trimmed pixels are counted by a ballot and popcount per wave and one integer
 * add -- exact, whatever order the waves arrive in. */
/* M planes on (M = 2, 4, 8, 16) or off (M = 0).  Drains the stream.
 * SURF_ERR_INVALID for any other M, and unless the accumulator is empty -- no
 * sample since surf_create* or the last surf_clear_accumulator: the buckets of
 * samples already absorbed cannot be recovered; SURF_ERR_OOM when the planes
 * cannot be allocated.  Switching off or to a smaller M keeps the allocation. */
int surf_set_sample_buckets(surf_ctx* ctx, uint32_t M);
int surf_get_sample_buckets(const surf_ctx* ctx, uint32_t* M);
/* The M planes, bucket-major, to a host buffer of M*rows*width*4 floats / a
 * buffer on the context's device (M*rows*width*16 bytes).  Drain the stream,
 * as every read does; SURF_ERR_INVALID while the buckets are off. */
int surf_read_sample_buckets(surf_ctx* ctx, float* out);
int surf_copy_sample_buckets_device(surf_ctx* ctx, void* dst_device);
typedef struct {
    float trim_scale;
    uint32_t _pad;
} surf_robust_params;
typedef struct {
    uint64_t pixels, trimmed;
} surf_robust_summary;
/* trim_scale 1.0 */
int surf_robust_default_params(surf_robust_params* params);
/* The estimate of the context's own rows from its accumulator and buckets:
 * out_acc rows*width*4 floats; out_trim (rows*width bytes) and summary may be
 * NULL.  Works per shard: the counts add across shards.  Drains the stream;
 * SURF_ERR_INVALID for a NULL context, params or out_acc, a trim_scale that is
 * not finite and >= 0, and while the buckets are off; SURF_ERR_OOM when a
 * scratch image cannot be allocated. */
int surf_robust_accumulator(surf_ctx* ctx, const surf_robust_params* params, float* out_acc, uint8_t* out_trim,
                            surf_robust_summary* summary);
/* ... the output plane to a buffer on the context's device (rows*width*16 bytes) */
int surf_robust_copy_device(surf_ctx* ctx, const surf_robust_params* params, void* dst_acc_device);
/* Host planes of npx pixels, npx in 1..2^27: acc npx*4 floats, buckets
 * M*npx*4 floats bucket-major, e.g. assembled from row shards; M = 2, 4, 8 or
 * 16.  Needs no scene and no buckets on the context. */
int surf_robust_image(surf_ctx* ctx, uint32_t npx, uint32_t M, const float* acc, const float* buckets,
                      const surf_robust_params* params, float* out_acc, uint8_t* out_trim, surf_robust_summary* summary);
/* The CPU twin; needs no device.  Bit-identical to surf_robust_image. */
int surf_robust_image_host(uint32_t npx, uint32_t M, const float* acc, const float* buckets,
                           const surf_robust_params* params, float* out_acc, uint8_t* out_trim, surf_robust_summary* summary);
/* Diagnostics: device time (HIP events) of the last k_robust launch on this context. */
int surf_debug_robust_time(surf_ctx* ctx, float* kernel_ms);

/* ---- dual-buffer non-local means for stills, fed by the sample buckets (no reference counterpart) ----
 * The even and the odd buckets sum to two independent half images of the same
 * picture.  Each half is filtered by non-local means whose patch weights are
 * taken from the OTHER half (Rousselle, Knaus, Zwicker 2012): weights and
 * values are independent, no feature plane is read, so the filter also works
 * behind the lens blur, in mirrors and through glass, where the a-trous
 * filters have no guide edges.  The two filtered halves' difference is a
 * per-pixel estimate of the output's error.  Opt-in and a pure post-process:
 * without a call to these entry points no kernel, launch, allocation or result
 * bit differs; the calls leave the accumulator, the buckets, the squares,
 * surf_stats and the counters untouched.
 *
 * The arithmetic (part of the interface: f32, uncontracted, / is IEEE, expf is
 * glibc's; surf_denoise_nlm_image_host reproduces every bit).  Inputs: a full
 * frame of W x H pixels, two planes H0, H1 of half accumulators (rgb sums,
 * w = the half's sample count).  Parameters: search_radius r in 1..10,
 * patch_radius f in 0..3, k finite and > 0, alpha finite and >= 0, eps finite
 * and > 0.  Host constants: kk = k*k, cnt = (float)(3*(2f+1)*(2f+1)).
 * clampF(x, y) clamps each coordinate to the frame.
 *
 * Prepare, per pixel p:  n0 = H0.w, n1 = H1.w;  ok = n0 > 0 && n1 > 0;  when
 *   ok, c0_k = H0_k / n0 and c1_k = H1_k / n1;  valid = ok && all six
 *   quotients finite;  an invalid pixel has c0 = c1 = (0, 0, 0).
 *   v_k = 0.5f * ((c0_k - c1_k) * (c0_k - c1_k));  V(p)_k = the sum from 0.0f
 *   of v_k over the nine texels clampF(x + dx, y + dy), dy = -1..1 outer and
 *   dx = -1..1 inner, divided by 9.0f.
 * Distance image of a search offset o = (dx, dy), at any unclamped texel s'
 *   (up to f outside the frame):  a = clampF(s'), b = clampF(s' + o), g the
 *   half the weights come from;  for k = x, y, z:
 *     d  = Cg(a)_k - Cg(b)_k
 *     vm = V(b)_k < V(a)_k ? V(b)_k : V(a)_k
 *     num = d*d - alpha*(V(a)_k + vm)
 *     den = eps + kk*(V(a)_k + V(b)_k)
 *     d_k = num / den
 *   d_o(s') = (d_x + d_y) + d_z.
 * Patch distance of p and o:  for j = -f..f, R_j = the sum from 0.0f over
 *   i = -f..f of d_o(p + (i, j));  S = the sum from 0.0f over j = -f..f of R_j;
 *   D = S / cnt.  (Rows first, then the column of row sums: a separable
 *   implementation on a tile is the definition.)
 * Filtering half h with weights from g = 1 - h, for a valid p:  sumW = 0,
 *   sum = 0;  the taps q = p + o, dy = -r..r outer and dx = -r..r inner;  a q
 *   outside the frame or invalid is skipped;  the centre tap has w = 1.0f;
 *   every other tap  e = D < 100.0f ? D : 100.0f  (a NaN becomes 100),
 *   e = e > 0.0f ? e : 0.0f,  w = expf(-e);  sumW = sumW + w,
 *   sum_k = sum_k + w * Ch(q)_k;  o_h(p) = sum / sumW.
 * Output, valid p:  out_k = ((o0_k*n0) + (o1_k*n1)) / (n0 + n1), out.w = 1;
 *   err_k = 0.25f * ((o0_k - o1_k)*(o0_k - o1_k)), err.w = 0.
 *   Invalid p, n = n0 + n1, inv = n > 0 ? 1.0f/n : 0.0f:
 *   out = ((H0.rgb + H1.rgb) * inv, 1), err = 0.
 * The halves from the buckets (context form): half 0 is the sum from 0.0f of
 *   the even planes j = 0, 2, ... in ascending order, half 1 the same over the
 *   odd planes.
 *
 * Three launches: the halves (context form), prepare (c0 + validity, c1 and V
 * packed into three 16-byte records per pixel), the filter -- both halves in
 * one launch on 32 x 8 pixel tiles.  The filter stages the tile with its halo
 * of r + f in LDS (40 bytes a texel) and computes each offset's distance image
 * once per texel of the tile and its halo of f; where that layout exceeds
 * 64 KiB (from r + f = 11) or under SURF_NLM_LDS=0 (read at surf_create*)
 * every value comes from global memory.
 * Identical bits either way.  MEASUREMENTS "Non-local means" has the errors
 * and the costs. */
typedef struct {
    uint32_t search_radius, patch_radius;
    float k, alpha, eps;
    uint32_t _pad;
} surf_nlm_params;
/* r 5, f 2, k 0.45, alpha 1.0, eps 1e-10 */
int surf_nlm_default_params(surf_nlm_params* params);
/* The context form: the halves of the context's own buckets, filtered;
 * out_rgba and out_err (may be NULL) height*width*4 floats.  Drains the
 * stream.  SURF_ERR_INVALID for a NULL context, params or out_rgba, parameters
 * outside the ranges above, while the buckets are off (surf_set_sample_buckets),
 * and on a row shard -- a patch reads its neighbours' rows: assemble the
 * shards' buckets and call surf_denoise_nlm_image; SURF_ERR_OOM when a scratch
 * image cannot be allocated. */
int surf_denoise_nlm(surf_ctx* ctx, const surf_nlm_params* params, float* out_rgba, float* out_err);
/* ... the two images to buffers on the context's device (height*width*16 bytes each; dst_err_device may be NULL) */
int surf_denoise_nlm_copy_device(surf_ctx* ctx, const surf_nlm_params* params, void* dst_rgba_device, void* dst_err_device);
/* Host planes of a w x h frame (w*h in 1..2^27), w*h*4 floats each.  Needs no
 * scene and no buckets on the context. */
int surf_denoise_nlm_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* half0, const float* half1,
                           const surf_nlm_params* params, float* out_rgba, float* out_err);
/* The CPU twin; needs no device.  Bit-identical to surf_denoise_nlm_image. */
int surf_denoise_nlm_image_host(uint32_t w, uint32_t h, const float* half0, const float* half1, const surf_nlm_params* params,
                                float* out_rgba, float* out_err);
/* Diagnostics: device times (HIP events) of the last run's halves, prepare and
 * filter launches into kernel_ms[0..count); the image form has no halves launch. */
int surf_debug_nlm_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);

/* ---- first-order feature regression on the half images (no reference counterpart) ----
 * The filter that joins the two half images of the sample buckets with the
 * noise-free feature planes: around every pixel each half's colour is fitted,
 * by weighted least squares, as a first-order function of the features
 * (normal, albedo, relative depth) with the non-local-means filter's
 * cross-half patch weights, and the fit is evaluated at the pixel itself
 * (Moon, Carr, Yoon 2014; Bitterli et al. 2016 without the collaborative
 * step).  Where the features explain the picture the fit follows them across
 * the window instead of averaging over them; where they do not (a miss, a
 * singular system) it is the non-local-means average.  Opt-in and a pure
 * post-process, as surf_denoise_nlm is: without a call nothing differs, and a
 * call leaves the accumulator, the buckets, the squares, surf_stats, the
 * counters and the cached feature planes as they are.
 *
 * The arithmetic (part of the interface: f32, uncontracted, / is IEEE, expf is
 * glibc's; surf_denoise_regress_image_host reproduces every bit).  Inputs: a
 * full frame of W x H pixels, the half accumulators H0, H1 as above, and the
 * three planes position, normal, albedo as surf_read_aov defines them.
 * Parameters: search_radius r, patch_radius f, k, alpha, eps as in
 * surf_nlm_params, and ridge finite and > 0.
 *
 * Prepare, the distance images and the patch distances D_0(p, o), D_1(p, o)
 *   are surf_denoise_nlm's, word for word; so is the weight
 *   w(D) = expf(-max(min(D, 100), 0)) (a NaN becomes 100).
 * Feature record of a pixel:  N = normal.xyz, a = albedo.xyz, z = position.w,
 *   hit = albedo.w != 0.
 * Features of a tap q against the centre p:  phi_0..2 = N(q) - N(p);
 *   phi_3..5 = a(q) - a(p);  phi_6 = (z(q) - z(p)) / z(p);  phi_7 = 1.0f (the
 *   constant goes last: its unknown is the prediction at p and needs no back
 *   substitution).
 * A pixel p that is invalid in surf_denoise_nlm's sense has that filter's
 *   invalid output.  For a valid p, per half h with g = 1 - h, the sums start
 *   at 0.0f and the taps q = p + o are taken dy = -r..r outer, dx = -r..r
 *   inner.  The centre tap has w = 1.0f, every other tap w = w(D_g(p, o)).
 *   p a miss:  every q inside the frame and valid is taken, at order zero:
 *     A_77 = A_77 + w;  b_7c = b_7c + w * Ch(q)_c  -- surf_denoise_nlm's sums.
 *   p a hit:  q is taken when it is inside the frame, valid, a hit itself and
 *     phi_0..6 are all finite (x - x == 0.0f).  pp_ij = phi_i * phi_j,
 *     A_ij = A_ij + w * pp_ij for i <= j;  u_i = w * phi_i,
 *     b_ic = b_ic + u_i * Ch(q)_c for the channels c = x, y, z.
 *     (A hit p whose own record is not finite -- z(p) = 0, say -- rejects every
 *     tap, its own included: 0 / 0, a NaN in, a NaN out.)
 * Solve, p a hit, per half:  sw = A_77;  zero_c = b_7c / sw;
 *   A_jj = A_jj + ridge * sw for j = 0..6.  For k = 0..6 in turn:  d_k = A_kk;
 *   for i = k+1..7:  l = A_ki / d_k;  A_ij = A_ij - l * A_kj for j = i..7;
 *   b_ic = b_ic - l * b_kc.  Then d_7 = A_77, beta_c = b_7c / d_7.  When every
 *   d_0..7 is finite and > 0 and the three beta_c are finite, o_h = beta, else
 *   o_h = zero.  p a miss:  o_h = zero.
 * Output, valid p:  surf_denoise_nlm's, from o_0 and o_1:
 *   out_k = ((o0_k*n0) + (o1_k*n1)) / (n0 + n1), out.w = 1;
 *   err_k = 0.25f * ((o0_k - o1_k)*(o0_k - o1_k)), err.w = 0.
 * On a frame whose pixels are all hits with the same feature record every
 * phi_0..6 and every l is 0: the result is surf_denoise_nlm_image's at the same
 * r, f, k, alpha, eps, bit for bit.
 *
 * Three launches: the halves (context form) and prepare are the
 * non-local-means filter's kernels; the filter handles both halves in one
 * launch on 32 x 8 pixel tiles, a pixel's 2 x (36 + 24) sums in registers,
 * at most two waves a SIMD.  It stages what the non-local-means kernel
 * stages and the feature records of the tile with its halo of r (32 bytes a
 * texel) in LDS: 68,128 B at the defaults, two workgroups a compute unit up
 * to 80 KiB, one from (6, 3) on, 129,728 B at (10, 3) -- every r and f in
 * range fits the 160 KiB of a compute unit.  Past that bound, or under
 * SURF_REGRESS_LDS=0 (read at surf_create*), every value comes from global
 * memory.  Identical bits either way.  MEASUREMENTS "First-order regression"
 * has the errors and the costs. */
typedef struct {
    uint32_t search_radius, patch_radius;
    float k, alpha, eps, ridge;
} surf_regress_params;
/* r 5, f 2, k 0.7, alpha 1.0, eps 1e-10, ridge 0.1 */
int surf_regress_default_params(surf_regress_params* params);
/* The context form: the halves of the context's own buckets and the planes
 * surf_set_filter_guides selects (first hit or chain, computed if need be, as
 * surf_denoise reads them); out_rgba and out_err (may be NULL) height*width*4
 * floats.  Drains the stream.  SURF_ERR_INVALID for a NULL context, params or
 * out_rgba, parameters outside the ranges above, while the buckets are off
 * (surf_set_sample_buckets), and on a row shard: assemble the shards' buckets
 * and planes and call surf_denoise_regress_image; SURF_ERR_OOM when a scratch
 * image cannot be allocated. */
int surf_denoise_regress(surf_ctx* ctx, const surf_regress_params* params, float* out_rgba, float* out_err);
/* ... the two images to buffers on the context's device (height*width*16 bytes each; dst_err_device may be NULL) */
int surf_denoise_regress_copy_device(surf_ctx* ctx, const surf_regress_params* params, void* dst_rgba_device, void* dst_err_device);
/* Host planes of a w x h frame (w*h in 1..2^27), w*h*4 floats each.  Needs no
 * scene and no buckets on the context. */
int surf_denoise_regress_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* half0, const float* half1, const float* position,
                               const float* normal, const float* albedo, const surf_regress_params* params, float* out_rgba,
                               float* out_err);
/* The CPU twin; needs no device.  Bit-identical to surf_denoise_regress_image. */
int surf_denoise_regress_image_host(uint32_t w, uint32_t h, const float* half0, const float* half1, const float* position,
                                    const float* normal, const float* albedo, const surf_regress_params* params, float* out_rgba,
                                    float* out_err);
/* Diagnostics: device times (HIP events) of the last run's halves, prepare and
 * filter launches into kernel_ms[0..count); the image form has no halves launch. */
int surf_debug_regress_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);

/* ---- per-pixel sample masks and the adaptive loop (no reference counterpart) ----
 * A context carries an active-pixel mask: one byte per pixel of the shard in
 * shard order (rows*width), nonzero = active.  After surf_create* and after
 * surf_clear_accumulator every pixel is active.  With a mask set,
 * surf_render(frames, first_sample_index, max_segments, spp) issues only the
 * active pixels' chains; frame k is still seeded initSeed(p + 1799 *
 * (first_sample_index + k*spp)), so an active pixel receives exactly the
 * samples it would receive without a mask, bit for bit, and an inactive
 * pixel's accumulator and squares records stay untouched: its w does not
 * advance.  surf_stats.samples and the event counters count what was traced.
 * An all-ones mask is no mask (the same kernels, counters and issue order); an
 * all-zero mask makes surf_render return SURF_OK and change nothing.  Setting
 * a mask drains and ends the open stream, as a change of spp does.  Camera,
 * scene and instance updates keep the mask.
 * surf_finalize_rgba8, surf_display_rgba8 and surf_stats.energy keep dividing
 * by the context's frame count -- the frames requested of surf_render since the
 * last clear, whatever the mask was: under a mask that is no pixel's mean but a
 * stale pixel's.  surf_finalize_rgba8_weighted divides each pixel by its own w.
 * Device side: the mask is compacted to the ascending list of active local
 * pixels (4 B per pixel, allocated on first use beside the 1 B per pixel of
 * the mask); a masked stream issues frame-major over the list and accumulates
 * through it, sample ids and the radiance ring are those of the full shard.
 *
 * The mask from the noise estimate.  Parameters: threshold and floor finite
 * and > 0, min_samples >= 2, max_samples >= min_samples, dilate in 0..2.  With
 * e(p) the noise estimate's error of pixel p (above) at `floor`:
 *   raw(p)    = !(A.w >= (float)min_samples) || !(e(p) <= threshold)
 *               (a NaN counts as noisy; n < 2 gives e = 1e30)
 *   active(p) = (some q with |dx| <= dilate, |dy| <= dilate inside the frame has raw(q))
 *               && A(p).w < (float)max_samples
 *   mask byte = active ? 1 : 0;  list = the active pixels' indices y*w + x, ascending
 * The dilation exists because the estimate is itself noisy: a lone pixel that
 * stops early shows as a speckle.
 * Launches: the flags kernel, 256 threads per 32 x 8 tile -- the raw flags of
 * the tile and its halo of `dilate` go to LDS (up to 36 x 12 bytes; 32 B read
 * per texel), then one byte is written per pixel -- and an order-preserving
 * compaction of the byte mask: per 256-pixel block a count (ballot and
 * popcount per wave), one block that scans the block counts, and a scatter
 * that repeats the ballots and writes each active index at block offset + wave
 * offset + its rank in the wave.  No atomic: the list does not depend on the
 * order the blocks arrive in.  1 B in twice and 4 B out per active pixel. */
typedef struct {
    float threshold, floor;
    uint32_t min_samples, max_samples, dilate, _pad[3];
} surf_adaptive_mask_params;
/* mask: rows*width bytes, NULL = every pixel.  Drains and ends the stream.
 * SURF_ERR_INVALID for a NULL context, SURF_ERR_OOM when the mask's buffers
 * cannot be allocated. */
int surf_set_pixel_mask(surf_ctx* ctx, const uint8_t* mask);
/* out_mask (rows*width bytes of 0 / 1, may be NULL) and the active count
 * (rows*width without a mask).  Reads what is set; drains nothing. */
int surf_get_pixel_mask(surf_ctx* ctx, uint8_t* out_mask, uint32_t* active_count);
/* threshold 0.05, floor 0.01, min_samples 16, max_samples 1024, dilate 1 */
int surf_adaptive_default_mask_params(surf_adaptive_mask_params* params);
/* Builds the mask from the context's accumulator and squares and sets it; the
 * planes, the mask and the list stay on the device, the count comes back.
 * Drains and ends the stream.  SURF_ERR_INVALID for bad parameters, while the
 * squares plane is off, and on a row shard when dilate > 0 -- a dilation needs
 * its neighbours' rows (surf_last_error points to surf_adaptive_mask_image);
 * with dilate == 0 it works per shard. */
int surf_mask_from_noise(surf_ctx* ctx, const surf_adaptive_mask_params* params, uint32_t* active_count);
/* Host planes of any w x h frame (w*h*4 floats each), e.g. one assembled from
 * row shards.  mask_out: w*h bytes; list_out (w*h words, the first *count
 * written) may be NULL.  Needs no scene and no squares plane; leaves the
 * context's mask alone. */
int surf_adaptive_mask_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* acc, const float* squares,
                             const surf_adaptive_mask_params* params, uint8_t* mask_out, uint32_t* list_out, uint32_t* count);
/* The CPU twin; needs no device.  Bit-identical to surf_adaptive_mask_image. */
int surf_adaptive_mask_image_host(uint32_t w, uint32_t h, const float* acc, const float* squares,
                                  const surf_adaptive_mask_params* params, uint8_t* mask_out, uint32_t* list_out, uint32_t* count);

/* "Render until converged".  Needs the squares plane on and an empty
 * accumulator (SURF_ERR_INVALID otherwise, as surf_set_sample_squares); renders
 * 1-sample frames.  The definition, part of the interface:
 *   1. mask = every pixel
 *   2. render mask.min_samples frames from first_sample_index; f = min_samples
 *   3. repeat: build the mask from the estimate (surf_mask_from_noise);
 *              stop when no pixel is active or f == mask.max_samples;
 *              nb = min(batch, max_samples - f);
 *              render nb frames at first_sample_index + f under the mask; f += nb
 *   4. the final mask stays set
 * round_active[r] (the first min(rounds, round_cap) entries; may be NULL) is
 * the active count round r of step 3 rendered with.  Summary: rounds (renders
 * of step 3), frames = f, active_last (the final mask's count), samples (camera
 * samples traced, step 2 included), noise (surf_noise_estimate's summary of the
 * final state at mask.threshold and mask.floor).  batch >= 1 (default 64,
 * the fastest of 8, 16, 32 and 64 at 1280 x 720: a round's drain costs about
 * what 16 full frames do, MEASUREMENTS "Adaptive sampling").
 * Known limits: stopping on an estimate made from the same samples biases the
 * result slightly towards dark (pixels whose early samples happen to agree
 * stop early); min_samples and dilate are the mitigation.  Each round drains
 * the stream -- the drain is the long Russian-roulette tail -- so small batches
 * cost throughput. */
typedef struct {
    surf_adaptive_mask_params mask;
    uint32_t batch, max_segments, first_sample_index, _pad;
} surf_adaptive_params;
typedef struct {
    uint32_t rounds, frames, active_last, _pad;
    uint64_t samples;
    surf_noise_summary noise;
} surf_adaptive_summary;
/* the mask defaults, batch 64, max_segments 0, first_sample_index 0 */
int surf_adaptive_default_params(surf_adaptive_params* params);
int surf_render_adaptive(surf_ctx* ctx, const surf_adaptive_params* params, uint32_t* round_active, uint32_t round_cap,
                         surf_adaptive_summary* summary);

/* ---- the mask from the non-local-means filter's error estimate, and the loop around it (no reference counterpart) ----
 * surf_mask_from_noise asks whether the UNFILTERED pixel has converged.  Who
 * shows the non-local-means output wants another answer: the filter removes
 * noise cheaply in smooth regions and cannot at edges, in caustics and in fine
 * detail, and its second output, err, estimates per pixel how wrong the
 * FILTERED picture still is (Rousselle, Knaus, Zwicker 2012).  The entry points
 * below turn (out, err) into an active-pixel mask and run the adaptive loop on
 * it.  Opt-in: without a call to them no kernel, launch, allocation or result
 * bit differs.
 *
 * The mask.  Inputs, full-frame W x H planes of 16-byte records: out, the
 * filter's result; err, its error plane; A, the accumulator, read only for A.w.
 * Parameters (surf_error_mask_params): threshold finite and > 0 -- a relative
 * RMS error; floor finite and > 0; min_samples >= 2; max_samples >=
 * min_samples; smooth in 0..3; dilate in 0..2.  Host constants, f32:
 * tt = threshold*threshold, ff = floor*floor, cnt = (float)((2 smooth + 1)^2).
 * The arithmetic is part of the interface: f32, uncontracted, / IEEE, every
 * sum starting from 0.0f in the order given; surf_error_mask_image_host
 * reproduces every bit.  With o = out(p), e = err(p):
 *   num = (e.x + e.y) + e.z
 *   den = (((o.x*o.x) + (o.y*o.y)) + (o.z*o.z)) + ff
 *   rel(p) = num / den
 *   S(p): smooth == 0: rel(p).  Otherwise, clampF clamping each coordinate to
 *         the frame: for j = -smooth..smooth, R_j = the sum from 0.0f over
 *         i = -smooth..smooth of rel(clampF(p + (i, j))); S = (the sum from
 *         0.0f over j = -smooth..smooth of R_j) / cnt.  (Rows first, then the
 *         column of row sums, as the filter's V and patch distance.)
 *   raw(p)    = !(A.w >= (float)min_samples) || !(S(p) <= tt)     (a NaN counts as noisy)
 *   active(p), the mask byte and the ascending list: exactly surf_mask_from_noise's --
 *               (some q with |dx| <= dilate, |dy| <= dilate inside the frame has raw(q))
 *               && A(p).w < (float)max_samples
 * The estimate is one squared difference per pixel, so unsmoothed it is very
 * noisy: that is what `smooth` is for.  A pixel the filter marked invalid has
 * err = 0, so rel = 0 there: it is quiet unless it is below min_samples (its
 * neighbours' S still take its 0).
 * Launches: the mask kernel, 256 threads per 32 x 8 tile, takes rel of the
 * tile and its halo of smooth + dilate (at most 5: 42 x 18 texels, 32 B read
 * per texel) into LDS, then the row sums, then the column sums and the raw
 * flags of the tile and its halo of dilate, ORs them and writes one byte per
 * pixel: 6 KB of LDS, no scratch; then surf_mask_from_noise's order-preserving
 * compaction.  A pointwise pre-pass that wrote rel to a plane of its own (4 B
 * per pixel) for the mask kernel to stage from was measured and was slower at
 * 1280 x 720 and 1920 x 1080 (MEASUREMENTS "Error-driven adaptive sampling"). */
typedef struct {
    float threshold, floor;
    uint32_t min_samples, max_samples, smooth, dilate, _pad[2];
} surf_error_mask_params;
/* threshold 0.1, floor 0.01, min_samples 16, max_samples 1024, smooth 3, dilate 1 */
int surf_error_mask_default_params(surf_error_mask_params* params);
/* Host planes of any w x h frame (w*h*4 floats each), e.g. surf_denoise_nlm_image's
 * two outputs and an assembled accumulator.  mask_out: w*h bytes; list_out (w*h
 * words, the first *count written) may be NULL.  Needs no scene and no buckets;
 * leaves the context's mask alone.  SURF_ERR_INVALID for a NULL context, plane,
 * params, mask_out or count, an empty frame or one of more than 2^31 pixels, and
 * parameters outside the ranges above. */
int surf_error_mask_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* out_rgba, const float* err, const float* acc,
                          const surf_error_mask_params* params, uint8_t* mask_out, uint32_t* list_out, uint32_t* count);
/* The CPU twin; needs no device.  Bit-identical to surf_error_mask_image. */
int surf_error_mask_image_host(uint32_t w, uint32_t h, const float* out_rgba, const float* err, const float* acc,
                               const surf_error_mask_params* params, uint8_t* mask_out, uint32_t* list_out, uint32_t* count);
/* The context form: the halves of the context's buckets through the filter
 * (surf_denoise_nlm's launches), the mask from its out and err and the
 * context's accumulator, set as surf_mask_from_noise sets it; everything stays
 * on the device, the count comes back.  Drains and ends the stream.
 * SURF_ERR_INVALID for a NULL context, bad parameters of either kind, while the
 * buckets are off and on a row shard. */
int surf_mask_from_nlm(surf_ctx* ctx, const surf_nlm_params* nlm_params, const surf_error_mask_params* mask_params,
                       uint32_t* active_count);
/* Diagnostics: device times (HIP events) of the last mask's kernel and of its
 * compaction into kernel_ms[0..count). */
int surf_debug_error_mask_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);

/* "Render until the filtered picture has converged".  Needs the buckets on
 * (any M), an empty accumulator and a context that owns every row of the frame
 * (SURF_ERR_INVALID otherwise, surf_last_error names the cause); the squares
 * plane is not needed.  Renders 1-sample frames.  The definition, part of the
 * interface:
 *   1. mask = every pixel; render mask.min_samples frames from
 *      first_sample_index; f = min_samples
 *   2. repeat: filter the context's halves (nlm) and build the mask from its
 *              out and err (surf_mask_from_nlm);
 *              stop when no pixel is active or f == mask.max_samples;
 *              nb = min(batch, max_samples - f);
 *              render nb frames at first_sample_index + f under the mask; f += nb
 *   3. the final mask stays set
 * The filter run that ends the loop is of the final state, so the loop also
 * returns that out and err without another launch: out_rgba and out_err, each
 * height*width*4 floats, each may be NULL.  round_active[r] (the first
 * min(rounds, round_cap) entries; may be NULL) is the active count round r of
 * step 2 rendered with.  Between rounds nothing but the active count crosses
 * to the host.  Summary, of the final state: rounds (renders of step 2),
 * frames = f, active_last (the final mask's count), samples (camera samples
 * traced, step 1 included), above (the pixels with A.w >= min_samples and
 * !(S <= tt): what the cap or nothing stopped), max_error (the largest S that
 * is no NaN, 0 when there is none; counted by integer adds and an integer max
 * of an order-preserving key, so independent of the order blocks arrive in).
 * batch >= 1.
 * Known limits: stopping on an estimate made from the same samples biases the
 * result slightly; smooth, dilate and min_samples are the mitigation.  A
 * heavy-tailed pixel -- one whose halves keep disagreeing -- stays active until
 * max_samples.  Each round drains the stream and runs the filter, so small
 * batches cost throughput.  INTEGRATION 13 and MEASUREMENTS "Error-driven
 * adaptive sampling" say what the loop gains over uniform sampling. */
typedef struct {
    surf_error_mask_params mask;
    surf_nlm_params nlm;
    uint32_t batch, max_segments, first_sample_index, _pad;
} surf_adaptive_nlm_params;
typedef struct {
    uint32_t rounds, frames, active_last, _pad;
    uint64_t samples, above;
    float max_error;
    uint32_t _pad2;
} surf_adaptive_nlm_summary;
/* the mask defaults, surf_nlm_default_params, batch 64, max_segments 0, first_sample_index 0 */
int surf_adaptive_nlm_default_params(surf_adaptive_nlm_params* params);
int surf_render_adaptive_nlm(surf_ctx* ctx, const surf_adaptive_nlm_params* params, float* out_rgba, float* out_err,
                             uint32_t* round_active, uint32_t round_cap, surf_adaptive_nlm_summary* summary);
/* ... the two images to buffers on the context's device (height*width*16 bytes each; each may be NULL) */
int surf_render_adaptive_nlm_copy_device(surf_ctx* ctx, const surf_adaptive_nlm_params* params, void* dst_rgba_device,
                                         void* dst_err_device, uint32_t* round_active, uint32_t round_cap,
                                         surf_adaptive_nlm_summary* summary);

/* RGBA8 of the accumulator with each pixel divided by its own sample count:
 *   inv = A.w > 0 ? 1.0f/A.w : 0.0f;  channel k = packChannel((a_k*inv)*255.0f), alpha included
 * (packChannel: surf_finalize_rgba8's rounding and saturation), and with
 * display != 0 surf_display_rgba8's displayChannel on top of each.  Drains the
 * stream.  One pointwise kernel, 16 B in and 4 B out per pixel. */
int surf_finalize_rgba8_weighted(surf_ctx* ctx, int display, uint32_t* out_rgba8);
/* The CPU twin on n records of a host plane; needs no device.  Bit-identical. */
int surf_pack_rgba8_weighted(const float* acc, uint32_t n, int display, uint32_t* out_rgba8);

/* ---- the display stage: metered exposure, bloom, tone curve, transfer, dither (no reference counterpart) ----
 * The road from any float RGBA image of this library -- the accumulator, the
 * robust estimate, a filter's output -- to RGBA8 words for a viewer, beside
 * surf_finalize_rgba8 / surf_display_rgba8, which reproduce the reference's
 * clamp (and sqrt of the 8-bit value) and stay as they are.  Opt-in and a
 * pure post-process: without a call to these entry points no kernel, launch,
 * allocation or result bit differs; the calls leave the accumulator, the
 * buckets, the squares, surf_stats and the counters untouched.
 *
 * The arithmetic (part of the interface: f32, uncontracted, / and sqrtf are
 * IEEE, expf is glibc's and evaluated on the host only;
 * surf_display_image_host reproduces every bit).  Input: a frame of W x H
 * records (rgb sums, w = the pixel's weight: 1 for a filter's output, the
 * sample count for an accumulator).
 *
 * 1. Colour.  n = .w;  c_k = n > 0 ? rgb_k / n : 0;  then c_k = c_k > 0 ? c_k : 0
 *    (a NaN or a negative value becomes 0, +inf stays).
 * 2. Luminance.  L = (0.2126f*c_x + 0.7152f*c_y) + 0.0722f*c_z.
 * 3. Meter (always runs; in manual mode it only fills *meter).  b = bits(L) >> 20.
 *    b < 888 (L < 2^-16): the pixel counts in `black` and nowhere else.  Else
 *    bin = b - 888, capped at 255: 8 bins per octave over 2^-16 .. 2^16, +inf in
 *    bin 255; hist[bin] and `counted` count it.  median_bin m = the smallest bin
 *    with 2 * (hist[0] + .. + hist[m]) >= counted, in 64-bit integers (0 when
 *    counted = 0).  Lm = the float whose bits are ((m + 888) << 20) | 0x80000.
 *    Auto: scale = key / Lm, then scale = scale < min_scale ? min_scale : scale,
 *    then scale = scale > max_scale ? max_scale : scale; counted = 0: scale = 1.
 *    Manual: scale = exposure.
 * 4. Exposed colour.  e_k = c_k * scale.
 * 5. Bloom, bloom_radius R > 0.  Host constants: sigma = 0.5f*R;
 *    g_i = expf(-(float)(i*i) / (2.0f*sigma*sigma)), i = 0..R;  S = g_0, then
 *    S = S + (g_i + g_i) for i = 1..R;  wn_i = g_i / S.
 *    B_k = (e_k - bloom_threshold) > 0 ? e_k - bloom_threshold : 0.
 *    Hh(x, y)_k = the sum from 0.0f over i = -R..R ascending of
 *    wn_|i| * B(clamp(x + i), y)_k;  Vv(x, y)_k = the same sum over j of
 *    wn_|j| * Hh(x, clamp(y + j))_k (clamp: to the frame).
 *    x_k = e_k + bloom_strength * Vv_k.  R = 0: x_k = e_k, and no blur plane is
 *    allocated or launched.
 * 6. Curve.  0: t = x.  1 (extended Reinhard): t = (x*(1.0f + x/(white*white))) / (1.0f + x).
 *    2 (the ACES fit of Narkowicz): t = (x*(2.51f*x + 0.03f)) / (x*(2.43f*x + 0.59f) + 0.14f).
 *    v = t < 1.0f ? t : 1.0f (a NaN, from +inf, becomes 1);  v = v > 0 ? v : 0.
 * 7. Transfer.  0: u = v.  1: u = sqrtf(v).  2 (sRGB): i = (uint)(sqrtf(v)*4095.0f + 0.5f),
 *    u = T[i];  T[i] is computed in double and rounded to f32:  l = (i/4095)^2,
 *    T[i] = l <= 0.0031308 ? 12.92*l : 1.055*pow(l, 1/2.4) - 0.055
 *    (surf_display_srgb_table).  Indexed by the square root, the table's error
 *    stays below a tenth of an 8-bit code in the dark, steep part.
 * 8. Quantise.  d = dither ? ((float)B8[y & 7][x & 7] + 0.5f) / 64.0f : 0.5f;
 *    q = (uint)(u*255.0f + d), capped at 255;  alpha = 255;  the word is
 *    r | g << 8 | b << 16 | a << 24, as surf_finalize_rgba8 packs it.
 *    B8, the standard 8 x 8 Bayer matrix (surf_display_bayer8, row-major):
 *       0 32  8 40  2 34 10 42
 *      48 16 56 24 50 18 58 26
 *      12 44  4 36 14 46  6 38
 *      60 28 52 20 62 30 54 22
 *       3 35 11 43  1 33  9 41
 *      51 19 59 27 49 17 57 25
 *      15 47  7 39 13 45  5 37
 *      63 31 55 23 61 29 53 21
 *
 * Launches: the meter (a 256-bin histogram per block in LDS with integer LDS
 * atomics, then one integer global atomic per non-empty bin per block, into
 * one of 16 copies of the record so that the blocks do not all wait on the
 * same addresses: the result does not depend on the order of arrival), the
 * scale (one wave sums the copies, scans the bins and writes the meter record
 * to device memory, where the following kernels read scale: no host
 * synchronisation between meter and pack; the sRGB table is in constant
 * memory), and
 * either the fused pack (rules 1, 4, 6-8) or, with bloom, the horizontal pass
 * and the vertical pass fused with the pack, on 32 x 8 pixel tiles staged in
 * LDS with their halo of R.  Exposure adaptation over time is left to the
 * caller: meter->scale is returned for it.  MEASUREMENTS "Display stage" has
 * the costs. */
typedef struct {
    uint32_t exposure_mode;       /* 0 manual, 1 auto */
    float exposure;               /* the manual linear scale; finite and > 0 */
    float key, min_scale, max_scale;   /* finite, > 0, min_scale <= max_scale */
    uint32_t bloom_radius;        /* 0 off, else 1..16 */
    float bloom_threshold;        /* finite and >= 0 */
    float bloom_strength;         /* finite and >= 0 */
    uint32_t curve;               /* 0 none, 1 extended Reinhard, 2 ACES fit */
    float white;                  /* finite and > 0 (curve 1's white point) */
    uint32_t transfer;            /* 0 linear, 1 sqrt, 2 sRGB */
    uint32_t dither;              /* 0 or 1 */
} surf_display_params;
/* Conventions, not measurements: exposure auto with the photographic key 0.18,
 * min_scale 1/64, max_scale 64, exposure 1; bloom off (radius 0), threshold 1,
 * strength 0.1; curve ACES, white 4; transfer sRGB; dither on. */
int surf_display_default_params(surf_display_params* params);
typedef struct {
    uint32_t hist[256];
    uint32_t counted, black, median_bin;
    float scale;
} surf_display_meter_result;
/* The context form, on the context's accumulator (each pixel divided by its
 * own .w); out_rgba8 height*width words, meter may be NULL.  Drains the
 * stream.  SURF_ERR_INVALID for a NULL context, params or out_rgba8,
 * parameters outside the ranges above, an accumulator nothing was rendered
 * into since the last clear, and on a row shard -- the meter and the blur read
 * the whole frame: assemble the shards' accumulators and call
 * surf_display_image; SURF_ERR_OOM when a scratch image cannot be allocated. */
int surf_display(surf_ctx* ctx, const surf_display_params* params, uint32_t* out_rgba8, surf_display_meter_result* meter);
/* A host plane of any w x h frame (w*h in 1..2^27, w*h*4 floats): a filter's
 * output (w = 1), an accumulator or a robust accumulator (w = the count).
 * Needs no scene on the context. */
int surf_display_image(surf_ctx* ctx, uint32_t w, uint32_t h, const float* rgba, const surf_display_params* params,
                       uint32_t* out_rgba8, surf_display_meter_result* meter);
/* ... the same from a plane on the context's device (w*h*16 bytes, e.g. what a
 * filter's _copy_device form filled) to words on the device (w*h*4 bytes): no
 * round trip through the host.  meter is a host pointer or NULL. */
int surf_display_image_device(surf_ctx* ctx, uint32_t w, uint32_t h, const void* src_rgba_device, const surf_display_params* params,
                              void* dst_rgba8_device, surf_display_meter_result* meter);
/* The CPU twin; needs no device.  Bit-identical to surf_display_image. */
int surf_display_image_host(uint32_t w, uint32_t h, const float* rgba, const surf_display_params* params, uint32_t* out_rgba8,
                            surf_display_meter_result* meter);
/* The two tables of the interface: T of rule 7 and B8 of rule 8 (row-major). */
int surf_display_srgb_table(float out[4096]);
int surf_display_bayer8(uint8_t out[64]);
/* Diagnostics: device times (HIP events) of the last run's stages into
 * kernel_ms[0..count): meter, scale, blur (the horizontal pass; 0 without
 * bloom), pack (with bloom: the vertical pass fused with it). */
int surf_debug_display_time(surf_ctx* ctx, float* kernel_ms, uint32_t count);

/* ---- the surfel sensor: path-traced irradiance at the caller's texels (no reference counterpart) ----
 * A context's samples start at its sensor.  After surf_create* that is the
 * camera.  With a surfel sensor set, surf_render starts every sample at a
 * surface point the caller gave -- a light-map texel, an irradiance probe's
 * facet, a pixel's first hit -- and gathers the light that arrives there; the
 * accumulator, the squares and bucket planes, the masks, the adaptive loops
 * and every *_image filter then work on that light map as on any image.
 *
 * Definition.  All arithmetic is f32 and uncontracted.  Texel lp of the shard
 * (rows*width, shard row order like the accumulator) has P = position[lp].xyz
 * and N = normal[lp].xyz; both w components are ignored.  The texel is VALID
 * iff N.x != 0 || N.y != 0 || N.z != 0 -- so a NaN normal component makes the
 * texel valid -- and surf_read_aov's miss normal is (0, 0, 0): the first-hit
 * position and normal planes can be handed in as they are.  N is used as
 * given: the caller supplies a unit vector, the library does not normalize it.
 * One degenerate input is refused (SURF_ERR_INVALID, nothing changes): a normal
 * with a nonzero component whose squared length x*x + y*y + z*z, in f32, lies
 * below FLT_MIN -- step 1's retry test dot(R, N) == 0 could then hold on every
 * try and the sample never start.  A NaN or infinite component is not refused.
 * Sample j of frame k of a valid texel is seeded as surf_render states above:
 * seed = initSeed(p + 1799 * (first_sample_index + k*spp)) for j = 0, with
 * p = x + row*width over the whole image; for j > 0 the seed is the state the
 * previous sample's path left.  Then
 *   1. R = cosineSample(seed, N): the path tracer's own
 *      randomOnHemisphereCosineWeighted loop, with its retry;
 *   2. o = P + 1e-5f * R, computed as add(P, lscl(kEps, R)): the continuation
 *      origin of a diffuse bounce;
 *   3. d = R;
 *   4. the path enters Renderer::trace's loop exactly as a camera ray does:
 *      throughput (1, 1, 1), no medium, last bounce specular, segment 1, RNG
 *      state seed -- an emitter met on the first segment therefore counts;
 *   5. (energy, 1) is accumulated per sample, in sample order.
 * accumulator.rgb / w then estimates E / pi, with E the irradiance at P about
 * N: the radiosity of a white diffuse texel.
 *
 * Validity and the mask.  An invalid texel is never issued: its accumulator,
 * squares and bucket records stay untouched and its w does not advance,
 * exactly like an inactive pixel of the mask.  The effective active set is
 * mask AND valid: wherever the context's mask is set or built
 * (surf_set_pixel_mask, surf_mask_from_noise, surf_mask_from_nlm, the reset by
 * surf_clear_accumulator, both adaptive loops) an invalid texel's byte is
 * forced to 0 before the compaction, and surf_get_pixel_mask reports the
 * forced bytes.  An all-valid sensor with no mask takes the unmasked kernels
 * and issue order.  With no valid texel at all surf_render returns SURF_OK and
 * changes nothing.
 *
 * State.  The library copies both planes into buffers of its own (2 x 16 B
 * and 1 B per texel, allocated on first use).  Setting or clearing a sensor
 * drains and ends the open stream, as a mask change does, and sets the mask
 * back to every (valid) texel.  The sensor survives surf_set_camera,
 * surf_upload_scene, surf_update_instances and surf_clear_accumulator: the
 * points are the caller's world-space data.  surf_render's requirements do not
 * change: it still needs a scene and a camera.
 *
 * Scheduling (none of it affects results).  Under a sensor the permuted head
 * of the stream, which classifies pixels by the camera's centre rays, is not
 * used: issue is frame-major.  Surfel rays take the camera rays' pool key.
 *
 * What stays as it is.  surf_read_aov*, surf_read_ao and every filter keep
 * describing the camera.  With a sensor set, the context forms of the guided
 * filters (surf_denoise, surf_svgf, surf_denoise_sampled, surf_denoise_regress,
 * surf_temporal_accumulate) make sense only when the surfels ARE those planes
 * -- the view baked at its own first hits; nothing is refused.  The *_image
 * forms, the noise estimate, the robust estimate, the non-local-means filter,
 * both adaptive loops, surf_finalize_rgba8_weighted and the display stage
 * operate on the light map as on any image.  surf_stats counts what was traced.
 *
 * Device side: the kernels that start a sample (k_regen, k_regen_count,
 * k_shade and the three drain kernels) have a second instantiation that reads
 * the texel's two 16-byte records in place of the camera; the camera's
 * instantiations are unchanged. */
#define SURF_SENSOR_CAMERA 0
#define SURF_SENSOR_SURFELS 1
/* position, normal: rows*width float4 records each, shard row order like the
 * accumulator; host pointers.  NULL, NULL: back to the camera.  One NULL:
 * SURF_ERR_INVALID (as for a NULL context, and for a nonzero normal whose
 * squared length underflows, see above).  SURF_ERR_OOM when the copies cannot
 * be allocated.  A call that fails before its copies leaves the sensor as it
 * was; one whose copies fail leaves the context on the camera with no mask. */
int surf_set_surfel_sensor(surf_ctx* ctx, const float* position, const float* normal);
/* the same from device pointers on the context's device (e.g. what surf_copy_aov_device wrote) */
int surf_set_surfel_sensor_device(surf_ctx* ctx, const void* position_device, const void* normal_device);
/* *kind = SURF_SENSOR_CAMERA or SURF_SENSOR_SURFELS; *valid = valid texels (rows*width for the camera); either may be NULL */
int surf_get_sensor(surf_ctx* ctx, int* kind, uint32_t* valid);

/* ---- the light-map atlas: UV rasterizer to surfels, finish, gutter fill (no reference counterpart) ----
 * What stands between a mesh with UVs and a light-map texture, around the
 * surfel sensor above: surf_atlas_build turns the UV layout of charts into one
 * surfel per texel (the planes surf_set_surfel_sensor takes), surf_atlas_finish
 * turns the baked accumulator into the texture, surf_atlas_dilate fills the
 * gutters bilinear sampling reads at chart borders.  The atlas is W x H texels
 * of its own, whatever the context's frame: the context supplies the device
 * and the stream (a sharded context serves as well).  Each stage has a device
 * form and a CPU twin (_host, no context) that agree bit for bit.  All
 * arithmetic is f32, every operation rounded on its own, nothing contracted,
 * in the order written.
 *
 * 1. surf_atlas_build.  Reads of the desc only triangles, tri_ext,
 * triangle_count, instances, instance_count, materials, material_count: no BVH
 * is needed.  Chart k maps the mesh of instance charts[k].instance; that mesh
 * is the triangles from the instance's tri_offset up to the next larger
 * tri_offset among the desc's instances, or triangle_count.
 *
 * Corner pairing.  A record keeps the reference's pairing (Triangle's
 * constructor stores OBJ vertex 0 in v1, the extension stores corners in OBJ
 * order): OBJ corner a is (v1, n0, uv0), corner b is (v0, n1, uv1), corner c
 * is (v2, n2, uv2).  hu is the weight of v1, hv of v2, w = (1 - hu) - hv of
 * v0: the Moller-Trumbore weights of the tracer, as in its normal
 * hu n0 + hv n2 + w n1.
 *
 * Texel space.  For chart k and a record's uv (u, v):
 *   X = (u*scale[0] + offset[0]) * (float)W,  Y = (v*scale[1] + offset[1]) * (float)H.
 * A, B, C are the results for uv0, uv1, uv2.  Texel (x, y) has the centre
 * c = ((float)x + 0.5f, (float)y + 0.5f); row y = 0 is v = 0.
 *
 * Skipped triangles.  det = (A.x-B.x)*(C.y-B.y) - (A.y-B.y)*(C.x-B.x).  A
 * triangle with a non-finite coordinate among the six, or with det 0 or
 * non-finite, is skipped: counted in skipped_triangles, covering nothing.
 *
 * Coverage.  For each edge (P, Q) of (A,B), (B,C), (C,A): the endpoints are put
 * in canonical order (swapped when Q.x < P.x || (Q.x == P.x && Q.y < P.y)),
 *   e = (Q.x-P.x)*(c.y-P.y) - (Q.y-P.y)*(c.x-P.x),
 * e is negated if the endpoints were swapped, and negated again if det > 0.
 * (With A = (0,0), B = (1,0), C = (0,1), det is -1 and the three e at the
 * interior point (1/4, 1/4) are 1/4, 1/2, 1/4: a triangle with det < 0 has
 * e >= 0 inside without the last negation, so det > 0 is the sense that
 * flips.)  The centre is covered iff all three e >= 0 and it lies in the
 * triangle's bounding box grown by one texel:
 *   min(A.x,B.x,C.x) - 1.0f <= c.x <= max(A.x,B.x,C.x) + 1.0f, likewise y.
 * The box is one condition more than "all three e >= 0": it is what the tile
 * expansion culls by, and stating it makes that culling exact in f32 instead
 * of an unproved superset.  In exact arithmetic the edge tests imply it.  In
 * f32 it can exclude only a centre that lies more than one texel outside the
 * triangle and that rounding in the edge functions admitted all the same,
 * which takes coordinates of the order of 2^23 texels; a centre within a
 * texel of a triangle -- every centre near a shared edge or vertex of a mesh
 * inside the atlas -- is decided by the edge functions alone, so the box drops
 * no centre between neighbours.  Negation is exact: two
 * triangles sharing an edge with bit-identical endpoints evaluate the same
 * number for it with opposite signs, so no centre between them is dropped and a
 * centre exactly on the edge is covered by both.  A mirrored chart (a negative
 * scale) covers what its unmirrored twin covers.  Partially covered texels
 * whose centre is outside are not covered (no conservative rasterization).
 *
 * Owner.  Among the triangles covering a centre the lowest key wins; the key is
 * first[k] + prim, first[k] the sum of the earlier charts' triangle counts,
 * prim the triangle's index in its mesh.  cover is the number of covering
 * triangles over all charts.  SURF_ERR_LIMIT when the charts hold 2^32 - 1
 * triangles or more.
 *
 * Surfel of an owned texel.  e1 = A-B, e2 = C-B, q = c-B,
 *   det' = e1.x*e2.y - e1.y*e2.x,
 *   hu = (q.x*e2.y - q.y*e2.x)/det',  hv = (e1.x*q.y - e1.y*q.x)/det'
 * (c = B + hu e1 + hv e2 solved by Cramer's rule; neither is clamped),
 *   Po = v0 + (hu*(v1-v0) + hv*(v2-v0)) per component,
 *   P = rows 0..2 of M (Po, 1), each row summed as (m0 x + m1 y) + (m2 z + m3 w),
 *   N = the tracer's shading normal term for term: no = (hu n0 + hv n2) + w n1,
 *       n4 = M (no, 0) with the same row sums, nn = (x*x + y*y) + (z*z + w*w)
 *       over all four, N = n4.xyz * (1.0f / sqrtf(nn)) -- without the flip
 *       against a ray.  flags bit 0 negates N.  If a component of N is then
 *       not finite (the interpolated normal vanished), N = 0: the texel is
 *       owned and never traced.
 * Planes, 16-byte records, W*H each, row-major:
 *   position  owned: (P, 1)                                    empty: 0
 *   normal    owned: (N, 0)                                    empty: 0
 *   albedo    owned: (albedo, 1); on an emitter -- strength > 0 and a colour
 *             component > 0, surf_read_aov's test -- (strength * colour, 2)
 *                                                              empty: 0
 *   ids       owned: (chart, instance, primitive, cover)       empty: (~0, ~0, ~0, 0)
 * An empty texel's zero normal is what the surfel sensor treats as invalid.
 * Summary: covered = texels with cover >= 1, overlapped = texels with
 * cover >= 2 (an overlapping UV layout is the usual mistake; shared edges that
 * pass exactly through centres count too), skipped_triangles, triangles (all
 * charts').
 * SURF_ERR_INVALID: W or H 0 or above 16384; n_charts 0; a chart whose
 * instance is out of range, whose instance's transform has a row 3 other than
 * (0, 0, 0, 1) or offsets out of range; a non-finite scale or offset; a NULL
 * desc, or NULL or empty triangles, tri_ext, instances or materials.
 *
 * Device side.  The result does not depend on the work mapping.  (a) one lane
 * per triangle computes A, B, C, det and the 8 x 8-texel tiles its clipped
 * bounding box touches, and one block scans the counts; (b) k_atlas_cover gives
 * one wave to each (triangle, tile) item, lane l at texel (l & 7, l >> 3),
 * with atomicMin on a u32 owner plane and atomicAdd on the cover plane -- both
 * order-independent, so the planes are deterministic; (c) k_atlas_resolve, one
 * lane per texel, recomputes the owner's surfel and counts the summary with one
 * atomic per wave.  SURF_ATLAS_MAP=0 (read when the context is created) keeps
 * the one-lane-per-triangle bounding-box walk as the A/B baseline: the same
 * atomics, identical planes.  An expansion of 2^32 items or more takes that
 * walk too.  The call uploads what it reads from the desc into buffers of its
 * own and frees them. */
typedef struct {
    uint32_t instance;
    uint32_t flags;             /* bit 0: flip the normal */
    float scale[2], offset[2];
} surf_atlas_chart;             /* 24 B */
typedef struct { uint32_t covered, overlapped, skipped_triangles, triangles; } surf_atlas_summary;
/* the four planes are host pointers, W*H*16 bytes each; any may be NULL, as may summary */
int surf_atlas_build(surf_ctx* ctx, const surf_scene_desc* desc, const surf_atlas_chart* charts, uint32_t n_charts, uint32_t W, uint32_t H,
                     float* position, float* normal, float* albedo, uint32_t* ids, surf_atlas_summary* summary);
/* the same with the four planes device pointers on the context's device (desc, charts and summary stay on the host) */
int surf_atlas_build_device(surf_ctx* ctx, const surf_scene_desc* desc, const surf_atlas_chart* charts, uint32_t n_charts, uint32_t W,
                            uint32_t H, void* position_device, void* normal_device, void* albedo_device, void* ids_device,
                            surf_atlas_summary* summary);
/* the CPU twin */
int surf_atlas_build_host(const surf_scene_desc* desc, const surf_atlas_chart* charts, uint32_t n_charts, uint32_t W, uint32_t H,
                          float* position, float* normal, float* albedo, uint32_t* ids, surf_atlas_summary* summary);
/* Charts on a grid, a pure host function: entry i of the list (instances NULL: instance i) gets cell i of a g x g grid,
 * g the smallest integer with g*g >= n, column i % g, row i / g.  Cell (col, row) spans texels
 * [col*W/g, (col+1)*W/g) x [row*H/g, (row+1)*H/g) in integer division, shrunk by margin_texels on every side to
 * [lo, hi); the mesh's [0,1]^2 maps onto it: scale = (float)(hi - lo) / (float)side, offset = (float)lo / (float)side per
 * axis (side W or H), flags 0.  SURF_ERR_INVALID when n is 0, out is NULL, W or H is 0 or above 16384, or the margins
 * leave nothing of a cell. */
int surf_atlas_grid_charts(uint32_t n_instances, const uint32_t* instances, uint32_t W, uint32_t H, uint32_t margin_texels,
                           surf_atlas_chart* out);
/* 2. surf_atlas_finish: accumulator to light-map texture, one lane per texel.
 *   albedo.w == 2 (an emitter shows itself):  out = (albedo.rgb, 1), valid = 1
 *   else acc.w > 0 and albedo.w == 1:         out = ((acc.r/acc.w)*albedo.r, (acc.g/acc.w)*albedo.g, (acc.b/acc.w)*albedo.b, 1), valid = 1
 *   otherwise:                                out = 0, valid = 0
 * acc is any plane in accumulator form, (sum of rgb, weight): surf_read_accumulator's, surf_robust_accumulator's out_acc,
 * or a filter's output image with w set to 1 where it is meaningful (a filtered mean is the sum of one sample).  albedo is
 * the build's plane.  out_valid is a byte per texel.  W*H records each; SURF_ERR_INVALID on a NULL argument or a size
 * outside 1..16384. */
int surf_atlas_finish(surf_ctx* ctx, uint32_t W, uint32_t H, const float* acc, const float* albedo, float* out_rgba, uint8_t* out_valid);
int surf_atlas_finish_device(surf_ctx* ctx, uint32_t W, uint32_t H, const void* acc_device, const void* albedo_device, void* out_rgba_device,
                             void* out_valid_device);
int surf_atlas_finish_host(uint32_t W, uint32_t H, const float* acc, const float* albedo, float* out_rgba, uint8_t* out_valid);
/* 3. surf_atlas_dilate: gutter fill.  Each iteration reads one buffer and writes another: a valid texel is copied as it
 * is; an invalid texel with at least one valid 8-neighbour inside the image becomes the mean of those neighbours -- per
 * channel the sum starts at 0 and runs in the order N, S, W, E, NW, NE, SW, SE (N is y - 1), then is divided by
 * (float)count, w = 1 -- and is valid from the next iteration on; an invalid texel with no valid neighbour is 0 and
 * stays invalid.  iterations 0..64; 0 copies.  The iterations are queued back to back with no trip to the host; the last
 * one writes the caller's buffers.  An output may not be its own input.  SURF_ERR_INVALID otherwise as for finish. */
int surf_atlas_dilate(surf_ctx* ctx, uint32_t W, uint32_t H, const float* rgba, const uint8_t* valid, uint32_t iterations, float* out_rgba,
                      uint8_t* out_valid);
int surf_atlas_dilate_device(surf_ctx* ctx, uint32_t W, uint32_t H, const void* rgba_device, const void* valid_device, uint32_t iterations,
                             void* out_rgba_device, void* out_valid_device);
int surf_atlas_dilate_host(uint32_t W, uint32_t H, const float* rgba, const uint8_t* valid, uint32_t iterations, float* out_rgba,
                           uint8_t* out_valid);
/* The chain on the device with buffers of the library's own on the context's device: surf_atlas_build_device at the
 * context's width x height, surf_set_surfel_sensor_device from its planes, surf_clear_accumulator, surf_render(frames,
 * first_sample_index, max_segments, samples_per_frame), the accumulator copied, the camera sensor restored (also when
 * the render failed), surf_atlas_finish_device, surf_atlas_dilate_device, then lightmap (W*H*16 B), valid (W*H bytes)
 * and, where not NULL, accumulator (W*H*16 B) and summary copied to the host.  The context's accumulator keeps the bake.
 * Needs a scene and a camera, as surf_render does, and a context that owns every row.  SURF_ERR_INVALID: a sharded
 * context, frames or samples_per_frame 0, iterations above 64, a NULL lightmap or valid, and whatever the build refuses. */
int surf_atlas_bake(surf_ctx* ctx, const surf_scene_desc* desc, const surf_atlas_chart* charts, uint32_t n_charts, uint32_t frames,
                    uint32_t first_sample_index, uint32_t max_segments, uint32_t samples_per_frame, uint32_t iterations, float* lightmap,
                    uint8_t* valid, float* accumulator, surf_atlas_summary* summary);
/* device times of the context's last runs, in ms: [0] the build's setup, scan and item-count readback, [1] its cover
 * kernel, [2] its resolve, [3] the last finish, [4] the last dilate (all iterations); a build zeroes [3] and [4].
 * *tile_map (may be NULL): 1 when the last build ran the tile mapping. */
int surf_debug_atlas_time(surf_ctx* ctx, float* kernel_ms, uint32_t count, uint32_t* tile_map);

/* ---- traversal entry points (kernel-level parity tests) ----
 * n world-space rays, o/d 3 floats each.  closest: depth starts at 1e30;
 * writes t,u,v (floats) and inst,prim (u32, ~0 on miss).  any: tmax per ray,
 * occluded[i] = 1 when a hit is found. Host buffers. */
int surf_trace_closest(surf_ctx* ctx, uint32_t n, const float* o, const float* d,
                       float* out_t, float* out_u, float* out_v, uint32_t* out_inst, uint32_t* out_prim);
int surf_trace_any(surf_ctx* ctx, uint32_t n, const float* o, const float* d, const float* tmax,
                   uint8_t* occluded);
/* 0: one ray per lane (the wavefront kernels' traversal); 1: one ray per
 * 64-lane wave, lanes as the node record's planes (the drain's traversal; any
 * TLAS; needs a BVH stack of <= 64 entries).  Results are identical; selects
 * what surf_trace_* run. */
int surf_set_trace_mode(surf_ctx* ctx, int mode);

/* ---- host scene build (the reference's main.cpp scene, OBJ assets) ----
 * variant 0: bundled indoor scene; 1: C5 deep scene (+648 Suzannes in one mesh);
 * 2 / 3: general-TLAS test scenes (+40 / +80 scattered cube, Suzanne and lens
 * instances: 51 instances with the LDS tables, 91 with global tables). */
int surf_scene_build_indoor(const char* assets_dir, int variant, surf_scene** out);
int surf_scene_desc_get(const surf_scene* scene, surf_scene_desc* out);
/* GPUScene::update (sources/scene.cpp:267-282): rotate instance 3 by
 * 1.0*delta_time radians about WORLD_UP, refit the TLAS, re-batch.  Follow
 * with surf_update_instances (or surf_upload_scene) on each context. */
int surf_scene_update(surf_scene* scene, float delta_time);
/* Reference camera of main.cpp:141-149 for a width x height render. */
int surf_scene_camera(const surf_scene* scene, uint32_t width, uint32_t height, surf_camera_ubo* out);
/* Deepest root-to-leaf edge counts of the TLAS and of all BLASes. */
int surf_scene_bvh_depths(const surf_scene* scene, uint32_t* tlas_depth, uint32_t* max_blas_depth);
void surf_scene_destroy(surf_scene* scene);

/* Image files for an RGBA8 image (R in the low byte, as surf_finalize_rgba8 /
 * surf_display_rgba8 write it), rows top to bottom: binary PPM (P6, alpha
 * dropped) or PNG (8-bit RGBA, zlib).  The reference only presents to a
 * swapchain; these are its on-disk equivalent. */
int surf_write_ppm(const char* path, uint32_t width, uint32_t height, const uint32_t* rgba8);
int surf_write_png(const char* path, uint32_t width, uint32_t height, const uint32_t* rgba8);
/* Float image file: a colour PFM ("PF\n<width> <height>\n-1.0\n", then the
 * rows BOTTOM to top, RGB as little-endian f32) of an RGBA float image given
 * rows top to bottom (the accumulator, a float feature plane); alpha is
 * dropped, the values are written bit for bit.  SURF_ERR_IO when the path
 * cannot be written. */
int surf_write_pfm(const char* path, uint32_t width, uint32_t height, const float* rgba);

/* Mesh::Mesh(path) (sources/mesh.cpp:69-154, tinyobjloader triangulate=true):
 * .obj or .obj.gz parsed in parallel chunks (threads = 0: default count).  The
 * triangles (64 B reference Triangle, OBJ corner 0 stored in v1) and
 * TriExtensions (80 B) are identical for every thread count. */
typedef struct surf_mesh surf_mesh;
int surf_obj_load(const char* path, uint32_t threads, surf_mesh** out);
int surf_mesh_data(const surf_mesh* mesh, const surf_triangle** triangles, const surf_tri_extension** tri_ext,
                   uint32_t* count);
void surf_mesh_destroy(surf_mesh* mesh);

/* BvhBLAS::build (sources/bvh.cpp:255-465: binned SAH, 8 bins, pre-order pair
 * allocation) over `count` reference Triangles, multi-threaded (threads = 0:
 * SURF_BUILD_THREADS / OMP_NUM_THREADS / hardware).  Writes the reference's
 * index permutation (count) and node pool (nodes_out needs 2*count records;
 * *nodes_used are written).  The arrays are identical for every thread count. */
int surf_bvh_build(const surf_triangle* triangles, uint32_t count, uint32_t threads, uint32_t* indices_out,
                   surf_bvh_node* nodes_out, uint32_t* nodes_used);

#ifdef __cplusplus
}  /* extern "C" */

static_assert(sizeof(surf_triangle) == 64, "Triangle is 64 B");
static_assert(sizeof(surf_tri_extension) == 80, "TriExtension is 80 B");
static_assert(sizeof(surf_bvh_node) == 48, "BvhNode is 48 B");
static_assert(sizeof(surf_material) == 64, "Material is 64 B");
static_assert(sizeof(surf_gpu_instance) == 160, "GPUInstance is 160 B");
static_assert(sizeof(surf_light) == 8, "GPULightData is 8 B");
static_assert(sizeof(surf_background) == 64, "SceneBackground is 64 B");
static_assert(sizeof(surf_camera_ubo) == 128, "CameraUBO is 128 B");
#endif

#endif /* SURF_HIP_H */
