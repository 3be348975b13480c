/*
 * types.h -- the plain-data records and constants the host and the kernels
 * share: scene tables, camera, path pool, shadow queue, stream counters.  No
 * device code: host translation units that launch no kernel include this and
 * not the kernel headers.
 */
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "lds_layout.h"

namespace surfdev {

constexpr uint32_t kUnset = 0xffffffffu;
constexpr uint32_t kFlagMedium = 1u, kFlagSpecular = 2u;
constexpr int kBlock = 256;

struct DevInstance {          /* 160 B */
    float Minv[16];
    float M[16];
    uint32_t triOffset, idxOffset, nodeOffset, material;
    float area;
    uint32_t affineInv;       /* Minv row 3 == (0,0,0,1): w == 1 exactly for finite points */
    uint32_t affine;          /* M row 3 == (0,0,0,1) */
    uint32_t _pad;
};

struct DevMaterial {          /* = Material (64 B) */
    float emit, refl, refr, ior;
    float ec[4], albedo[4], absorb[4];
};

/* Per-instance traversal record (176 B), host-built at upload: rows of M^-1
 * (row i = m[i], m[4+i], m[8+i], m[12+i]), offsets, and the BLAS root record.
 * Kernels stage the table in LDS, so the per-instance loop of every ray reads
 * LDS instead of paying two dependent memory trips per instance. */
struct TraceInst {
    float4 m0, m1, m2, m3;
    uint4 meta;               /* nodeOffset, idxOffset, affineInv, instance id */
    float4 r0, r1, r2, r3;    /* root node record */
    float4 wlo, whi;          /* conservative world box of the BLAS's triangles (wlo.w != 0: usable) */
};
constexpr uint32_t kLdsTraceInst = 64;   /* instances staged in LDS (11 KB) */

struct DevScene {
    const TraceInst* tinst;   /* [nInst], instance-id order */
    const float4* nodes;      /* BLAS: 4 float4 per node (see upload) */
    const float4* tris;       /* 3 float4 per BLAS index slot: (v0, prim), e1, e2 */
    const float4* normals;    /* 3 float4 per global triangle: n0, n1, n2 */
    const float4* verts;      /* reference Triangle records (v0, v1, v2, centroid) */
    const float4* tlasNodes;  /* 4 float4 per TLAS node */
    const uint32_t* tlasIdx;
    const DevInstance* inst;
    const DevMaterial* mats;
    const uint2* lights;      /* (instance, primitive count) */
    uint32_t nLights;
    /* the emitters' BLAS k_connect stages in LDS (sbRecN = 0: none): the
     * instances whose BLAS root is node sbNode0 walk its sbRecN interior records
     * in compact form (sbRec: the children's boxes, each child an interior
     * record index or a leaf's triangle range -- no leaf records) and its sbTriN
     * triangle slots (S.tris + 3 * sbTri0) from LDS */
    uint32_t sbNode0, sbRecN, sbTri0, sbTriN;
    const float4* sbRec;
    uint32_t nInst, nMats;
    uint32_t tlasLeafCount;   /* TLAS root is a leaf with this many instances (0: general TLAS) */
    uint32_t finiteBoxes;     /* every BLAS node box is finite: slabFinite is exact */
    uint32_t nodes4G;         /* every BLAS-local record offset (64 B each) fits 32 bits: the asm wave walk's buffer offsets */
    const float* wnodes;      /* two-level records (48 floats per BLAS node, see surf_upload_scene), or null */
    uint32_t nWnodes;         /* nodes in wnodes (every 192-B offset fits 32 bits) */
    uint32_t laneW;           /* the one-ray-per-lane traversal walks the two-level records too (HBM-resident BVHs) */
    float cullRadius;         /* the instance world boxes cull only rays whose origin coordinates lie within it (buildInstanceTables) */
    uint32_t bgType;
    float bgColor[3], bgA[3], bgB[3];
    float cellLo[3], cellScale[3];   /* ray-order cells: the TLAS root box split in 2 per axis (scale 0: one cell) */
    /* ray-order membership key (single-leaf TLAS): the world boxes of the (at
     * most 3) instances with the largest BLASes; keyMode 1: pool key by them */
    uint32_t nHeavy, keyMode;
    float4 hvLo[3], hvHi[3];
    /* leaf runs of a single-leaf TLAS (traceScene, leafRun), one bit per TLAS
     * position: runMember = the position belongs to a run, runHead = it is the
     * run's first.  A run is kLeafRunMin..kLeafRunMax consecutive positions
     * whose instances are affine root leaves of at most kLeafRunTris triangles
     * over one triangle range (the room's planes).  0: no runs */
    unsigned long long runHead, runMember;
};
/* kLeafRunMax: the lanes' 32-bit mask; kLeafRunPositions: runs lie in the first 63
 * TLAS positions, so the walk's look at the bit behind a run never shifts by 64 */
constexpr uint32_t kLeafRunTris = 2, kLeafRunMin = 2, kLeafRunMax = 32, kLeafRunPositions = 63;

struct DevCamera {
    float pos[3], firstPixel[3], uVec[3], vVec[3], diskU[3], diskV[3];
    float invW, invH;
    uint32_t defocus;
};

/* Path pool: od[2i] = (origin, sample id), od[2i + 1] = (direction, flags) --
 * the ray a traversal reads is one 32-B piece of one cache line, also when it
 * is gathered through the ray order -- T[i] = (throughput, rng state),
 * key[i] = ray-order bin (start instance). */
struct Pool { float4* od; float4* T; uint8_t* key; };

/* Shadow queue: od[2i] = (origin, tmax), od[2i + 1] = (direction, sample id)
 * -- the ray k_connect traverses is one 32-B piece of one cache line --
 * c[i] = (T * Ld, 0), read only for an unoccluded ray.  k_shade appends each
 * shadow ray straight into the region of its order bin (shadowKey: Q.bins
 * regions of `region` slots, then an overflow region of the pool's capacity
 * for a bin that outgrows its region), so k_connect reads the rays in bin
 * order sequentially: no sort pass and no gather through an order array.
 * The key layouts (SURF_SH_KEY, shadowKey) use 16, 32 or 40 bins; kShBins is
 * the most a layout may use, which sizes the LDS arrays and the cursor array.
 * At most 63: one atomic instruction of k_shade's wave 0 reserves every bin
 * and the continuations. */
constexpr uint32_t kShBins = 40;
constexpr uint32_t kShBinsBase = 16; /* layout 0: light slot (mod 2) x octant cell */
static_assert(kShBins <= 63u, "k_shade reserves kShBins bins + the continuations in one wave instruction");
/* Each bin's cursor and region are split by XCD (SURF_SH_XCDS parts, the
 * appending workgroup's HW_REG_XCC_ID) and the cursors lie SURF_SH_STRIDE words
 * apart: every workgroup iteration of k_shade reserves once per non-empty bin,
 * and same-address device atomics serialize. */
#ifndef SURF_SH_XCDS
#define SURF_SH_XCDS 1
#endif
#ifndef SURF_SH_STRIDE
#define SURF_SH_STRIDE 32
#endif
constexpr uint32_t kShXcds = SURF_SH_XCDS, kShStride = SURF_SH_STRIDE;
constexpr uint32_t kShSegs = kShBins * kShXcds + 1u;      /* the most queue segments: (bin, XCD) regions, then the overflow */
struct ShadowQ {
    float4* od; float4* c;
    uint32_t* cur;        /* [2 parities][kShSegs] cursors, kShStride words apart (may count past a region's end) */
    uint32_t region;      /* slots per (bin, XCD) region */
    /* bins in use: 16, 32 or 40 (the key layout, shadowKey), or 1: no shadow
     * order (SURF_SORT=0/2).  Segments 0 .. bins * kShXcds - 1 are the bins'
     * regions, segment shOverflowSeg(bins) -- behind at least 16 bins -- is
     * the overflow; the cursors behind it stay 0 */
    uint32_t bins;
};

/* Device counters of the sample stream.  Double-buffered by phase parity so no
 * kernel writes a word another block of the same launch still reads. */
struct Counters {
    uint32_t nIn[2];                 /* paths in pool[p] when a phase reads it */
    uint32_t app[2];                 /* phase parity p: paths appended to pool[p^1] (the shadow
                                        queue's cursors are ShadowQ::cur) */
    uint32_t maxSeg;                 /* 0 = unbounded */
    uint32_t zeroCutoff;             /* end paths whose throughput is exactly 0 (radiance-neutral) */
    uint32_t segMax;                 /* longest finished path (extension rays), diagnostics */
    uint32_t survN;                  /* k_tail survivors appended (may exceed survCap) */
    uint32_t survCap;
    uint32_t rowNext;                /* k_tail_pair path queue: next path to hand out */
    /* issue order of the stream's first permFrames frames: every frame's
     * samples of the permA pixels listed first in StreamGeom::perm, then each
     * frame's other pixels frame by frame (0: frame-major throughout) */
    uint32_t permFrames, permA;
    /* samples per frame (config().samplesPerFrame, renderer.cpp:171): a frame's
     * samples of one pixel form a chain -- sample k + 1 starts from the RNG state
     * sample k's path left -- so k_regen issues only the first sample of each
     * (frame, pixel) and the kernel that ends a sample's path starts the next */
    uint32_t spp;
    /* masked streams (surf_set_pixel_mask): the length of the active-pixel list
     * StreamGeom::perm then points to; k_regen<true> issues frame-major over it.
     * Takes the word the 64-bit members' alignment left free: no other offset moves. */
    uint32_t nActive;
    unsigned long long issued[2];    /* stream chains issued (first samples of (frame, pixel)), per parity */
    unsigned long long limit;        /* host-written issue limit (frame window) */
    unsigned long long baseFrame;    /* absolute frame index of stream frame 0 */
    unsigned long long ev[16];       /* ext, hit, cont, shadow, acc, unocc, tail paths, capped paths, wavefront ext,
                                        shadow rays queued in the overflow region */
    uint32_t capped[64];             /* sample ids of paths ended by the segment cap, slot blockIdx % 64 (diagnostics, ~0 = none) */
    /* event counts striped over kStripes cache lines (block b adds to stripe
     * b % kStripes): a counter shared by every block of a launch serializes its
     * atomics (~12 ns each, measured); totals = ev + sum over stripes */
    unsigned long long evS[32][16];
    unsigned long long dbg[8];       /* SURF_SEG_TIMING builds: k_tail_coop cycles (extend, shade, connect, segments) */
};
static_assert(offsetof(Counters, issued) == 56, "nActive fills the alignment gap in front of issued");
constexpr uint32_t kStripes = 32;    /* frameDone and event-count stripes */
constexpr int kEvents = 10;          /* event kinds counted (ev / evS index) */

/* Where a stream sample lives: radiance slot sid = (pass % window) * npx + pixel,
 * pass = the sample's index in the stream (frame * spp + its place in the
 * frame; window is a multiple of spp, so a frame's samples occupy consecutive
 * slots and slot % spp is the place in the frame). */
struct StreamGeom {
    const uint32_t* rows;            /* shard rows */
    uint32_t width, npx, window;
    const uint32_t* perm;            /* local pixels, class A (Counters::permA of them) first; a masked stream's
                                        graph: the ascending active-pixel list (Counters::nActive of them) */
};
/* The stream geometry of a stream under a surfel sensor (surf_set_surfel_sensor):
 * the same record and behind it the sensor's two planes, npx float4 records
 * each in the shard's row order -- texel lp starts its samples at position[lp]
 * about normal[lp] (surfelSample).  Only the SURFEL instantiations take this
 * type: the camera kernels' arguments are what they were. */
struct SurfelGeom : StreamGeom {
    const float4* position;
    const float4* normal;
};
/* the stream-geometry argument of a kernel instantiated for the camera (false) or for a surfel sensor (true) */
template <bool SURFEL> struct GeomOf { using type = StreamGeom; };
template <> struct GeomOf<true> { using type = SurfelGeom; };
template <bool SURFEL> using Geom = typename GeomOf<SURFEL>::type;

/* Record encodings the upload writes and the walks read */
constexpr uint32_t kLeafTagC = 0x80000000u;   /* compact staged BLAS (blasAnyStaged): a child that is a leaf */
constexpr uint32_t kLeafTag = 0x80000000u;    /* two-level records (blasTraceW): a packed leaf reference */
constexpr uint32_t kLeafInW = 3;     /* triangles a two-level leaf record holds */

/* shading tables staged in LDS when the scene has at most this many (ShadeTables) */
constexpr uint32_t kLdsInst = 64, kLdsMats = 64, kLdsLights = 64;

constexpr int kDenoiseMaxIterations = 6;      /* a-trous levels a denoise call may ask for */

/* the element sizes device/lds_layout.h counts in words */
static_assert(sizeof(TraceInst) == 4 * layout::kTraceInstWords && sizeof(DevInstance) == 4 * layout::kInstanceWords &&
                  sizeof(DevMaterial) == 4 * layout::kMaterialWords && sizeof(uint2) == 4 * layout::kLightWords &&
                  sizeof(float4) * 4 == 4 * layout::kNodeRecWords && sizeof(float4) * 3 == 4 * layout::kTriRecWords,
              "lds_layout.h states the table elements' sizes");

}  // namespace surfdev
