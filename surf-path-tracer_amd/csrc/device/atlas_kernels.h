/*
 * atlas_kernels.h -- the light-map atlas (include/surf_hip.h, "the light-map
 * atlas"): the rasterizer that turns the UV layout of a chart's triangles into
 * one surfel per texel, the finish from an accumulator to the texture and the
 * gutter fill.  The arithmetic is SURF_HD: the kernels and the CPU twins
 * (host/atlas.hip) run the same functions, f32, nothing contracted, so the
 * planes agree bit for bit.  Reads the caller's scene records as they are
 * (surf_triangle, surf_tri_extension, surf_gpu_instance, surf_material): nothing
 * of DevScene, no BVH, nothing of the captured graph.  No reference counterpart.
 */
#pragma once
#include "surf_hip.h"
#include "surf_math.h"
#include "types.h"

namespace surfdev {

constexpr uint32_t kAtlasMaxSide = 16384;    /* W and H at most */
constexpr uint32_t kAtlasTile = 8;           /* a wave's tile is 8 x 8 texels */
constexpr uint32_t kAtlasMaxIterations = 64; /* surf_atlas_dilate */
constexpr uint32_t kAtlasBlock = 256;

/* a chart as the kernels read it: the caller's record, the triangle range of its instance's mesh, the key of
 * its first triangle (the running sum of the earlier charts' triangle counts) and its material */
struct AtlasChart {
    uint32_t instance, flags, tri0, triN;
    uint32_t first, material;
    float sx, sy, ox, oy;
    uint32_t _pad[2];
};

/* a triangle in texel space: A from uv0, B from uv1, C from uv2, det, and whether it is skipped */
struct AtlasTri {
    float ax, ay, bx, by, cx, cy, det;
    uint32_t skip;
};

SURF_HD bool atlasFinite(float v) { return fabsf(v) <= 3.40282347e38f; }

/* Texel space: X = (u*scale[0] + offset[0]) * (float)W, Y = (v*scale[1] + offset[1]) * (float)H; det; the skip rule */
SURF_HD AtlasTri atlasTriangle(const AtlasChart& ch, const surf_tri_extension& x, float Wf, float Hf) {
    AtlasTri t;
    t.ax = (x.uv0[0] * ch.sx + ch.ox) * Wf; t.ay = (x.uv0[1] * ch.sy + ch.oy) * Hf;
    t.bx = (x.uv1[0] * ch.sx + ch.ox) * Wf; t.by = (x.uv1[1] * ch.sy + ch.oy) * Hf;
    t.cx = (x.uv2[0] * ch.sx + ch.ox) * Wf; t.cy = (x.uv2[1] * ch.sy + ch.oy) * Hf;
    t.det = (t.ax - t.bx) * (t.cy - t.by) - (t.ay - t.by) * (t.cx - t.bx);
    const bool fin = atlasFinite(t.ax) && atlasFinite(t.ay) && atlasFinite(t.bx) && atlasFinite(t.by) && atlasFinite(t.cx) &&
                     atlasFinite(t.cy);
    t.skip = (!fin || !atlasFinite(t.det) || t.det == 0.0f) ? 1u : 0u;
    return t;
}

/* The edge function of (P, Q) at the centre c: endpoints in canonical order, negated back when they were swapped,
 * negated again when det > 0 -- so a triangle of either orientation has e >= 0 on its own side of every edge, and
 * two triangles sharing an edge with bit-identical endpoints evaluate the same number with opposite signs. */
SURF_HD float atlasEdge(float px, float py, float qx, float qy, float cx, float cy, bool detPositive) {
    const bool swapped = qx < px || (qx == px && qy < py);
    if (swapped) { const float tx = px, ty = py; px = qx; py = qy; qx = tx; qy = ty; }
    float e = (qx - px) * (cy - py) - (qy - py) * (cx - px);
    if (swapped) e = -e;
    if (detPositive) e = -e;
    return e;
}

/* the triangle's bounding box; the coordinates are finite */
SURF_HD void atlasBox(const AtlasTri& t, float& x0, float& x1, float& y0, float& y1) {
    x0 = tmin(tmin(t.ax, t.bx), t.cx); x1 = tmax(tmax(t.ax, t.bx), t.cx);
    y0 = tmin(tmin(t.ay, t.by), t.cy); y1 = tmax(tmax(t.ay, t.by), t.cy);
}

/* Coverage of the centre (cx, cy) by a triangle that is not skipped: inside the bounding box grown by one texel on
 * every side and all three edge functions >= 0.  The box is what the tile expansion culls by, so it is part of the
 * definition; grown by a texel it can only exclude a centre that lies more than a texel outside the triangle. */
SURF_HD bool atlasCovers(const AtlasTri& t, float cx, float cy) {
    float x0, x1, y0, y1;
    atlasBox(t, x0, x1, y0, y1);
    if (!(cx >= x0 - 1.0f && cx <= x1 + 1.0f && cy >= y0 - 1.0f && cy <= y1 + 1.0f)) return false;
    const bool pos = t.det > 0.0f;
    const float e0 = atlasEdge(t.ax, t.ay, t.bx, t.by, cx, cy, pos);
    const float e1 = atlasEdge(t.bx, t.by, t.cx, t.cy, cx, cy, pos);
    const float e2 = atlasEdge(t.cx, t.cy, t.ax, t.ay, cx, cy, pos);
    return e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f;
}

/* Texels [a, b] of an axis of n whose centres can lie in [lo, hi], the grown box's interval (a superset: a centre
 * i + 0.5 in the interval has i > lo - 1 and i <= hi); false: none. */
SURF_HD bool atlasRange(float lo, float hi, uint32_t n, uint32_t& a, uint32_t& b) {
    if (hi < 0.0f || lo > (float)n) return false;
    const float l = tmax(lo, 0.0f), h = tmin(hi, (float)n);
    a = (uint32_t)floorf(l);
    a = a > 0u ? a - 1u : 0u;
    b = (uint32_t)floorf(h);
    if (b > n - 1u) b = n - 1u;
    return true;
}

/* the texels a triangle's clipped bounding box can cover; false: none, or the triangle is skipped */
SURF_HD bool atlasTexelBox(const AtlasTri& t, uint32_t W, uint32_t H, uint32_t& xa, uint32_t& xb, uint32_t& ya, uint32_t& yb) {
    if (t.skip) return false;
    float x0, x1, y0, y1;
    atlasBox(t, x0, x1, y0, y1);
    return atlasRange(x0 - 1.0f, x1 + 1.0f, W, xa, xb) && atlasRange(y0 - 1.0f, y1 + 1.0f, H, ya, yb);
}

/* the 8 x 8 tiles that box touches (0: none): 2048 x 2048 at most */
SURF_HD uint32_t atlasTileCount(const AtlasTri& t, uint32_t W, uint32_t H) {
    uint32_t xa, xb, ya, yb;
    if (!atlasTexelBox(t, W, H, xa, xb, ya, yb)) return 0u;
    return ((xb / kAtlasTile) - (xa / kAtlasTile) + 1u) * ((yb / kAtlasTile) - (ya / kAtlasTile) + 1u);
}

/* the four records of an owned texel */
struct AtlasSurfel {
    float4 position, normal, albedo;
    uint4 ids;
};

/* the chart that holds key: the last one whose first <= key (charts with no triangle share a first with their
 * successor, which the search passes over) */
SURF_HD uint32_t atlasChartOf(const AtlasChart* charts, uint32_t nCharts, uint32_t key) {
    uint32_t lo = 0u, hi = nCharts;          /* first[lo] <= key < first[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (charts[mid].first <= key) lo = mid; else hi = mid;
    }
    return lo;
}

/* The surfel of the texel with centre (cx, cy) owned by triangle `prim` of chart k: the Moller-Trumbore weights of
 * the centre in texel space, the object point through M, hitNormal's expression without its flip against a ray. */
SURF_HD AtlasSurfel atlasSurfel(const AtlasChart& ch, uint32_t k, uint32_t prim, const AtlasTri& t, const surf_triangle& tr,
                                const surf_tri_extension& x, const surf_gpu_instance& I, const surf_material& m, float cx, float cy,
                                uint32_t cover) {
    const float e1x = t.ax - t.bx, e1y = t.ay - t.by, e2x = t.cx - t.bx, e2y = t.cy - t.by;
    const float qx = cx - t.bx, qy = cy - t.by;
    const float det = e1x * e2y - e1y * e2x;
    const float hu = (qx * e2y - qy * e2x) / det;
    const float hv = (e1x * qy - e1y * qx) / det;
    const V3 v0 = mk3(tr.v0.x, tr.v0.y, tr.v0.z), v1 = mk3(tr.v1.x, tr.v1.y, tr.v1.z), v2 = mk3(tr.v2.x, tr.v2.y, tr.v2.z);
    const V3 Po = add(v0, add(lscl(hu, sub(v1, v0)), lscl(hv, sub(v2, v0))));
    const float* M = I.transform;
    const V3 P = mk3(mrow(M, 0, Po.x, Po.y, Po.z, 1.0f), mrow(M, 1, Po.x, Po.y, Po.z, 1.0f), mrow(M, 2, Po.x, Po.y, Po.z, 1.0f));
    const float w = (1.0f - hu) - hv;
    const V3 n0 = mk3(x.n0.x, x.n0.y, x.n0.z), n1 = mk3(x.n1.x, x.n1.y, x.n1.z), n2 = mk3(x.n2.x, x.n2.y, x.n2.z);
    const V3 no = add(add(lscl(hu, n0), lscl(hv, n2)), lscl(w, n1));
    const float nx4 = mrow(M, 0, no.x, no.y, no.z, 0.0f), ny4 = mrow(M, 1, no.x, no.y, no.z, 0.0f);
    const float nz4 = mrow(M, 2, no.x, no.y, no.z, 0.0f), nw4 = mrow(M, 3, no.x, no.y, no.z, 0.0f);
    const float nn = (nx4 * nx4 + ny4 * ny4) + (nz4 * nz4 + nw4 * nw4);
    const float ninv = 1.0f / sqrtf(nn);
    V3 N = mk3(nx4 * ninv, ny4 * ninv, nz4 * ninv);
    if (ch.flags & 1u) N = mk3(-N.x, -N.y, -N.z);
    if (!finite3(N)) N = mk3(0.0f, 0.0f, 0.0f);          /* no normal to speak of: the texel is owned and never traced */
    const bool isLight = m.emission_strength > 0.0f && (m.emission_color.x > 0.0f || m.emission_color.y > 0.0f || m.emission_color.z > 0.0f);
    const V3 a = isLight ? lscl(m.emission_strength, mk3(m.emission_color.x, m.emission_color.y, m.emission_color.z))
                         : mk3(m.albedo.x, m.albedo.y, m.albedo.z);
    AtlasSurfel s;
    s.position = make_float4(P.x, P.y, P.z, 1.0f);
    s.normal = make_float4(N.x, N.y, N.z, 0.0f);
    s.albedo = make_float4(a.x, a.y, a.z, isLight ? 2.0f : 1.0f);
    s.ids = make_uint4(k, ch.instance, prim, cover);
    return s;
}

/* the whole resolve of one texel from its owner key and cover count */
SURF_HD AtlasSurfel atlasResolve(const AtlasChart* charts, uint32_t nCharts, const AtlasTri* tris, const surf_triangle* tr,
                                 const surf_tri_extension* ext, const surf_gpu_instance* inst, const surf_material* mats, uint32_t key,
                                 uint32_t cover, uint32_t x, uint32_t y) {
    if (key == kUnset) {
        AtlasSurfel s;
        s.position = s.normal = s.albedo = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s.ids = make_uint4(kUnset, kUnset, kUnset, 0u);
        return s;
    }
    const uint32_t k = atlasChartOf(charts, nCharts, key);
    const AtlasChart ch = charts[k];
    const uint32_t prim = key - ch.first, g = ch.tri0 + prim;
    return atlasSurfel(ch, k, prim, tris[key], tr[g], ext[g], inst[ch.instance], mats[ch.material], (float)x + 0.5f, (float)y + 0.5f,
                       cover);
}

/* surf_atlas_finish's texel */
SURF_HD void atlasFinish(float4 acc, float4 alb, float4& out, uint8_t& valid) {
    out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    valid = 0;
    if (alb.w == 2.0f) {
        out = make_float4(alb.x, alb.y, alb.z, 1.0f);
        valid = 1;
    } else if (acc.w > 0.0f && alb.w == 1.0f) {
        out = make_float4((acc.x / acc.w) * alb.x, (acc.y / acc.w) * alb.y, (acc.z / acc.w) * alb.z, 1.0f);
        valid = 1;
    }
}

/* one iteration of surf_atlas_dilate at texel (x, y): a valid texel is copied; an invalid one with valid 8-neighbours
 * inside the image becomes their mean, summed from 0 in the order N, S, W, E, NW, NE, SW, SE */
SURF_HD void atlasDilate(const float4* rgba, const uint8_t* valid, int W, int H, int x, int y, float4& out, uint8_t& outValid) {
    const size_t q = (size_t)y * (size_t)W + (size_t)x;
    if (valid[q]) { out = rgba[q]; outValid = 1; return; }
    const int dx[8] = {0, 0, -1, 1, -1, 1, -1, 1}, dy[8] = {-1, 1, 0, 0, -1, -1, 1, 1};
    float r = 0.0f, g = 0.0f, b = 0.0f;
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int nx = x + dx[k], ny = y + dy[k];
        if (nx < 0 || ny < 0 || nx >= W || ny >= H) continue;
        const size_t p = (size_t)ny * (size_t)W + (size_t)nx;
        if (!valid[p]) continue;
        const float4 v = rgba[p];
        r = r + v.x; g = g + v.y; b = b + v.z;
        ++n;
    }
    if (n) { const float d = (float)n; out = make_float4(r / d, g / d, b / d, 1.0f); outValid = 1; }
    else { out = make_float4(0.0f, 0.0f, 0.0f, 0.0f); outValid = 0; }
}

#if defined(__HIPCC__) || defined(__HIP__)

/* what the build's kernels share */
struct AtlasArgs {
    const AtlasChart* charts;
    uint32_t nCharts, nKeys;       /* nKeys: the triangles of all charts */
    uint32_t W, H;
    const surf_triangle* tr;
    const surf_tri_extension* ext;
    const surf_gpu_instance* inst;
    const surf_material* mats;
    AtlasTri* tris;                /* [nKeys] */
    uint32_t* counts;              /* [nKeys + 1]: tiles per key, then their exclusive prefix sums */
    uint32_t* owner;               /* [W * H], ~0: empty */
    uint32_t* cover;               /* [W * H] */
    uint32_t* sums;                /* covered, overlapped, skipped, -, then the tiles' total as two words */
};

/* (a) one lane per key: the triangle in texel space, its tile count, the skipped triangles counted per wave */
static __global__ __launch_bounds__(kAtlasBlock) void k_atlas_setup(AtlasArgs a) {
    const uint32_t key = blockIdx.x * kAtlasBlock + threadIdx.x;
    bool skipped = false;
    if (key < a.nKeys) {
        const AtlasChart ch = a.charts[atlasChartOf(a.charts, a.nCharts, key)];
        const AtlasTri t = atlasTriangle(ch, a.ext[ch.tri0 + (key - ch.first)], (float)a.W, (float)a.H);
        a.tris[key] = t;
        a.counts[key] = atlasTileCount(t, a.W, a.H);
        skipped = t.skip != 0u;
    }
    const unsigned long long votes = __ballot(skipped);
    if ((threadIdx.x & 63u) == 0u && votes) atomicAdd(&a.sums[2], (uint32_t)__popcll(votes));
}

/* (a) one block of 1024 threads: counts[0 .. n) become their exclusive prefix sums, counts[n] the total; the total
 * also as 64 bits in sums[4..5], so the host sees a sum the 32-bit offsets cannot hold (k_compact_scan's pattern) */
static __global__ __launch_bounds__(1024) void k_atlas_scan(uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ sums) {
    __shared__ unsigned long long part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = n / 1024u + (n % 1024u ? 1u : 0u);
    const uint64_t a64 = (uint64_t)t * per;
    const uint32_t a = a64 < n ? (uint32_t)a64 : n, b = (uint64_t)a + per < n ? a + per : n;
    unsigned long long sum = 0;
    for (uint32_t k = a; k < b; ++k) sum += counts[k];
    part[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) {
        const unsigned long long v = t >= off ? part[t - off] : 0ull;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    unsigned long long run = part[t] - sum;
    for (uint32_t k = a; k < b; ++k) { const uint32_t c = counts[k]; counts[k] = (uint32_t)run; run += c; }
    if (t == 1023u) {
        const unsigned long long total = part[1023];
        counts[n] = (uint32_t)total;
        sums[4] = (uint32_t)total;
        sums[5] = (uint32_t)(total >> 32);
    }
}

/* a covered centre: the lowest key owns the texel, every covering triangle counts; both order-independent */
__device__ __forceinline__ void atlasMark(const AtlasArgs& a, const AtlasTri& t, uint32_t key, uint32_t x, uint32_t y) {
    if (!atlasCovers(t, (float)x + 0.5f, (float)y + 0.5f)) return;
    const size_t q = (size_t)y * a.W + x;
    atomicMin(&a.owner[q], key);
    atomicAdd(&a.cover[q], 1u);
}

/* (b) one wave per (triangle, tile) item, lane l at texel (l & 7, l >> 3) of the tile: the item's triangle by a
 * search of the prefix sums, wave-uniform, then three edge functions per lane */
static __global__ __launch_bounds__(kAtlasBlock) void k_atlas_cover(AtlasArgs a, uint32_t nItems) {
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t item = blockIdx.x * (kAtlasBlock / 64u) + wave;
    if (item >= nItems) return;
    uint32_t lo = 0u, hi = a.nKeys;          /* counts[lo] <= item < counts[hi] */
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a.counts[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t key = lo;
    const AtlasTri t = a.tris[key];
    uint32_t xa, xb, ya, yb;
    if (!atlasTexelBox(t, a.W, a.H, xa, xb, ya, yb)) return;   /* never: a key with items has a box */
    const uint32_t tx0 = xa / kAtlasTile, ntx = xb / kAtlasTile - tx0 + 1u, local = item - a.counts[key];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t x = (tx0 + local % ntx) * kAtlasTile + (lane & 7u), y = (ya / kAtlasTile + local / ntx) * kAtlasTile + (lane >> 3);
    if (x < a.W && y < a.H) atlasMark(a, t, key, x, y);
}

/* (b), the A/B baseline (SURF_ATLAS_MAP=0): one lane per triangle walks its clipped bounding box */
static __global__ __launch_bounds__(kAtlasBlock) void k_atlas_cover_tri(AtlasArgs a) {
    const uint32_t key = blockIdx.x * kAtlasBlock + threadIdx.x;
    if (key >= a.nKeys) return;
    const AtlasTri t = a.tris[key];
    uint32_t xa, xb, ya, yb;
    if (!atlasTexelBox(t, a.W, a.H, xa, xb, ya, yb)) return;
    for (uint32_t y = ya; y <= yb; ++y)
        for (uint32_t x = xa; x <= xb; ++x) atlasMark(a, t, key, x, y);
}

/* (c) one lane per texel: the owner's surfel into the planes the caller asked for, covered and overlapped counted per wave */
static __global__ __launch_bounds__(kAtlasBlock) void k_atlas_resolve(AtlasArgs a, float4* __restrict__ position, float4* __restrict__ normal,
                                                                      float4* __restrict__ albedo, uint4* __restrict__ ids) {
    const size_t npx = (size_t)a.W * a.H;
    const size_t q = (size_t)blockIdx.x * kAtlasBlock + threadIdx.x;
    uint32_t cover = 0u;
    if (q < npx) {
        cover = a.cover[q];
        const AtlasSurfel s = atlasResolve(a.charts, a.nCharts, a.tris, a.tr, a.ext, a.inst, a.mats, a.owner[q], cover,
                                           (uint32_t)(q % a.W), (uint32_t)(q / a.W));
        if (position) position[q] = s.position;
        if (normal) normal[q] = s.normal;
        if (albedo) albedo[q] = s.albedo;
        if (ids) ids[q] = s.ids;
    }
    const unsigned long long c1 = __ballot(cover >= 1u), c2 = __ballot(cover >= 2u);
    if ((threadIdx.x & 63u) == 0u) {
        if (c1) atomicAdd(&a.sums[0], (uint32_t)__popcll(c1));
        if (c2) atomicAdd(&a.sums[1], (uint32_t)__popcll(c2));
    }
}

/* surf_atlas_finish: one lane per texel */
static __global__ __launch_bounds__(kAtlasBlock) void k_atlas_finish(const float4* __restrict__ acc, const float4* __restrict__ alb, size_t npx,
                                                                     float4* __restrict__ out, uint8_t* __restrict__ valid) {
    const size_t q = (size_t)blockIdx.x * kAtlasBlock + threadIdx.x;
    if (q >= npx) return;
    float4 o;
    uint8_t v;
    atlasFinish(acc[q], alb[q], o, v);
    out[q] = o;
    valid[q] = v;
}

/* one iteration of surf_atlas_dilate: one lane per texel, a block a 32 x 8 tile */
static __global__ __launch_bounds__(kAtlasBlock) void k_atlas_dilate(const float4* __restrict__ rgba, const uint8_t* __restrict__ valid, int W, int H,
                                                                     float4* __restrict__ out, uint8_t* __restrict__ outValid) {
    const int x = (int)(blockIdx.x * 32u + (threadIdx.x & 31u)), y = (int)(blockIdx.y * 8u + (threadIdx.x >> 5));
    if (x >= W || y >= H) return;
    float4 o;
    uint8_t v;
    atlasDilate(rgba, valid, W, H, x, y, o, v);
    const size_t q = (size_t)y * (size_t)W + (size_t)x;
    out[q] = o;
    outValid[q] = v;
}

#endif  /* HIP */

}  // namespace surfdev
