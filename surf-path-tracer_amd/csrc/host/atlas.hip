/*
 * atlas.hip -- the light-map atlas (surf_atlas_*, include/surf_hip.h): the
 * checks and the chart table, the uploads of the caller's scene records into
 * buffers of this call's own, the launches of the rasterizer (setup, scan,
 * cover, resolve), of the finish and of the gutter fill, the copies out, and
 * the CPU twins.  The arithmetic lives in device/atlas_kernels.h.  Touches
 * nothing of the uploaded scene, the sample stream or the captured graph: the
 * context supplies the device, the stream and the timer.
 */
#include "host/filter_host.h"

#include <cmath>

#include "device/atlas_kernels.h"

namespace {

static_assert(sizeof(surf_atlas_chart) == 24, "a chart is 24 B");
static_assert(sizeof(surf_atlas_summary) == 16, "the summary is 16 B");
static_assert(sizeof(AtlasChart) == 48 && sizeof(AtlasTri) == 32, "the kernels' records");

/* device buffers of one call, freed when it returns (hipFree waits for the work that reads them) */
struct Scratch {
    std::vector<void*> list;
    ~Scratch() { freeList(list); }
    template <class T>
    int get(surf_ctx* c, T** out, size_t count) { return devAlloc(c, list, out, count); }
    template <class T>
    int put(surf_ctx* c, const T** out, const T* host, size_t count) {
        T* d = nullptr;
        const int rc = get(c, &d, count);
        if (rc) return rc;
        SURF_CHECK(c, hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
        *out = d;
        return SURF_OK;
    }
};

const char* sizeError(uint32_t W, uint32_t H) {
    if (W == 0 || H == 0) return "W or H is 0";
    if (W > kAtlasMaxSide || H > kAtlasMaxSide) return "W or H is above 16384";
    return nullptr;
}

/* The checks of a build and its chart table.  An instance's mesh is the triangles from its tri_offset up to the next
 * larger tri_offset among the instances, or triangle_count. */
int planAtlas(surf_ctx* c, const std::string& who, const surf_scene_desc* d, const surf_atlas_chart* charts, uint32_t n, uint32_t W, uint32_t H,
              std::vector<AtlasChart>& out) {
    if (const char* why = sizeError(W, H)) return fail(c, SURF_ERR_INVALID, who + ": " + why);
    if (!charts || n == 0) return fail(c, SURF_ERR_INVALID, who + ": no charts");
    if (!d || !d->triangles || !d->tri_ext || !d->instances || !d->materials || d->triangle_count == 0 || d->instance_count == 0 ||
        d->material_count == 0)
        return fail(c, SURF_ERR_INVALID, who + ": the desc or one of triangles, tri_ext, instances and materials is NULL or empty");
    std::vector<uint32_t> starts(d->instance_count);
    for (uint32_t i = 0; i < d->instance_count; ++i) starts[i] = d->instances[i].tri_offset;
    std::sort(starts.begin(), starts.end());
    out.resize(n);
    uint64_t first = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const surf_atlas_chart& ch = charts[k];
        const std::string what = who + ": chart " + std::to_string(k);
        if (ch.instance >= d->instance_count) return fail(c, SURF_ERR_INVALID, what + " names instance " + std::to_string(ch.instance) + " of " + std::to_string(d->instance_count));
        for (const float v : {ch.scale[0], ch.scale[1], ch.offset[0], ch.offset[1]})
            if (!std::isfinite(v)) return fail(c, SURF_ERR_INVALID, what + " has a scale or offset that is not finite");
        const surf_gpu_instance& g = d->instances[ch.instance];
        const float* m = g.transform;
        if (!(m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f))
            return fail(c, SURF_ERR_INVALID, what + ": row 3 of its instance's transform is not (0, 0, 0, 1)");
        if (g.tri_offset >= d->triangle_count || g.material_offset >= d->material_count)
            return fail(c, SURF_ERR_INVALID, what + ": its instance's offsets are out of range");
        const auto next = std::upper_bound(starts.begin(), starts.end(), g.tri_offset);
        const uint32_t end = next == starts.end() ? d->triangle_count : std::min(*next, d->triangle_count);
        AtlasChart& a = out[k];
        a = AtlasChart{};
        a.instance = ch.instance;
        a.flags = ch.flags;
        a.tri0 = g.tri_offset;
        a.triN = end - g.tri_offset;
        a.first = (uint32_t)first;
        a.material = g.material_offset;
        a.sx = ch.scale[0]; a.sy = ch.scale[1];
        a.ox = ch.offset[0]; a.oy = ch.offset[1];
        first += a.triN;
        if (first >= 0xFFFFFFFFull) return fail(c, SURF_ERR_LIMIT, who + ": the charts hold 2^32 - 1 triangles or more");
    }
    return SURF_OK;
}

uint32_t keysOf(const std::vector<AtlasChart>& charts) { return charts.back().first + charts.back().triN; }

/* The build on the device.  The planes are device pointers (any may be NULL); *sum is filled.  Stages 0..2 of the
 * context's timer: setup and scan, cover, resolve.  Waits. */
int runBuild(surf_ctx* c, Scratch& S, const surf_scene_desc* d, const std::vector<AtlasChart>& charts, uint32_t W, uint32_t H, float4* position,
             float4* normal, float4* albedo, uint4* ids, surf_atlas_summary* sum) {
    const size_t npx = (size_t)W * H;
    AtlasArgs a{};
    a.nCharts = (uint32_t)charts.size();
    a.nKeys = keysOf(charts);
    a.W = W;
    a.H = H;
    int rc;
    if ((rc = S.put(c, &a.charts, charts.data(), charts.size()))) return rc;
    if ((rc = S.put(c, &a.tr, d->triangles, d->triangle_count))) return rc;
    if ((rc = S.put(c, &a.ext, d->tri_ext, d->triangle_count))) return rc;
    if ((rc = S.put(c, &a.inst, d->instances, d->instance_count))) return rc;
    if ((rc = S.put(c, &a.mats, d->materials, d->material_count))) return rc;
    if ((rc = S.get(c, &a.tris, a.nKeys))) return rc;
    if ((rc = S.get(c, &a.counts, (size_t)a.nKeys + 1))) return rc;
    if ((rc = S.get(c, &a.owner, npx))) return rc;
    if ((rc = S.get(c, &a.cover, npx))) return rc;
    if ((rc = S.get(c, &a.sums, 8))) return rc;
    SURF_CHECK(c, hipMemsetAsync(a.owner, 0xFF, npx * sizeof(uint32_t), c->stream));
    SURF_CHECK(c, hipMemsetAsync(a.cover, 0, npx * sizeof(uint32_t), c->stream));
    SURF_CHECK(c, hipMemsetAsync(a.sums, 0, 8 * sizeof(uint32_t), c->stream));
    StageTimer<5>& T = c->atTime;
    const uint32_t keyBlocks = (a.nKeys + kAtlasBlock - 1) / kAtlasBlock;
    SURF_CHECK(c, T.mark(0, c->stream));
    hipLaunchKernelGGL(k_atlas_setup, dim3(keyBlocks), dim3(kAtlasBlock), 0, c->stream, a);
    SURF_CHECK(c, hipGetLastError());
    uint64_t items = 0;
    if (c->atlasTileMap) {
        /* the grid of the cover kernel is the number of items: one trip to the host, inside stage 0 */
        hipLaunchKernelGGL(k_atlas_scan, dim3(1), dim3(1024), 0, c->stream, a.counts, a.nKeys, a.sums);
        SURF_CHECK(c, hipGetLastError());
        SURF_CHECK(c, hipMemcpyAsync(&items, a.sums + 4, sizeof items, hipMemcpyDeviceToHost, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
    }
    SURF_CHECK(c, T.mark(1, c->stream));
    /* an expansion the 32-bit prefix sums cannot hold is walked per triangle: the same atomics, the same planes */
    const bool tiles = c->atlasTileMap && items <= 0xFFFFFFFFull;
    if (tiles && items) {
        const uint32_t perBlock = kAtlasBlock / 64u;
        hipLaunchKernelGGL(k_atlas_cover, dim3((uint32_t)((items + perBlock - 1) / perBlock)), dim3(kAtlasBlock), 0, c->stream, a, (uint32_t)items);
    } else if (!tiles) {
        hipLaunchKernelGGL(k_atlas_cover_tri, dim3(keyBlocks), dim3(kAtlasBlock), 0, c->stream, a);
    }
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, T.mark(2, c->stream));
    hipLaunchKernelGGL(k_atlas_resolve, dim3((uint32_t)((npx + kAtlasBlock - 1) / kAtlasBlock)), dim3(kAtlasBlock), 0, c->stream, a, position, normal,
                       albedo, ids);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, T.mark(3, c->stream));
    uint32_t sums[4] = {};
    SURF_CHECK(c, hipMemcpyAsync(sums, a.sums, sizeof sums, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    SURF_CHECK(c, T.collect(3));
    c->atTiles = tiles;
    if (sum) *sum = surf_atlas_summary{sums[0], sums[1], sums[2], a.nKeys};
    return SURF_OK;
}

dim3 texelGrid(size_t npx) { return dim3((uint32_t)((npx + kAtlasBlock - 1) / kAtlasBlock)); }

/* the finish on device planes: stage 3 of the timer.  Waits. */
int runFinish(surf_ctx* c, size_t npx, const float4* acc, const float4* alb, float4* out, uint8_t* valid) {
    StageTimer<5>& T = c->atTime;
    SURF_CHECK(c, T.mark(3, c->stream));
    hipLaunchKernelGGL(k_atlas_finish, texelGrid(npx), dim3(kAtlasBlock), 0, c->stream, acc, alb, npx, out, valid);
    SURF_CHECK(c, hipGetLastError());
    SURF_CHECK(c, T.mark(4, c->stream));
    SURF_CHECK(c, hipEventSynchronize(T.ev[4]));
    (void)hipEventElapsedTime(&T.ms[3], T.ev[3], T.ev[4]);
    return SURF_OK;
}

/* The gutter fill on device planes: the iterations queued back to back, each reading the buffer the last one wrote;
 * the last one writes the caller's.  One scratch pair from two iterations on.  Stage 4 of the timer.  Waits. */
int runDilate(surf_ctx* c, Scratch& S, uint32_t W, uint32_t H, const float4* rgba, const uint8_t* valid, uint32_t iterations, float4* out,
              uint8_t* outValid) {
    const size_t npx = (size_t)W * H;
    StageTimer<5>& T = c->atTime;
    float4* tmp = nullptr;
    uint8_t* tmpValid = nullptr;
    int rc;
    if (iterations >= 2) {
        if ((rc = S.get(c, &tmp, npx))) return rc;
        if ((rc = S.get(c, &tmpValid, npx))) return rc;
    }
    SURF_CHECK(c, T.mark(4, c->stream));
    if (iterations == 0) {
        SURF_CHECK(c, hipMemcpyAsync(out, rgba, npx * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
        SURF_CHECK(c, hipMemcpyAsync(outValid, valid, npx, hipMemcpyDeviceToDevice, c->stream));
    }
    const float4* src = rgba;
    const uint8_t* srcValid = valid;
    for (uint32_t i = 0; i < iterations; ++i) {
        /* the last iteration writes out, and the ones before it alternate so that it does not read out */
        const bool toOut = ((iterations - 1 - i) & 1u) == 0u;
        float4* dst = toOut ? out : tmp;
        uint8_t* dstValid = toOut ? outValid : tmpValid;
        hipLaunchKernelGGL(k_atlas_dilate, dim3((W + 31) / 32, (H + 7) / 8), dim3(kAtlasBlock), 0, c->stream, src, srcValid, (int)W, (int)H, dst,
                           dstValid);
        SURF_CHECK(c, hipGetLastError());
        src = dst;
        srcValid = dstValid;
    }
    SURF_CHECK(c, T.mark(5, c->stream));
    SURF_CHECK(c, hipEventSynchronize(T.ev[5]));
    (void)hipEventElapsedTime(&T.ms[4], T.ev[4], T.ev[5]);
    return SURF_OK;
}

const char* finishError(uint32_t W, uint32_t H, const void* acc, const void* alb, const void* out, const void* valid) {
    if (!acc || !alb || !out || !valid) return "NULL argument";
    return sizeError(W, H);
}

const char* dilateError(uint32_t W, uint32_t H, const void* rgba, const void* valid, uint32_t iterations, const void* out, const void* outValid) {
    if (!rgba || !valid || !out || !outValid) return "NULL argument";
    if (iterations > kAtlasMaxIterations) return "iterations outside 0..64";
    if (rgba == out || valid == outValid) return "an output is its own input";
    return sizeError(W, H);
}

/* the build with its planes on the host (kind: device to host) or on the device (kind: device to device: written in place) */
int build(surf_ctx* c, const char* name, const surf_scene_desc* d, const surf_atlas_chart* charts, uint32_t n, uint32_t W, uint32_t H, void* position,
          void* normal, void* albedo, void* ids, surf_atlas_summary* sum, bool onDevice) {
    if (!c) return SURF_ERR_INVALID;
    std::vector<AtlasChart> table;
    int rc = planAtlas(c, name, d, charts, n, W, H, table);
    if (rc) return rc;
    SURF_CHECK(c, hipSetDevice(c->device));
    Scratch S;
    void* host[4] = {position, normal, albedo, ids};
    float4* dev[4] = {};
    const size_t npx = (size_t)W * H;
    for (int k = 0; k < 4; ++k) {
        if (!host[k]) continue;
        if (onDevice) dev[k] = static_cast<float4*>(host[k]);
        else if ((rc = S.get(c, &dev[k], npx))) return rc;
    }
    if ((rc = runBuild(c, S, d, table, W, H, dev[0], dev[1], dev[2], reinterpret_cast<uint4*>(dev[3]), sum))) return rc;
    if (!onDevice) {
        for (int k = 0; k < 4; ++k)
            if (host[k]) SURF_CHECK(c, hipMemcpyAsync(host[k], dev[k], npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
        SURF_CHECK(c, hipStreamSynchronize(c->stream));
    }
    return SURF_OK;
}

void store16(void* plane, size_t q, const void* rec) {
    if (plane) std::memcpy(static_cast<char*>(plane) + 16 * q, rec, 16);
}

}  // namespace

void surfhost::freeAtlas(surf_ctx* c) { c->atTime.destroy(); }

extern "C" {

int surf_atlas_grid_charts(uint32_t n, const uint32_t* instances, uint32_t W, uint32_t H, uint32_t margin, surf_atlas_chart* out) {
    const char* why = !out ? "NULL argument" : n == 0 ? "no instances" : sizeError(W, H);
    if (why) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_atlas_grid_charts: ") + why);
    uint32_t g = 1;
    while ((uint64_t)g * g < n) ++g;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t col = i % g, row = i / g;
        const uint32_t lo[2] = {(uint32_t)((uint64_t)col * W / g), (uint32_t)((uint64_t)row * H / g)};
        const uint32_t hi[2] = {(uint32_t)((uint64_t)(col + 1) * W / g), (uint32_t)((uint64_t)(row + 1) * H / g)};
        const uint32_t side[2] = {W, H};
        surf_atlas_chart& ch = out[i];
        ch.instance = instances ? instances[i] : i;
        ch.flags = 0;
        for (int a = 0; a < 2; ++a) {
            if ((uint64_t)hi[a] <= (uint64_t)lo[a] + 2ull * margin)
                return fail(nullptr, SURF_ERR_INVALID, "surf_atlas_grid_charts: the margins leave nothing of a cell");
            ch.scale[a] = (float)(hi[a] - lo[a] - 2u * margin) / (float)side[a];
            ch.offset[a] = (float)(lo[a] + margin) / (float)side[a];
        }
    }
    return SURF_OK;
}

int surf_atlas_build(surf_ctx* c, const surf_scene_desc* d, const surf_atlas_chart* charts, uint32_t n, uint32_t W, uint32_t H, float* position,
                     float* normal, float* albedo, uint32_t* ids, surf_atlas_summary* sum) {
    return build(c, "surf_atlas_build", d, charts, n, W, H, position, normal, albedo, ids, sum, false);
}

int surf_atlas_build_device(surf_ctx* c, const surf_scene_desc* d, const surf_atlas_chart* charts, uint32_t n, uint32_t W, uint32_t H,
                            void* position, void* normal, void* albedo, void* ids, surf_atlas_summary* sum) {
    return build(c, "surf_atlas_build_device", d, charts, n, W, H, position, normal, albedo, ids, sum, true);
}

/* The CPU twin: the SURF_HD functions of device/atlas_kernels.h on host arrays; a triangle's candidates are the
 * texels of its clipped bounding box, as on the device. */
int surf_atlas_build_host(const surf_scene_desc* d, const surf_atlas_chart* charts, uint32_t n, uint32_t W, uint32_t H, float* position,
                          float* normal, float* albedo, uint32_t* ids, surf_atlas_summary* sum) {
    std::vector<AtlasChart> table;
    const int rc = planAtlas(nullptr, "surf_atlas_build_host", d, charts, n, W, H, table);
    if (rc) return rc;
    const uint32_t nKeys = keysOf(table);
    const size_t npx = (size_t)W * H;
    std::vector<AtlasTri> tris(nKeys);
    std::vector<uint32_t> owner(npx, kUnset), cover(npx, 0u);
    surf_atlas_summary s{0, 0, 0, nKeys};
    for (uint32_t key = 0; key < nKeys; ++key) {
        const AtlasChart& ch = table[atlasChartOf(table.data(), n, key)];
        const AtlasTri t = tris[key] = atlasTriangle(ch, d->tri_ext[ch.tri0 + (key - ch.first)], (float)W, (float)H);
        s.skipped_triangles += t.skip;
        uint32_t xa, xb, ya, yb;
        if (!atlasTexelBox(t, W, H, xa, xb, ya, yb)) continue;
        for (uint32_t y = ya; y <= yb; ++y)
            for (uint32_t x = xa; x <= xb; ++x) {
                if (!atlasCovers(t, (float)x + 0.5f, (float)y + 0.5f)) continue;
                const size_t q = (size_t)y * W + x;
                owner[q] = std::min(owner[q], key);
                ++cover[q];
            }
    }
    for (size_t q = 0; q < npx; ++q) {
        s.covered += cover[q] >= 1u;
        s.overlapped += cover[q] >= 2u;
        const AtlasSurfel r = atlasResolve(table.data(), n, tris.data(), d->triangles, d->tri_ext, d->instances, d->materials, owner[q], cover[q],
                                           (uint32_t)(q % W), (uint32_t)(q / W));
        store16(position, q, &r.position);
        store16(normal, q, &r.normal);
        store16(albedo, q, &r.albedo);
        store16(ids, q, &r.ids);
    }
    if (sum) *sum = s;
    return SURF_OK;
}

int surf_atlas_finish(surf_ctx* c, uint32_t W, uint32_t H, const float* acc, const float* albedo, float* out, uint8_t* valid) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = finishError(W, H, acc, albedo, out, valid)) return fail(c, SURF_ERR_INVALID, std::string("surf_atlas_finish: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    Scratch S;
    const size_t npx = (size_t)W * H;
    const float4 *dAcc = nullptr, *dAlb = nullptr;
    float4* dOut = nullptr;
    uint8_t* dValid = nullptr;
    int rc;
    if ((rc = S.put(c, &dAcc, reinterpret_cast<const float4*>(acc), npx))) return rc;
    if ((rc = S.put(c, &dAlb, reinterpret_cast<const float4*>(albedo), npx))) return rc;
    if ((rc = S.get(c, &dOut, npx))) return rc;
    if ((rc = S.get(c, &dValid, npx))) return rc;
    if ((rc = runFinish(c, npx, dAcc, dAlb, dOut, dValid))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, dOut, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(valid, dValid, npx, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_atlas_finish_device(surf_ctx* c, uint32_t W, uint32_t H, const void* acc, const void* albedo, void* out, void* valid) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = finishError(W, H, acc, albedo, out, valid)) return fail(c, SURF_ERR_INVALID, std::string("surf_atlas_finish_device: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    return runFinish(c, (size_t)W * H, static_cast<const float4*>(acc), static_cast<const float4*>(albedo), static_cast<float4*>(out),
                     static_cast<uint8_t*>(valid));
}

int surf_atlas_finish_host(uint32_t W, uint32_t H, const float* acc, const float* albedo, float* out, uint8_t* valid) {
    if (const char* why = finishError(W, H, acc, albedo, out, valid)) return fail(nullptr, SURF_ERR_INVALID, std::string("surf_atlas_finish_host: ") + why);
    const size_t npx = (size_t)W * H;
    const std::vector<float4> A = hostPlane(acc, npx), B = hostPlane(albedo, npx);
    for (size_t q = 0; q < npx; ++q) {
        float4 o;
        atlasFinish(A[q], B[q], o, valid[q]);
        store16(out, q, &o);
    }
    return SURF_OK;
}

int surf_atlas_dilate(surf_ctx* c, uint32_t W, uint32_t H, const float* rgba, const uint8_t* valid, uint32_t iterations, float* out,
                      uint8_t* outValid) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = dilateError(W, H, rgba, valid, iterations, out, outValid)) return fail(c, SURF_ERR_INVALID, std::string("surf_atlas_dilate: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    Scratch S;
    const size_t npx = (size_t)W * H;
    const float4* dIn = nullptr;
    const uint8_t* dValid = nullptr;
    float4* dOut = nullptr;
    uint8_t* dOutValid = nullptr;
    int rc;
    if ((rc = S.put(c, &dIn, reinterpret_cast<const float4*>(rgba), npx))) return rc;
    if ((rc = S.put(c, &dValid, valid, npx))) return rc;
    if ((rc = S.get(c, &dOut, npx))) return rc;
    if ((rc = S.get(c, &dOutValid, npx))) return rc;
    if ((rc = runDilate(c, S, W, H, dIn, dValid, iterations, dOut, dOutValid))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(out, dOut, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(outValid, dOutValid, npx, hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_atlas_dilate_device(surf_ctx* c, uint32_t W, uint32_t H, const void* rgba, const void* valid, uint32_t iterations, void* out,
                             void* outValid) {
    if (!c) return SURF_ERR_INVALID;
    if (const char* why = dilateError(W, H, rgba, valid, iterations, out, outValid))
        return fail(c, SURF_ERR_INVALID, std::string("surf_atlas_dilate_device: ") + why);
    SURF_CHECK(c, hipSetDevice(c->device));
    Scratch S;
    return runDilate(c, S, W, H, static_cast<const float4*>(rgba), static_cast<const uint8_t*>(valid), iterations, static_cast<float4*>(out),
                     static_cast<uint8_t*>(outValid));
}

int surf_atlas_dilate_host(uint32_t W, uint32_t H, const float* rgba, const uint8_t* valid, uint32_t iterations, float* out, uint8_t* outValid) {
    if (const char* why = dilateError(W, H, rgba, valid, iterations, out, outValid))
        return fail(nullptr, SURF_ERR_INVALID, std::string("surf_atlas_dilate_host: ") + why);
    const size_t npx = (size_t)W * H;
    std::vector<float4> A = hostPlane(rgba, npx), B(npx);
    std::vector<uint8_t> va(valid, valid + npx), vb(npx);
    for (uint32_t i = 0; i < iterations; ++i) {
        for (uint32_t y = 0; y < H; ++y)
            for (uint32_t x = 0; x < W; ++x) {
                const size_t q = (size_t)y * W + x;
                atlasDilate(A.data(), va.data(), (int)W, (int)H, (int)x, (int)y, B[q], vb[q]);
            }
        A.swap(B);
        va.swap(vb);
    }
    std::memcpy(out, A.data(), npx * sizeof(float4));
    std::memcpy(outValid, va.data(), npx);
    return SURF_OK;
}

/* The whole chain on buffers of this call's own, all on the context's device: build, the sensor set from the build's
 * planes (the library copies them), clear, render, the accumulator copied, the camera sensor back -- also when the
 * render failed -- then finish and dilate, and the copies out. */
int surf_atlas_bake(surf_ctx* c, const surf_scene_desc* d, const surf_atlas_chart* charts, uint32_t n, uint32_t frames, uint32_t first_sample,
                    uint32_t max_segments, uint32_t spp, uint32_t iterations, float* lightmap, uint8_t* valid, float* accumulator,
                    surf_atlas_summary* sum) {
    if (!c) return SURF_ERR_INVALID;
    const std::string who("surf_atlas_bake");
    if (!lightmap || !valid) return fail(c, SURF_ERR_INVALID, who + ": NULL argument");
    if (c->rows.size() != c->height)
        return fail(c, SURF_ERR_INVALID, who + " needs a context that owns every row of the frame: the context's width x height is the atlas");
    if (frames == 0 || spp == 0) return fail(c, SURF_ERR_INVALID, who + ": frames or samples per frame is 0");
    if (iterations > kAtlasMaxIterations) return fail(c, SURF_ERR_INVALID, who + ": iterations outside 0..64");
    const uint32_t W = c->width, H = c->height;
    std::vector<AtlasChart> table;
    int rc = planAtlas(c, who, d, charts, n, W, H, table);
    if (rc) return rc;
    SURF_CHECK(c, hipSetDevice(c->device));
    Scratch S;
    const size_t npx = (size_t)W * H;
    float4 *pos = nullptr, *nrm = nullptr, *alb = nullptr, *acc = nullptr, *lit = nullptr, *out = nullptr;
    uint8_t *litValid = nullptr, *outValid = nullptr;
    for (float4** p : {&pos, &nrm, &alb, &acc, &lit, &out})
        if ((rc = S.get(c, p, npx))) return rc;
    if ((rc = S.get(c, &litValid, npx))) return rc;
    if ((rc = S.get(c, &outValid, npx))) return rc;
    if ((rc = runBuild(c, S, d, table, W, H, pos, nrm, alb, nullptr, sum))) return rc;
    if ((rc = surf_set_surfel_sensor_device(c, pos, nrm))) return rc;
    rc = surf_clear_accumulator(c);
    if (!rc) rc = surf_render(c, frames, first_sample, max_segments, spp);
    if (!rc) rc = surf_copy_accumulator_device(c, acc);
    const std::string why = c->err;
    const int back = surf_set_surfel_sensor(c, nullptr, nullptr);
    if (rc) return fail(c, rc, why);
    if (back) return back;
    if ((rc = runFinish(c, npx, acc, alb, lit, litValid))) return rc;
    if ((rc = runDilate(c, S, W, H, lit, litValid, iterations, out, outValid))) return rc;
    SURF_CHECK(c, hipMemcpyAsync(lightmap, out, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipMemcpyAsync(valid, outValid, npx, hipMemcpyDeviceToHost, c->stream));
    if (accumulator) SURF_CHECK(c, hipMemcpyAsync(accumulator, acc, npx * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    return SURF_OK;
}

int surf_debug_atlas_time(surf_ctx* c, float* kernel_ms, uint32_t count, uint32_t* tile_map) {
    if (!c || !kernel_ms) return SURF_ERR_INVALID;
    c->atTime.read(kernel_ms, count);
    if (tile_map) *tile_map = c->atTiles ? 1u : 0u;
    return SURF_OK;
}

}  // extern "C"
