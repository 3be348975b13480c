/*
 * scene_upload.hip -- surf_upload_scene / surf_update_instances: validation
 * of the application's scene descriptor and its re-layout into the records
 * the kernels read (device/types.h).  Host code only: no kernel is included
 * or launched here.  Built with the kernels' floating-point flags: the world
 * boxes and records computed here are what the traversal consumes.
 */
#include "host/surf_ctx.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "device/surf_math.h"

namespace {

/* Walks every BLAS/TLAS from its root: validates indices (no kernel can
 * fault on a malformed scene), measures depth, and emits the device node
 * record that carries the children's boxes. */
struct TreeWalk {
    uint32_t depth = 0;
    bool ok = true;
    std::string why;
};

TreeWalk walkTree(const surf_bvh_node* nodes, uint32_t nodeCount, uint32_t offset, uint32_t idxCount, uint32_t idxOffset,
                  std::vector<float4>& out, std::vector<uint8_t>& leafSeen, std::vector<uint32_t>* owner = nullptr) {
    TreeWalk w;
    std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};
    size_t visits = 0;
    while (!st.empty()) {
        auto [local, dep] = st.back();
        st.pop_back();
        if (++visits > (size_t)nodeCount + 1 || dep > 4096) { w.ok = false; w.why = "BVH has a cycle"; return w; }
        const uint64_t g = (uint64_t)offset + local;
        if (g >= nodeCount) { w.ok = false; w.why = "BVH node index out of range"; return w; }
        const surf_bvh_node& n = nodes[g];
        float4* rec = &out[4 * g];
        if (owner) (*owner)[g] = offset;
        rec[0].w = u2f(n.left_first);
        rec[1].w = u2f(n.count);
        if (n.count != 0) {
            if ((uint64_t)idxOffset + n.left_first + n.count > idxCount) { w.ok = false; w.why = "BVH leaf range out of range"; return w; }
            for (uint32_t k = 0; k < n.count; ++k) leafSeen[idxOffset + n.left_first + k] = 1;
            w.depth = std::max(w.depth, dep);
            continue;
        }
        const uint64_t l = (uint64_t)offset + n.left_first;
        if (l + 1 >= nodeCount) { w.ok = false; w.why = "BVH child index out of range"; return w; }
        const surf_bvh_node& L = nodes[l];
        const surf_bvh_node& R = nodes[l + 1];
        rec[0] = make_float4(L.bb_min.x, L.bb_min.y, L.bb_min.z, rec[0].w);
        rec[1] = make_float4(L.bb_max.x, L.bb_max.y, L.bb_max.z, rec[1].w);
        rec[2] = make_float4(R.bb_min.x, R.bb_min.y, R.bb_min.z, 0.0f);
        rec[3] = make_float4(R.bb_max.x, R.bb_max.y, R.bb_max.z, 0.0f);
        st.push_back({n.left_first + 1, dep + 1});
        st.push_back({n.left_first, dep + 1});
    }
    return w;
}

constexpr uint64_t kLdsLightBlas = 20480;     /* k_connect's staged emitter BLAS (compact records + triangles), bytes at most */

/* Instance-dependent tables (GPUScene::update re-uploads exactly these,
 * scene.cpp:267-282): DevInstance + TraceInst per instance, the TLAS node
 * records and index array, the light list.  BLAS roots come from the upload. */
struct InstanceTables {
    std::vector<DevInstance> inst;
    std::vector<TraceInst> tinst;
    std::vector<float4> tnodes;
    std::vector<uint32_t> tidx;
    std::vector<uint2> lights;
    uint32_t tlasDepth = 0, tlasLeafCount = 0;
    uint32_t nHeavy = 0;
    float4 hvLo[3], hvHi[3];
    uint32_t hvInst[3] = {0, 0, 0};
    unsigned long long runHead = 0, runMember = 0;
    float cullRadius = FLT_MAX;
};

/* The heavy-instance boxes of the ray-order keys (kernel arguments). */
void setKeys(surf_ctx* c, DevScene& S, const InstanceTables& T) {
    c->heavyInst.assign(T.hvInst, T.hvInst + T.nHeavy);
    dropDerivedPlanes(c);                 /* the pixel classes and the plane passes follow the instances */
    S.nHeavy = T.nHeavy;
    for (uint32_t h = 0; h < 3; ++h) {
        S.hvLo[h] = h < T.nHeavy ? T.hvLo[h] : make_float4(0, 0, 0, 0);
        S.hvHi[h] = h < T.nHeavy ? T.hvHi[h] : make_float4(0, 0, 0, 0);
    }
    S.keyMode = T.nHeavy ? c->keyMode : 0u;
    S.runHead = c->leafRun ? T.runHead : 0ull;
    S.runMember = c->leafRun ? T.runMember : 0ull;
    S.cullRadius = T.cullRadius;
    /* the emitters' BLAS, when every light instance uses one BLAS and its
     * node records fit kLdsLightBlas bytes: k_connect stages them */
    S.sbNode0 = S.sbRecN = S.sbTri0 = S.sbTriN = 0u;
    S.sbRec = nullptr;
    if (c->ldsLightBlas && !T.lights.empty()) {
        bool one = true;
        const DevInstance* L0 = T.lights[0].x < T.inst.size() ? &T.inst[T.lights[0].x] : nullptr;
        for (const uint2& L : T.lights)
            one = one && L0 && L.x < T.inst.size() && T.inst[L.x].nodeOffset == L0->nodeOffset &&
                  T.inst[L.x].idxOffset == L0->idxOffset && T.inst[L.x].triOffset == L0->triOffset;
        const auto sb = one ? c->stagedBlas.find(L0->nodeOffset) : c->stagedBlas.end();
        /* 16-bit stack entries: every BLAS and TLAS node index below 65536 */
        const bool small = c->nBlasNodes < 65536u && T.tnodes.size() / 4 < 65536u;
        if (small && sb != c->stagedBlas.end() && sb->second.tri0 == L0->idxOffset) {
            S.sbNode0 = sb->first; S.sbRec = sb->second.rec; S.sbRecN = sb->second.recN;
            S.sbTri0 = sb->second.tri0; S.sbTriN = sb->second.triN;
        }
    }
}

int buildInstanceTables(surf_ctx* c, const surf_gpu_instance* instances, uint32_t n, const uint32_t* tlasIdx,
                        const surf_bvh_node* tlasNodes, uint32_t nTlas, const surf_light* lights, uint32_t nLights, InstanceTables& T) {
    auto affine = [](const float* m) { return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f; };
    T.inst.resize(n);
    T.tinst.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        const surf_gpu_instance& g = instances[i];
        const auto root = c->blasRoots.find(std::make_tuple(g.bvh_node_offset, g.bvh_idx_offset, g.tri_offset));
        if (root == c->blasRoots.end() || g.material_offset >= c->nMaterials)
            return fail(c, SURF_ERR_INVALID, "instance " + std::to_string(i) + ": offsets do not name an uploaded BLAS/material");
        DevInstance& D = T.inst[i];
        std::memcpy(D.Minv, g.inv_transform, sizeof D.Minv);
        std::memcpy(D.M, g.transform, sizeof D.M);
        D.triOffset = g.tri_offset; D.idxOffset = g.bvh_idx_offset; D.nodeOffset = g.bvh_node_offset; D.material = g.material_offset;
        D.area = g.area;
        /* row 3 of a column-major matrix: elements 3, 7, 11, 15 */
        D.affineInv = affine(g.inv_transform) ? 1u : 0u;
        D.affine = affine(g.transform) ? 1u : 0u;
        const float* m = D.Minv;
        TraceInst& R = T.tinst[i];
        R.m0 = make_float4(m[0], m[4], m[8], m[12]);
        R.m1 = make_float4(m[1], m[5], m[9], m[13]);
        R.m2 = make_float4(m[2], m[6], m[10], m[14]);
        R.m3 = make_float4(m[3], m[7], m[11], m[15]);
        R.meta = make_uint4(D.nodeOffset, D.idxOffset, D.affineInv, i);
        R.r0 = root->second[0]; R.r1 = root->second[1]; R.r2 = root->second[2]; R.r3 = root->second[3];
        /* conservative world box: the triangle bounds' corners mapped to world
         * space by the inverse of the M^-1 the traversal applies (inverted in
         * double, so the box matches the object-space rays whatever M says),
         * padded by 1e-4 of the box's coordinate magnitude times the matrix's
         * condition number (~1000x the float rounding of the ray transform,
         * slab terms and triangle test); not usable (never culls) for a
         * projective or singular M^-1 or non-finite bounds */
        R.wlo = make_float4(0, 0, 0, 0);
        R.whi = make_float4(0, 0, 0, 0);
        const auto bb = c->blasBounds.find(g.tri_offset);
        double A[3][3], t[3], B[3][3];      /* M^-1 = [A t; 0 1] (column-major input), B = A^-1 */
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 3; ++q) A[r][q] = (double)g.inv_transform[4 * q + r];
            t[r] = (double)g.inv_transform[12 + r];
        }
        const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                           A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
        if (bb != c->blasBounds.end() && D.affineInv && std::isfinite(det) && det != 0.0) {
            B[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det; B[0][1] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det;
            B[0][2] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det; B[1][0] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det;
            B[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det; B[1][2] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det;
            B[2][0] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det; B[2][1] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
            B[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
            double na = 0.0, nb = 0.0;
            for (int r = 0; r < 3; ++r)
                for (int q = 0; q < 3; ++q) { na += A[r][q] * A[r][q]; nb += B[r][q] * B[r][q]; }
            const double cond = std::sqrt(na * nb);
            double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
            for (int corner = 0; corner < 8; ++corner) {
                const double p[3] = {bb->second[(corner & 1) ? 3 : 0] - t[0], bb->second[(corner & 2) ? 4 : 1] - t[1],
                                     bb->second[(corner & 4) ? 5 : 2] - t[2]};
                for (int r = 0; r < 3; ++r) {
                    const double w = B[r][0] * p[0] + B[r][1] * p[1] + B[r][2] * p[2];
                    lo[r] = std::min(lo[r], w); hi[r] = std::max(hi[r], w);
                }
            }
            double mag = 0.0;
            for (int r = 0; r < 3; ++r) mag = std::max({mag, std::fabs(lo[r]), std::fabs(hi[r]), hi[r] - lo[r]});
            const double pad = 1e-4 * mag * std::max(1.0, cond) + 1e-6;
            bool ok = std::isfinite(mag) && mag < 1e30;
            float flo[3], fhi[3];
            for (int r = 0; r < 3; ++r) {
                flo[r] = (float)(lo[r] - pad); fhi[r] = (float)(hi[r] + pad);
                ok = ok && std::isfinite(flo[r]) && std::isfinite(fhi[r]);
            }
            if (ok) {
                R.wlo = make_float4(flo[0], flo[1], flo[2], 1.0f);
                R.whi = make_float4(fhi[0], fhi[1], fhi[2], 0.0f);
                /* the kernels' slab test of this box computes (b - o) * (1 / d) in f32: each term is off by
                 * up to 2^-23 (|b| + |o|) |1 / d|, and the pad gives pad |1 / d| of slack on the same axis.
                 * |b| <= mag <= 1e4 pad; an origin within 2^20 pad keeps the error below pad / 4.  Rays
                 * from farther away (at 1e17 from a unit box the three axes' terms differ by rounding
                 * alone, and the test rejects rays the reference's walk accepts) skip the cull. */
                T.cullRadius = std::min(T.cullRadius, (float)std::min(pad * 1048576.0, (double)FLT_MAX));
            }
        }
    }
    T.tnodes.assign((size_t)nTlas * 4, make_float4(0, 0, 0, 0));
    std::vector<uint8_t> tseen(n, 0);
    TreeWalk tw = walkTree(tlasNodes, nTlas, 0, n, 0, T.tnodes, tseen);
    if (!tw.ok) return fail(c, SURF_ERR_INVALID, "TLAS: " + tw.why);
    T.tlasDepth = tw.depth;
    T.tidx.assign(tlasIdx, tlasIdx + n);
    for (uint32_t v : T.tidx) if (v >= n) return fail(c, SURF_ERR_INVALID, "TLAS index out of range");
    T.tlasLeafCount = tlasNodes[0].count;        /* root leaf: wave-uniform instance loop */
    if (T.tlasLeafCount && tlasNodes[0].left_first != 0) T.tlasLeafCount = 0;   /* general path unless indices start at 0 */
    /* ray-order membership key: the (at most 3) instances of a single-leaf
     * TLAS with the largest BLASes (>= 64 triangles) and a usable world box */
    if (T.tlasLeafCount) {
        std::vector<std::pair<uint32_t, uint32_t>> big;     /* (triangles, instance) */
        for (uint32_t i = 0; i < n; ++i) {
            const auto it = c->blasSlots.find(instances[i].tri_offset);
            const uint32_t tris = it == c->blasSlots.end() ? 0u : it->second;
            if (tris >= 64 && T.tinst[i].wlo.w != 0.0f) big.push_back({tris, i});
        }
        std::stable_sort(big.begin(), big.end(), [](const auto& a, const auto& b) { return a.first > b.first; });
        for (size_t h = 0; h < big.size() && h < 3; ++h) {
            T.hvLo[h] = T.tinst[big[h].second].wlo;
            T.hvHi[h] = T.tinst[big[h].second].whi;
            T.hvInst[h] = big[h].second;
            T.nHeavy = (uint32_t)h + 1;
        }
    }
    /* leaf runs (DevScene::runHead): maximal sequences of consecutive TLAS
     * positions whose instances are affine root leaves of at most kLeafRunTris
     * triangles over one triangle range; a sequence longer than kLeafRunMax
     * (the lanes' bit mask) continues as another run, a lone position is none */
    if (T.tlasLeafCount && T.tlasLeafCount <= 64u) {
        auto runLeaf = [&](uint32_t k) {
            const TraceInst& R = T.tinst[T.tidx[k]];
            return R.meta.z != 0u && f2u(R.r1.w) >= 1u && f2u(R.r1.w) <= kLeafRunTris;
        };
        auto sameRange = [&](uint32_t k, uint32_t j) {
            const TraceInst &A = T.tinst[T.tidx[k]], &B = T.tinst[T.tidx[j]];
            return A.meta.y == B.meta.y && f2u(A.r0.w) == f2u(B.r0.w) && f2u(A.r1.w) == f2u(B.r1.w);
        };
        const uint32_t end = std::min(T.tlasLeafCount, kLeafRunPositions);
        for (uint32_t k = 0; k < end;) {
            uint32_t len = 0;
            if (runLeaf(k))
                for (len = 1; k + len < end && len < kLeafRunMax && runLeaf(k + len) && sameRange(k, k + len);) ++len;
            if (len >= kLeafRunMin) {
                T.runHead |= 1ull << k;
                for (uint32_t j = 0; j < len; ++j) T.runMember |= 1ull << (k + j);
            }
            k += std::max(len, 1u);
        }
    }
    T.lights.resize(nLights);
    for (uint32_t l = 0; l < nLights; ++l) {
        const surf_light& L = lights[l];
        if (L.light_instance_idx >= n || L.primitive_count == 0 ||
            (uint64_t)instances[L.light_instance_idx].tri_offset + L.primitive_count > c->nTriangles)
            return fail(c, SURF_ERR_INVALID, "light " + std::to_string(l) + " out of range");
        T.lights[l] = make_uint2(L.light_instance_idx, L.primitive_count);
    }
    return SURF_OK;
}

/* ---- surf_upload_scene, step by step ------------------------------------ */

/* Step 1: every BLAS an instance names, validated and walked from its root. */
struct BlasWalk {
    std::vector<float4> nodes;       /* the device node records, 4 float4 per BLAS node */
    std::vector<int64_t> idxTri;     /* index slot -> triangle offset of the mesh that owns it (-1: unreached) */
    std::vector<uint32_t> owner;     /* node -> BLAS node offset of its tree (kUnset: unreached) */
    uint32_t maxDepth = 0;
};
int walkBlases(surf_ctx* c, const surf_scene_desc* d, BlasWalk& B) {
    B.idxTri.assign(d->blas_index_count, -1);
    B.nodes.assign((size_t)d->blas_node_count * 4, make_float4(0, 0, 0, 0));
    B.owner.assign(d->blas_node_count, kUnset);
    std::vector<uint8_t> walked(d->blas_node_count, 0);
    for (uint32_t i = 0; i < d->instance_count; ++i) {
        const surf_gpu_instance& g = d->instances[i];
        if (g.tri_offset >= d->triangle_count || g.material_offset >= d->material_count ||
            g.bvh_node_offset >= d->blas_node_count || g.bvh_idx_offset >= d->blas_index_count)
            return fail(c, SURF_ERR_INVALID, "instance " + std::to_string(i) + " offsets out of range");
        if (walked[g.bvh_node_offset]) continue;
        std::vector<uint8_t> leaf(d->blas_index_count, 0);
        TreeWalk w = walkTree(d->blas_nodes, d->blas_node_count, g.bvh_node_offset, d->blas_index_count, g.bvh_idx_offset, B.nodes, leaf,
                              &B.owner);
        if (!w.ok) return fail(c, SURF_ERR_INVALID, "instance " + std::to_string(i) + ": " + w.why);
        B.maxDepth = std::max(B.maxDepth, w.depth);
        walked[g.bvh_node_offset] = 1;
        for (uint32_t k = 0; k < d->blas_index_count; ++k)
            if (leaf[k]) {
                if (B.idxTri[k] >= 0 && B.idxTri[k] != (int64_t)g.tri_offset) return fail(c, SURF_ERR_INVALID, "BLAS index range shared by two meshes");
                B.idxTri[k] = g.tri_offset;
            }
    }
    return SURF_OK;
}

/* Step 2: the compact form of every small BLAS (k_connect stages the
 * emitters' one, blasAnyStaged): its interior records in DFS order from the
 * root (record 0), each child an interior record index or a leaf's kLeafTagC |
 * count << 16 | leftFirst; and the span of its triangle slots.  By BLAS node
 * offset. */
struct CompactBlas { std::vector<float4> recs; uint32_t tri0, triN; };   /* records; index offset, triangle slots */
std::map<uint32_t, CompactBlas> compactBlases(const surf_scene_desc* d, const std::vector<float4>& nodes) {
    std::map<uint32_t, CompactBlas> compact;
    for (uint32_t i = 0; i < d->instance_count; ++i) {
        const uint32_t root = d->instances[i].bvh_node_offset;
        if (compact.count(root) || d->blas_nodes[root].count != 0) continue;
        std::vector<float4> recs;
        std::vector<uint32_t> order{root};                     /* interior nodes by record index */
        uint32_t slots = 0;
        bool ok = true;
        for (size_t k = 0; k < order.size() && ok; ++k) {
            const uint32_t g = order[k];
            const float4* r = &nodes[4 * (size_t)g];
            uint32_t ref[2];
            for (int ch = 0; ch < 2; ++ch) {
                const uint32_t cg = root + f2u(r[0].w) + (uint32_t)ch;
                const surf_bvh_node& q = d->blas_nodes[cg];
                if (q.count != 0) {
                    ok = ok && q.count < 32768u && q.left_first < 65536u;
                    ref[ch] = kLeafTagC | (q.count << 16) | (q.left_first & 0xffffu);
                    slots = std::max(slots, q.left_first + q.count);
                } else {
                    ok = ok && order.size() < 32768u;
                    ref[ch] = (uint32_t)order.size();
                    order.push_back(cg);
                }
            }
            recs.push_back(make_float4(r[0].x, r[0].y, r[0].z, u2f(ref[0])));
            recs.push_back(make_float4(r[1].x, r[1].y, r[1].z, u2f(ref[1])));
            recs.push_back(make_float4(r[2].x, r[2].y, r[2].z, 0.0f));
            recs.push_back(make_float4(r[3].x, r[3].y, r[3].z, 0.0f));
            ok = ok && (recs.size() / 4) * 64 + (uint64_t)slots * 48 <= kLdsLightBlas;
        }
        if (ok) compact[root] = CompactBlas{std::move(recs), d->instances[i].bvh_idx_offset, slots};
    }
    return compact;
}

/* Step 3: the triangle records, and per mesh (by triangle offset) the bounds
 * and the slot count buildInstanceTables needs. */
struct TriangleRecords {
    std::vector<float4> tris;        /* per BLAS index slot: (v0, prim), e1, e2 */
    std::vector<float4> normals;     /* per triangle: n0, n1, n2 */
    std::vector<float4> verts;       /* per triangle: v0, v1, v2, centroid */
    std::map<uint32_t, std::array<double, 6>> bounds;
    std::map<uint32_t, uint32_t> slots;
};
int triangleRecords(surf_ctx* c, const surf_scene_desc* d, const std::vector<int64_t>& idxTri, TriangleRecords& R) {
    /* BVH-ordered triangles: (v0, prim), e1 = v1 - v0, e2 = v2 - v0 (mesh.cpp:25-26) */
    std::vector<float4>& tris = R.tris;
    tris.assign((size_t)d->blas_index_count * 3, make_float4(0, 0, 0, 0));
    for (uint32_t k = 0; k < d->blas_index_count; ++k) {
        if (idxTri[k] < 0) continue;
        const uint64_t t = (uint64_t)idxTri[k] + d->blas_indices[k];
        if (t >= d->triangle_count) return fail(c, SURF_ERR_INVALID, "BLAS index " + std::to_string(k) + " out of range");
        const surf_triangle& T = d->triangles[t];
        tris[3 * (size_t)k + 0] = make_float4(T.v0.x, T.v0.y, T.v0.z, u2f(d->blas_indices[k]));
        tris[3 * (size_t)k + 1] = make_float4(T.v1.x - T.v0.x, T.v1.y - T.v0.y, T.v1.z - T.v0.z, 0.0f);
        tris[3 * (size_t)k + 2] = make_float4(T.v2.x - T.v0.x, T.v2.y - T.v0.y, T.v2.z - T.v0.z, 0.0f);
    }
    /* object-space bounds of each BLAS's triangles as the traversal sees them
     * (v0, v0 + e1, v0 + e2 of the slot records), for the world-box cull */
    for (uint32_t k = 0; k < d->blas_index_count; ++k) {
        if (idxTri[k] < 0) continue;
        ++R.slots[(uint32_t)idxTri[k]];
        auto it = R.bounds.emplace((uint32_t)idxTri[k], std::array<double, 6>{HUGE_VAL, HUGE_VAL, HUGE_VAL, -HUGE_VAL, -HUGE_VAL, -HUGE_VAL}).first;
        const float4 a = tris[3 * (size_t)k], e1 = tris[3 * (size_t)k + 1], e2 = tris[3 * (size_t)k + 2];
        const double v[3][3] = {{a.x, a.y, a.z}, {(double)a.x + e1.x, (double)a.y + e1.y, (double)a.z + e1.z},
                                {(double)a.x + e2.x, (double)a.y + e2.y, (double)a.z + e2.z}};
        for (const auto& p : v)
            for (int q = 0; q < 3; ++q) { it->second[q] = std::min(it->second[q], p[q]); it->second[3 + q] = std::max(it->second[3 + q], p[q]); }
    }
    std::vector<float4>&normals = R.normals, &verts = R.verts;
    normals.resize((size_t)d->triangle_count * 3);
    verts.resize((size_t)d->triangle_count * 4);
    for (uint32_t t = 0; t < d->triangle_count; ++t) {
        const surf_tri_extension& x = d->tri_ext[t];
        normals[3 * (size_t)t + 0] = make_float4(x.n0.x, x.n0.y, x.n0.z, 0.0f);
        normals[3 * (size_t)t + 1] = make_float4(x.n1.x, x.n1.y, x.n1.z, 0.0f);
        normals[3 * (size_t)t + 2] = make_float4(x.n2.x, x.n2.y, x.n2.z, 0.0f);
        const surf_triangle& T = d->triangles[t];
        verts[4 * (size_t)t + 0] = make_float4(T.v0.x, T.v0.y, T.v0.z, 0.0f);
        verts[4 * (size_t)t + 1] = make_float4(T.v1.x, T.v1.y, T.v1.z, 0.0f);
        verts[4 * (size_t)t + 2] = make_float4(T.v2.x, T.v2.y, T.v2.z, 0.0f);
        verts[4 * (size_t)t + 3] = make_float4(T.centroid.x, T.centroid.y, T.centroid.z, 0.0f);
    }
    return SURF_OK;
}

/* Step 4: two-level records for the wave walk (blasWalk2): W(g) = the records
 * of g and of its two children, each in the lanes-as-planes order (lane l of a
 * row = dword planeDword(l) of the 64-B record), 48 floats; a leaf's W holds
 * its own record.  192-B offsets are 32-bit buffer offsets: at most 22.3 M
 * nodes.  Empty when the scene has too many nodes or SURF_WALK2=0. */
std::vector<float> twoLevelRecords(const surf_scene_desc* d, const std::vector<float4>& nodes, const std::vector<uint32_t>& owner,
                                   const std::vector<float4>& tris) {
    std::vector<float> W;
    const bool walk2 = !(std::getenv("SURF_WALK2") && std::getenv("SURF_WALK2")[0] == '0');   /* A/B: 0 = one-level walk (read per upload) */
    if (walk2 && (uint64_t)d->blas_node_count * 192u < (1ull << 32)) {
        W.assign((size_t)d->blas_node_count * 48, 0.0f);
        /* lanes 14 / 15 of a row (unused by the wave walk): the row node's two
         * children as packed leaf references for the lane walk (blasTraceW):
         * kLeafTag | count << 24 | leftFirst, 0 when not a leaf or too large */
        auto packLeaf = [&](uint64_t m) -> uint32_t {
            const surf_bvh_node& q = d->blas_nodes[m];
            return (q.count != 0 && q.count < 128u && q.left_first < (1u << 24)) ? (kLeafTag | (q.count << 24) | q.left_first) : 0u;
        };
        auto putRec = [&](size_t g, size_t row, uint64_t src) {
            const float* r = reinterpret_cast<const float*>(&nodes[4 * src]);
            for (uint32_t l = 0; l < 14; ++l) {
                const uint32_t dw = l < 12u ? (l / 6u) * 8u + (l & 1u) * 4u + ((l % 6u) >> 1) : (l == 12u ? 3u : 7u);
                W[48 * g + 16 * row + l] = r[dw];
            }
            const surf_bvh_node& q = d->blas_nodes[src];
            if (q.count == 0 && owner[src] != kUnset) {
                W[48 * g + 16 * row + 14] = u2f(packLeaf((uint64_t)owner[src] + q.left_first));
                W[48 * g + 16 * row + 15] = u2f(packLeaf((uint64_t)owner[src] + q.left_first + 1));
            }
        };
        /* a leaf's W holds its own record in row 0 and, for <= kLeafInW
         * triangles, the triangles themselves (row j: lanes 0..2 v0, 3..5 e1,
         * 6..8 e2, 9 prim -- the BVH-ordered records of its index slots), so the
         * wave walk tests them from the record its visit loaded (leafWaveW) */
        std::map<uint32_t, uint32_t> idxOfNode;                      /* BLAS node offset -> index offset */
        for (uint32_t i = 0; i < d->instance_count; ++i) idxOfNode[d->instances[i].bvh_node_offset] = d->instances[i].bvh_idx_offset;
        for (uint32_t g = 0; g < d->blas_node_count; ++g) {
            if (owner[g] == kUnset) continue;
            putRec(g, 0, g);
            const surf_bvh_node& n = d->blas_nodes[g];
            if (n.count == 0) {
                putRec(g, 1, (uint64_t)owner[g] + n.left_first);
                putRec(g, 2, (uint64_t)owner[g] + n.left_first + 1);
            } else if (n.count <= kLeafInW) {
                const uint64_t slot0 = (uint64_t)idxOfNode[owner[g]] + n.left_first;
                for (uint32_t j = 0; j < n.count; ++j) {
                    const float4* t = &tris[3 * (slot0 + j)];
                    float* w = &W[48 * (size_t)g + 16 * j];
                    w[0] = t[0].x; w[1] = t[0].y; w[2] = t[0].z;
                    w[3] = t[1].x; w[4] = t[1].y; w[5] = t[1].z;
                    w[6] = t[2].x; w[7] = t[2].y; w[8] = t[2].z;
                    w[9] = t[0].w;
                }
            }
        }
    }
    return W;
}

/* Step 5: the tables on the device (c->sceneAllocs) and the descriptor S the
 * kernels get; c->stagedBlas names the uploaded compact BLASes. */
int uploadTables(surf_ctx* c, const surf_scene_desc* d, const std::vector<float4>& nodes, const std::vector<float>& W,
                 const TriangleRecords& R, const InstanceTables& IT, const std::map<uint32_t, CompactBlas>& compact, DevScene& S) {
    int rc;
    if ((rc = upload(c, nodes, &S.nodes))) return rc;
    if (!W.empty()) {
        if ((rc = upload(c, W, &S.wnodes))) return rc;
        S.nWnodes = d->blas_node_count;
        /* the lane traversal walks them too when the BVH cannot stay in the
         * caches (nodes + triangles past the 256 MB of MALL): one DRAM round
         * trip per two levels instead of one per level (SURF_LANEW=0|1: A/B) */
        const uint64_t bvhBytes = (uint64_t)d->blas_node_count * 64u + (uint64_t)d->blas_index_count * 48u;
        S.laneW = bvhBytes > (256ull << 20) ? 1u : 0u;
        if (const char* e = std::getenv("SURF_LANEW")) S.laneW = e[0] == '1' ? 1u : 0u;
    }
    std::vector<DevMaterial> mats(d->material_count);
    std::memcpy(mats.data(), d->materials, d->material_count * sizeof(DevMaterial));
    if ((rc = upload(c, R.tris, &S.tris))) return rc;
    if ((rc = upload(c, R.normals, &S.normals))) return rc;
    if ((rc = upload(c, R.verts, &S.verts))) return rc;
    if ((rc = upload(c, IT.tnodes, &S.tlasNodes))) return rc;
    if ((rc = upload(c, IT.tidx, &S.tlasIdx))) return rc;
    if ((rc = upload(c, IT.inst, &S.inst))) return rc;
    if ((rc = upload(c, IT.tinst, &S.tinst))) return rc;
    if ((rc = upload(c, mats, &S.mats))) return rc;
    if ((rc = upload(c, IT.lights, &S.lights))) return rc;
    c->stagedBlas.clear();
    for (const auto& kv : compact) {
        const float4* dR = nullptr;
        if ((rc = upload(c, kv.second.recs, &dR))) return rc;
        c->stagedBlas[kv.first] = surf_ctx::StagedBlas{dR, (uint32_t)(kv.second.recs.size() / 4), kv.second.tri0, kv.second.triN};
    }
    return SURF_OK;
}

}  // namespace

extern "C" {

int surf_upload_scene(surf_ctx* c, const surf_scene_desc* d) {
    if (!c || !d) return SURF_ERR_INVALID;
    if (d->triangle_count == 0 || !d->triangles || !d->tri_ext || !d->blas_indices || !d->blas_nodes || !d->materials ||
        !d->instances || d->instance_count == 0 || !d->tlas_indices || !d->tlas_nodes || d->tlas_node_count == 0 ||
        !d->background || d->material_count == 0 || d->blas_node_count == 0 || d->blas_index_count == 0 ||
        (d->light_count && !d->lights))
        return fail(c, SURF_ERR_INVALID, "incomplete scene descriptor");
    /* the kernels index records with 32-bit element offsets (16 floats per node,
     * 12 per BLAS index slot, 16 per triangle record) */
    if (d->blas_node_count >= (1u << 28) || d->blas_index_count >= (1u << 28) || d->triangle_count >= (1u << 28))
        return fail(c, SURF_ERR_LIMIT, "scene larger than 2^28 BVH nodes / index slots / triangles");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);
    if (rc) return rc;
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    destroyGraph(c);
    freeList(c->sceneAllocs);
    c->hasScene = false;

    BlasWalk B;
    if ((rc = walkBlases(c, d, B))) return rc;
    const std::map<uint32_t, CompactBlas> compact = compactBlases(d, B.nodes);
    TriangleRecords R;
    if ((rc = triangleRecords(c, d, B.idxTri, R))) return rc;
    /* what buildInstanceTables -- now and in surf_update_instances -- looks up per instance */
    c->nBlasNodes = d->blas_node_count;
    c->nTriangles = d->triangle_count;
    c->nMaterials = d->material_count;
    c->blasRoots.clear();
    for (uint32_t i = 0; i < d->instance_count; ++i) {
        const surf_gpu_instance& g = d->instances[i];
        const size_t r = 4 * (size_t)g.bvh_node_offset;
        c->blasRoots[std::make_tuple(g.bvh_node_offset, g.bvh_idx_offset, g.tri_offset)] = {B.nodes[r], B.nodes[r + 1], B.nodes[r + 2], B.nodes[r + 3]};
    }
    c->blasBounds = std::move(R.bounds);
    c->blasSlots = std::move(R.slots);
    InstanceTables IT;
    if ((rc = buildInstanceTables(c, d->instances, d->instance_count, d->tlas_indices, d->tlas_nodes, d->tlas_node_count, d->lights,
                                  d->light_count, IT)))
        return rc;
    const uint32_t depth = IT.tlasDepth + B.maxDepth + 1;
    if (depth > kMaxStack) return fail(c, SURF_ERR_LIMIT, "BVH too deep for the LDS traversal stack (" + std::to_string(depth) + " entries)");

    DevScene S{};
    if ((rc = uploadTables(c, d, B.nodes, twoLevelRecords(d, B.nodes, B.owner, R.tris), R, IT, compact, S))) return rc;
    S.nLights = d->light_count;
    S.nInst = d->instance_count;
    S.nMats = d->material_count;
    S.nodes4G = d->blas_node_count < (1u << 26) ? 1u : 0u;
    S.finiteBoxes = 1u;
    for (const float4& q : B.nodes)
        if (!(std::fabs(q.x) <= FLT_MAX && std::fabs(q.y) <= FLT_MAX && std::fabs(q.z) <= FLT_MAX)) { S.finiteBoxes = 0u; break; }
    S.tlasLeafCount = IT.tlasLeafCount;
    setKeys(c, S, IT);
    const surf_background& bg = *d->background;
    S.bgType = bg.type;
    S.bgColor[0] = bg.color.x; S.bgColor[1] = bg.color.y; S.bgColor[2] = bg.color.z;
    S.bgA[0] = bg.gradient_a.x; S.bgA[1] = bg.gradient_a.y; S.bgA[2] = bg.gradient_a.z;
    S.bgB[0] = bg.gradient_b.x; S.bgB[1] = bg.gradient_b.y; S.bgB[2] = bg.gradient_b.z;
    {
        /* ray-order cells (a sort key only: any value is correct, a stale box after refits too) */
        const surf_bvh_node& root = d->tlas_nodes[0];
        const float lo[3] = {root.bb_min.x, root.bb_min.y, root.bb_min.z}, hi[3] = {root.bb_max.x, root.bb_max.y, root.bb_max.z};
        for (int a = 0; a < 3; ++a) {
            const float ext = hi[a] - lo[a];
            const bool ok = std::isfinite(lo[a]) && std::isfinite(ext) && ext > 0.0f;
            S.cellLo[a] = ok ? lo[a] : 0.0f;
            S.cellScale[a] = ok ? 2.0f / ext : 0.0f;
        }
    }
    c->S = S;
    c->ldsTables = d->instance_count <= kLdsInst && d->instance_count <= kLdsTraceInst && d->material_count <= kLdsMats &&
                   d->light_count <= kLdsLights;
    c->stackDepth = depth;
    c->nInstances = d->instance_count;
    c->nLightsUp = d->light_count;
    c->tlasNodeCount = d->tlas_node_count;
    c->maxBlasDepth = B.maxDepth;
    c->instHost.assign(d->instances, d->instances + d->instance_count);
    c->tpHave = false;                /* another scene: the temporal history starts again */
    c->svHave = false;                /* ... and the luminance moments with it */
    c->hasScene = true;
    return SURF_OK;
}

int surf_update_instances(surf_ctx* c, const surf_gpu_instance* instances, uint32_t n, const uint32_t* tlasIdx,
                          const surf_bvh_node* tlasNodes, uint32_t nTlas, const surf_light* lights, uint32_t nLights) {
    if (!c || !instances || !tlasIdx || !tlasNodes || (nLights && !lights)) return SURF_ERR_INVALID;
    if (!c->hasScene) return fail(c, SURF_ERR_NO_SCENE, "no scene uploaded");
    if (n != c->nInstances || nTlas != c->tlasNodeCount || nLights != c->nLightsUp)
        return fail(c, SURF_ERR_INVALID, "instance/TLAS/light counts differ from the uploaded scene: use surf_upload_scene");
    SURF_CHECK(c, hipSetDevice(c->device));
    int rc = endStream(c);            /* in-flight paths belong to the old transforms */
    if (rc) return rc;
    InstanceTables IT;
    if ((rc = buildInstanceTables(c, instances, n, tlasIdx, tlasNodes, nTlas, lights, nLights, IT))) return rc;
    const uint32_t depth = IT.tlasDepth + c->maxBlasDepth + 1;
    if (depth > kMaxStack) return fail(c, SURF_ERR_LIMIT, "BVH too deep for the LDS traversal stack (" + std::to_string(depth) + " entries)");
    SURF_CHECK(c, hipStreamSynchronize(c->stream));
    auto put = [&](const void* dst, const void* src, size_t bytes) {
        return hipMemcpy(const_cast<void*>(dst), src, bytes, hipMemcpyHostToDevice);
    };
    SURF_CHECK(c, put(c->S.inst, IT.inst.data(), IT.inst.size() * sizeof(DevInstance)));
    SURF_CHECK(c, put(c->S.tinst, IT.tinst.data(), IT.tinst.size() * sizeof(TraceInst)));
    SURF_CHECK(c, put(c->S.tlasNodes, IT.tnodes.data(), IT.tnodes.size() * sizeof(float4)));
    SURF_CHECK(c, put(c->S.tlasIdx, IT.tidx.data(), IT.tidx.size() * sizeof(uint32_t)));
    if (nLights) SURF_CHECK(c, put(c->S.lights, IT.lights.data(), IT.lights.size() * sizeof(uint2)));
    c->S.tlasLeafCount = IT.tlasLeafCount;
    setKeys(c, c->S, IT);
    c->stackDepth = std::max(c->stackDepth, depth);
    c->instHost.assign(instances, instances + n);
    destroyGraph(c);                  /* kernel arguments carry the scene descriptor */
    return SURF_OK;
}

}  // extern "C"
