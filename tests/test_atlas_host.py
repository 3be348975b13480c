"""The light-map atlas on the CPU (include/surf_hip.h, "the light-map atlas"): a numpy restatement of the three stages --
the UV rasterizer to surfels, the finish, the gutter fill -- in f32, brute force per texel, held bit for bit against the
library's CPU twins (surf_atlas_build_host, surf_atlas_finish_host, surf_atlas_dilate_host).  tests/test_gpu_atlas.py holds
the device to the same restatement and to the twins.  The scenes are descs built from numpy record arrays: no BVH."""
import ctypes as C

import numpy as np
import pytest

import surf_amd

F = np.float32
U = np.uint32
UNSET = 0xFFFFFFFF


# ---- scenes from record arrays ---------------------------------------------------------------------------

def tri_records(pos, nrm, uv):
    """Triangle (n, 16) and TriExtension (n, 20) records from per-corner arrays in OBJ corner order a, b, c:
    pos, nrm (n, 3, 3), uv (n, 3, 2).  The record's pairing: a is (v1, n0, uv0), b is (v0, n1, uv1), c is (v2, n2, uv2)."""
    pos, nrm, uv = (np.asarray(a, F) for a in (pos, nrm, uv))
    n = len(pos)
    tris, ext = np.zeros((n, 16), F), np.zeros((n, 20), F)
    tris[:, 0:3], tris[:, 4:7], tris[:, 8:11] = pos[:, 1], pos[:, 0], pos[:, 2]
    ext[:, 0:3], ext[:, 4:7], ext[:, 8:11] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    ext[:, 12:14], ext[:, 14:16], ext[:, 16:18] = uv[:, 0], uv[:, 1], uv[:, 2]
    return tris, ext


def instance_records(rows):
    """GPUInstance records (n, 40) as uint32 words from (tri_offset, material, 4x4 row-major matrix) rows."""
    out = np.zeros((len(rows), 40), U)
    for i, (tri0, mat, M) in enumerate(rows):
        out[i, 0], out[i, 3] = tri0, mat
        out[i, 8:24] = np.asarray(M, F).T.reshape(16).view(U)          # glm column major
    return out


def material_records(rows):
    """Material records (n, 16) from (emission_strength, emission_colour, albedo) rows."""
    out = np.zeros((len(rows), 16), F)
    for i, (strength, colour, albedo) in enumerate(rows):
        out[i, 0], out[i, 3] = strength, 1.0
        out[i, 4:7], out[i, 8:11] = colour, albedo
    return out


class Case:
    """One atlas: the record arrays, the charts as (instance, flags, sx, sy, ox, oy) rows, the size."""

    def __init__(self, tris, ext, inst, mats, charts, W, H):
        self.tris, self.ext = np.ascontiguousarray(tris, F), np.ascontiguousarray(ext, F)
        self.inst, self.mats = np.ascontiguousarray(inst, U), np.ascontiguousarray(mats, F)
        self.charts, self.W, self.H = [tuple(c) for c in charts], W, H

    def desc(self) -> surf_amd.SceneDesc:
        d = surf_amd.SceneDesc()
        d.triangles, d.tri_ext, d.triangle_count = self.tris.ctypes.data, self.ext.ctypes.data, len(self.tris)
        d.instances, d.instance_count = self.inst.ctypes.data, len(self.inst)
        d.materials, d.material_count = self.mats.ctypes.data, len(self.mats)
        return d


IDENTITY = np.eye(4, dtype=F)
WHITE = [(0.0, (0, 0, 0), (0.75, 0.5, 0.25))]


def lift(uv, rng=None):
    """A curved surface over the uv triangles: positions and (unnormalised) normals per corner."""
    uv = np.asarray(uv, F)
    u, v = uv[..., 0], uv[..., 1]
    pos = np.stack([F(3) * u - F(1), F(2) * v + F(0.5) * u, u * v + F(0.25)], -1).astype(F)
    nrm = np.stack([F(0.3) * v - F(0.1), F(0.2) - F(0.3) * u, np.ones_like(u)], -1).astype(F)
    if rng is not None:
        nrm = (nrm + rng.uniform(-0.2, 0.2, nrm.shape)).astype(F)
    return pos, nrm


def uv_case(uv, W, H, charts=((0, 0, 1.0, 1.0, 0.0, 0.0),), M=IDENTITY, mats=WHITE, rng=None):
    pos, nrm = lift(uv, rng)
    tris, ext = tri_records(pos, nrm, uv)
    return Case(tris, ext, instance_records([(0, 0, M)]), material_records(mats), charts, W, H)


QUAD_UV = np.array([[(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 1), (0, 1)]], F)


def quad(W, H):
    return uv_case(QUAD_UV, W, H)


def jitter_grid(W=64, H=48, n=9):
    rng = np.random.default_rng(7)
    g = (np.arange(n + 1, dtype=F) / F(n)).astype(F)
    vu, vv = np.meshgrid(g, g)
    vu, vv = vu.copy(), vv.copy()
    vu[1:-1, 1:-1] += rng.uniform(-0.3 / n, 0.3 / n, (n - 1, n - 1)).astype(F)
    vv[1:-1, 1:-1] += rng.uniform(-0.3 / n, 0.3 / n, (n - 1, n - 1)).astype(F)
    P = np.stack([vu, vv], -1)
    uv = []
    for j in range(n):
        for i in range(n):
            a, b, c, d = P[j, i], P[j, i + 1], P[j + 1, i + 1], P[j + 1, i]
            uv += [(a, b, c), (a, c, d)] if (i + j) & 1 else [(a, b, d), (b, c, d)]
    return uv_case(np.array(uv, F), W, H)


FAN_CENTRE = (8, 8)


def fan(W=32, H=32, n=33):
    c = np.array([(FAN_CENTRE[0] + 0.5) / W, (FAN_CENTRE[1] + 0.5) / H], F)          # 8.5 / 32: on a texel centre, exactly
    ang = np.arange(n + 1) * (2 * np.pi / n)
    rim = np.stack([c[0] + 0.2 * np.cos(ang), c[1] + 0.2 * np.sin(ang)], -1).astype(F)
    rim[n] = rim[0]
    return uv_case(np.array([(c, rim[k], rim[k + 1]) for k in range(n)], F), W, H)


NAN = float("nan")
DEGENERATE = [[(0.25, 0.25), (0.25, 0.25), (0.75, 0.5)],   # zero area: det is exactly 0
              [(0.1, 0.1), (NAN, 0.5), (0.9, 0.2)]]      # a NaN uv


def edge_big(W=17, H=13):
    """UVs far outside [0,1], negative coordinates among them: the bounding box is clipped on every side."""
    return uv_case(np.array([[(-3.0, -2.0), (5.0, -1.0), (0.5, 0.9)]] + DEGENERATE, F), W, H)


def edge_small(W=17, H=13):
    """A sub-texel triangle that covers no centre, one that covers exactly one, and the two skipped ones."""
    t = lambda pts: [(x / W, y / H) for x, y in pts]
    return uv_case(np.array([t([(2.1, 2.1), (2.4, 2.15), (2.2, 2.4)]), t([(5.3, 5.2), (5.9, 5.4), (5.4, 5.9)])] + DEGENERATE, F), W, H)


def two_charts(W=32, H=32):
    c = quad(W, H)
    c.charts = [(0, 0, 0.5, 0.5, 0.125, 0.125), (0, 0, 0.5, 0.5, 0.375, 0.25)]
    return c


def dyadic_soup(mirrored, W=32, H=32, n=40):
    """Random triangles with uvs on a 1/64 grid, so that 1 - u is exact and the mirrored chart is the exact mirror image."""
    rng = np.random.default_rng(11)
    uv = (rng.integers(0, 65, (n, 3, 2)) / 64.0).astype(F)
    return uv_case(uv, W, H, charts=[(0, 0, -1.0, 1.0, 1.0, 0.0)] if mirrored else [(0, 0, 1.0, 1.0, 0.0, 0.0)])


def posed_matrix():
    """Anisotropic scale, shear and rotation, row 3 = (0, 0, 0, 1)."""
    a = 0.7
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    S = np.array([[2.0, 0.6, 0.0], [0.0, 0.5, -0.3], [0.0, 0.0, 3.0]])
    M = np.eye(4)
    M[:3, :3] = R @ S
    M[:3, 3] = (1.5, -2.0, 0.25)
    return M.astype(F)


def posed(W=23, H=19):
    return uv_case(QUAD_UV, W, H, charts=[(0, 1, 0.9, 0.8, 0.05, 0.1)], M=posed_matrix(), rng=np.random.default_rng(3))


def soup(W, H, n=500):
    """Random triangles with random uvs in two meshes: a diffuse instance and an emitter, a chart each."""
    rng = np.random.default_rng(5)
    c = rng.uniform(-0.1, 1.1, (n, 1, 2))
    uv = (c + rng.uniform(-0.15, 0.15, (n, 3, 2))).astype(F)
    pos, nrm = lift(uv, rng)
    tris, ext = tri_records(pos, nrm, uv)
    inst = instance_records([(0, 0, posed_matrix()), (n // 2, 1, IDENTITY)])
    mats = material_records(WHITE + [(5.0, (1.0, 0.8, 0.6), (0, 0, 0))])
    return Case(tris, ext, inst, mats, [(1, 0, 1.0, 1.0, 0.0, 0.0), (0, 1, 0.8, 0.9, 0.1, 0.05)], W, H)


CASES = {
    "quad-32x32": lambda: quad(32, 32), "quad-61x45": lambda: quad(61, 45), "jitter-grid-64x48": jitter_grid, "fan-33": fan,
    "edge-big-17x13": edge_big, "edge-small-17x13": edge_small, "two-charts": two_charts,
    "mirror-off": lambda: dyadic_soup(False), "mirror-on": lambda: dyadic_soup(True), "posed-flip": posed,
    "soup-37x29": lambda: soup(37, 29), "soup-128x128": lambda: soup(128, 128),
}


# ---- the restatement -------------------------------------------------------------------------------------

def np_mesh_range(inst, ntri, i):
    """An instance's mesh: from its tri_offset to the next larger tri_offset among the instances, or the end."""
    t0 = int(inst[i, 0])
    later = [int(t) for t in inst[:, 0] if int(t) > t0]
    return t0, min(min(later), ntri) if later else ntri


def np_edge(P, Q, cx, cy, det_positive):
    (px, py), (qx, qy) = P, Q
    swapped = qx < px or (qx == px and qy < py)
    if swapped:
        px, py, qx, qy = qx, qy, px, py
    e = (qx - px) * (cy - py) - (qy - py) * (cx - px)
    if swapped:
        e = -e
    if det_positive:
        e = -e
    return e


def np_mrow(M, i, x, y, z, w):
    return (M[0 + i] * x + M[4 + i] * y) + (M[8 + i] * z + M[12 + i] * w)


def np_atlas_build(case):
    """Section 1 of the header, texel by texel over the whole image: the four planes, the summary, and `onedge`, the
    texels where a covering triangle has an edge function that is exactly 0."""
    W, H = case.W, case.H
    Wf, Hf = F(W), F(H)
    cx, cy = np.meshgrid(np.arange(W, dtype=F) + F(0.5), np.arange(H, dtype=F) + F(0.5))
    owner = np.full((H, W), UNSET, U)
    cover = np.zeros((H, W), U)
    onedge = np.zeros((H, W), bool)
    position, normal, albedo = (np.zeros((H, W, 4), F) for _ in range(3))
    ids = np.zeros((H, W, 4), U)
    ids[..., :3] = UNSET
    skipped, first, keyed = 0, 0, []
    with np.errstate(all="ignore"):
        for k, (i, flags, sx, sy, ox, oy) in enumerate(case.charts):
            sx, sy, ox, oy = F(sx), F(sy), F(ox), F(oy)
            t0, t1 = np_mesh_range(case.inst, len(case.tris), i)
            for prim in range(t1 - t0):
                x = case.ext[t0 + prim]
                A, B, Cc = [((x[12 + 2 * j] * sx + ox) * Wf, (x[13 + 2 * j] * sy + oy) * Hf) for j in range(3)]
                det = (A[0] - B[0]) * (Cc[1] - B[1]) - (A[1] - B[1]) * (Cc[0] - B[0])
                keyed.append((k, i, flags, prim, t0 + prim, A, B, Cc))
                if not np.isfinite([*A, *B, *Cc]).all() or not np.isfinite(det) or det == 0:
                    skipped += 1
                    continue
                xs, ys = (A[0], B[0], Cc[0]), (A[1], B[1], Cc[1])
                inside = (cx >= min(xs) - F(1)) & (cx <= max(xs) + F(1)) & (cy >= min(ys) - F(1)) & (cy <= max(ys) + F(1))
                e = [np_edge(P, Q, cx, cy, det > 0) for P, Q in ((A, B), (B, Cc), (Cc, A))]
                cov = inside & (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
                onedge |= cov & ((e[0] == 0) | (e[1] == 0) | (e[2] == 0))
                owner[cov] = np.minimum(owner[cov], U(first + prim))
                cover[cov] += U(1)
            first += t1 - t0
        for key in np.unique(owner[owner != UNSET]):
            k, i, flags, prim, g, A, B, Cc = keyed[int(key)]
            m = owner == key
            c_x, c_y = cx[m], cy[m]
            e1x, e1y, e2x, e2y = A[0] - B[0], A[1] - B[1], Cc[0] - B[0], Cc[1] - B[1]
            qx, qy = c_x - B[0], c_y - B[1]
            det = e1x * e2y - e1y * e2x
            hu = (qx * e2y - qy * e2x) / det
            hv = (e1x * qy - e1y * qx) / det
            t, x = case.tris[g], case.ext[g]
            v0, v1, v2 = t[0:3], t[4:7], t[8:11]
            Po = [v0[a] + (hu * (v1[a] - v0[a]) + hv * (v2[a] - v0[a])) for a in range(3)]
            M = case.inst[i, 8:24].view(F)
            P = [np_mrow(M, r, Po[0], Po[1], Po[2], F(1)) for r in range(3)]
            w = (F(1) - hu) - hv
            n0, n1, n2 = x[0:3], x[4:7], x[8:11]
            no = [(hu * n0[a] + hv * n2[a]) + w * n1[a] for a in range(3)]
            n4 = [np_mrow(M, r, no[0], no[1], no[2], F(0)) for r in range(4)]
            nn = (n4[0] * n4[0] + n4[1] * n4[1]) + (n4[2] * n4[2] + n4[3] * n4[3])
            ninv = F(1) / np.sqrt(nn)
            N = np.stack([n4[a] * ninv for a in range(3)], -1)
            if flags & 1:
                N = -N
            N[~np.isfinite(N).all(-1)] = 0
            mat = case.mats[int(case.inst[i, 3])]
            light = mat[0] > 0 and (mat[4] > 0 or mat[5] > 0 or mat[6] > 0)
            position[m] = np.concatenate([np.stack(P, -1), np.ones((m.sum(), 1), F)], -1)
            normal[m] = np.concatenate([N, np.zeros((m.sum(), 1), F)], -1)
            albedo[m] = [*(mat[0] * mat[4:7]), 2.0] if light else [*mat[8:11], 1.0]
            ids[m, 0], ids[m, 1], ids[m, 2] = k, i, prim
    ids[..., 3] = cover
    summary = {"covered": int((cover >= 1).sum()), "overlapped": int((cover >= 2).sum()), "skipped_triangles": skipped, "triangles": first}
    return {"position": position, "normal": normal, "albedo": albedo, "ids": ids, "summary": summary, "onedge": onedge}


def np_atlas_finish(acc, alb):
    out, valid = np.zeros_like(acc), np.zeros(acc.shape[:2], np.uint8)
    with np.errstate(all="ignore"):
        lit = (acc[..., 3] > 0) & (alb[..., 3] == 1)
        out[lit, :3] = (acc[lit, :3] / acc[lit, 3:4]) * alb[lit, :3]
    emit = alb[..., 3] == 2
    out[emit, :3] = alb[emit, :3]
    out[lit | emit, 3] = 1
    valid[lit | emit] = 1
    return out, valid


NEIGHBOURS = ((0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))      # N, S, W, E, NW, NE, SW, SE as (dx, dy)


def np_atlas_dilate(rgba, valid, iterations):
    H, W = valid.shape
    a, v = rgba.copy(), valid.copy()
    for _ in range(iterations):
        b, vb = np.zeros_like(a), np.zeros_like(v)
        for y in range(H):
            for x in range(W):
                if v[y, x]:
                    b[y, x], vb[y, x] = a[y, x], 1
                    continue
                s, n = np.zeros(3, F), 0
                for dx, dy in NEIGHBOURS:
                    xx, yy = x + dx, y + dy
                    if 0 <= xx < W and 0 <= yy < H and v[yy, xx]:
                        s = s + a[yy, xx, :3]
                        n += 1
                if n:
                    b[y, x], vb[y, x] = [*(s / F(n)), 1.0], 1
        a, v = b, vb
    return a, v


# ---- comparisons -----------------------------------------------------------------------------------------

def assert_atlas_equal(got, want, what):
    for k in surf_amd.ATLAS_PLANES:
        g, w = np.ascontiguousarray(got[k]).view(U), np.ascontiguousarray(want[k]).view(U)
        assert g.shape == w.shape, f"{what}: {k} has shape {g.shape}, not {w.shape}"
        bad = np.argwhere((g != w).any(-1))
        assert len(bad) == 0, f"{what}: {k} differs at {len(bad)} texels, first (y, x) = {tuple(bad[0])}: {got[k][tuple(bad[0])]} != {want[k][tuple(bad[0])]}"
    assert got["summary"] == want["summary"], f"{what}: summary {got['summary']} != {want['summary']}"


_expected = {}


def expected(name):
    """(case, numpy's planes), computed once per case and shared with tests/test_gpu_atlas.py; never modified."""
    if name not in _expected:
        case = CASES[name]()
        want = np_atlas_build(case)
        for a in want.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _expected[name] = (case, want)
    return _expected[name]


def check_case_properties(name, case, got):
    """What each case is there to show, on planes that already equal numpy's."""
    W, H, s = case.W, case.H, got["summary"]
    cover, chart = got["ids"][..., 3], got["ids"][..., 0]
    want = _expected[name][1]
    if name.startswith("quad"):
        assert s["covered"] == W * H and s["skipped_triangles"] == 0 and s["triangles"] == 2
        if name == "quad-32x32":
            d = np.arange(32)
            assert (cover[d, d] == 2).all() and (got["ids"][d, d, 2] == 0).all() and s["overlapped"] == 32
    elif name == "jitter-grid-64x48":
        assert s["covered"] == W * H                                          # no cracks
        assert not ((cover >= 2) & ~want["onedge"]).any()
    elif name == "fan-33":
        x, y = FAN_CENTRE
        assert cover[y, x] == 33 and got["ids"][y, x, 2] == 0
        assert not ((cover >= 2) & ~want["onedge"]).any()
    elif name == "edge-big-17x13":
        assert s["skipped_triangles"] == 2 and 0 < s["covered"] < W * H and cover[0, 0] == 1 and cover[H - 1, W - 1] == 0
    elif name == "edge-small-17x13":
        assert s["skipped_triangles"] == 2 and s["covered"] == 1 and cover[5, 5] == 1 and got["ids"][5, 5, 2] == 1
    elif name == "two-charts":
        both = np.zeros((H, W), bool)
        both[8:20, 12:20] = True                                              # texels [4,20)^2 and [12,28) x [8,24) meet here
        assert (cover[both] >= 2).all() and (chart[both] == 0).all() and (chart[24:, :] == UNSET).all() and (chart[20:24, 12:28] == 1).all()
        assert s["overlapped"] == want["summary"]["overlapped"] >= both.sum()
    elif name == "posed-flip":
        n = got["normal"][cover >= 1][:, :3]
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max() < 1e-6
        assert s["covered"] > 0
    elif name.startswith("soup"):
        assert s["skipped_triangles"] == 0 and s["overlapped"] > 0 and (got["albedo"][..., 3] == 2).any() and (got["albedo"][..., 3] == 1).any()


# ---- 1. the rasterizer -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_build_host_equals_numpy(name):
    case, want = expected(name)
    got = surf_amd.atlas_build_host(case.desc(), case.charts, case.W, case.H)
    assert_atlas_equal(got, want, name)
    check_case_properties(name, case, got)
    empty = got["ids"][..., 3] == 0
    assert (got["normal"][empty].view(U) == 0).all() and (got["position"][empty].view(U) == 0).all()
    assert (got["ids"][empty][:, :3] == UNSET).all()


def assert_mirror_image(plain, mirrored, what):
    """The mirrored chart (scale -1, offset 1 in u) owns the mirror image of what its unmirrored twin owns, texel for
    texel, with the same cover counts and the same triangles."""
    a, b = plain["ids"][..., 3], mirrored["ids"][..., 3][:, ::-1]
    assert (a >= 1).any() and np.array_equal(a >= 1, b >= 1), f"{what}: the owned sets differ"
    assert np.array_equal(a, b), f"{what}: the cover counts differ"
    assert np.array_equal(plain["ids"][..., 2], mirrored["ids"][..., 2][:, ::-1]), f"{what}: the owners differ"
    assert plain["summary"] == mirrored["summary"]


def test_mirrored_chart_owns_the_mirror_image():
    (off, _), (on, _) = expected("mirror-off"), expected("mirror-on")
    plain = surf_amd.atlas_build_host(off.desc(), off.charts, off.W, off.H)
    mirrored = surf_amd.atlas_build_host(on.desc(), on.charts, on.W, on.H)
    assert_mirror_image(plain, mirrored, "the CPU twin")


def test_planes_may_be_null_and_unaligned():
    case, want = expected("soup-37x29")
    d, (arr, n) = case.desc(), surf_amd.atlas_chart_array(case.charts)
    raw = np.zeros(case.W * case.H * 16 + 4, np.uint8)
    s = surf_amd.AtlasSummary()
    rc = surf_amd.load().surf_atlas_build_host(C.byref(d), arr, n, case.W, case.H, None, raw[4:].ctypes.data, None, None, C.byref(s))
    assert rc == 0 and s.as_dict() == want["summary"]
    assert np.array_equal(raw[4:].view(U).reshape(case.H, case.W, 4), want["normal"].view(U))


def test_bundled_meshes_carry_uvs_and_bake_planes():
    """The bundled room through grid charts: the planes are the surfel sensor's, every owned texel has a unit normal."""
    scene = surf_amd.Scene.indoor()
    try:
        n = scene.desc().instance_count
        charts = surf_amd.atlas_grid_charts(n, 64, 64, 1)
        got = surf_amd.atlas_build_host(scene, charts, 64, 64)
    finally:
        scene.close()
    s, owned = got["summary"], got["ids"][..., 3] >= 1
    assert s["triangles"] == 6 * 2 + 2 * 188 + 2 * 15744 + 960 and s["covered"] == owned.sum() >= 6 * 14 * 14
    nn = np.linalg.norm(got["normal"][owned][:, :3].astype(np.float64), axis=1)
    assert np.abs(nn - 1).max() < 1e-5 and (got["albedo"][..., 3] == 2).any()


# ---- 2. finish -------------------------------------------------------------------------------------------

def finish_planes(W=19, H=13):
    rng = np.random.default_rng(2)
    acc = rng.uniform(0, 40, (H, W, 4)).astype(F)
    acc[..., 3] = rng.integers(0, 4, (H, W)) * F(4)                   # w == 0 among them
    acc[acc[..., 3] == 0] = 0
    alb = rng.uniform(0, 1, (H, W, 4)).astype(F)
    alb[..., 3] = rng.integers(0, 3, (H, W))                          # empty, surface, emitter
    alb[alb[..., 3] == 0] = 0
    return acc, alb


def test_finish_host_equals_numpy():
    acc, alb = finish_planes()
    want, want_valid = np_atlas_finish(acc, alb)
    got, valid = surf_amd.atlas_finish_host(acc, alb)
    assert np.array_equal(got.view(U), want.view(U)) and np.array_equal(valid, want_valid)
    for kind in ((alb[..., 3] == 2), (alb[..., 3] == 1) & (acc[..., 3] == 0), (alb[..., 3] == 0)):
        assert kind.any()
    assert (valid[alb[..., 3] == 2] == 1).all() and (valid[(alb[..., 3] == 1) & (acc[..., 3] == 0)] == 0).all()


# ---- 3. dilate -------------------------------------------------------------------------------------------

def dilate_planes(W=19, H=13):
    """Islands and holes: two blobs, a lone texel, a hole inside a blob, wide gutters around them."""
    rng = np.random.default_rng(4)
    valid = np.zeros((H, W), np.uint8)
    valid[1:5, 1:6] = 1
    valid[2, 3] = 0
    valid[7:12, 9:17] = 1
    valid[9:11, 12:14] = 0
    valid[11, 2] = 1
    rgba = rng.uniform(0, 2, (H, W, 4)).astype(F)
    rgba[..., 3] = 1
    rgba[valid == 0] = 0
    return rgba, valid


DILATE_ITERATIONS = (0, 1, 3, 64)
_dilated = {}


def dilate_expected(iterations):
    if iterations not in _dilated:
        _dilated[iterations] = np_atlas_dilate(*dilate_planes(), iterations)
    return _dilated[iterations]


@pytest.mark.parametrize("iterations", DILATE_ITERATIONS)
def test_dilate_host_equals_numpy(iterations):
    rgba, valid = dilate_planes()
    want, want_valid = dilate_expected(iterations)
    got, got_valid = surf_amd.atlas_dilate_host(rgba, valid, iterations)
    assert np.array_equal(got.view(U), want.view(U)) and np.array_equal(got_valid, want_valid)
    if iterations == 0:
        assert np.array_equal(got.view(U), rgba.view(U))
    if iterations == 64:
        assert got_valid.all()
    assert np.array_equal(got[valid == 1].view(U), rgba[valid == 1].view(U))        # a valid texel is copied


@pytest.mark.parametrize("fill", [0, 1])
def test_dilate_host_leaves_uniform_masks_alone(fill):
    rgba, _ = dilate_planes()
    valid = np.full(rgba.shape[:2], fill, np.uint8)
    if not fill:
        rgba = np.zeros_like(rgba)
    got, got_valid = surf_amd.atlas_dilate_host(rgba, valid, 3)
    assert np.array_equal(got.view(U), rgba.view(U)) and np.array_equal(got_valid, valid)
