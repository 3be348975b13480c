"""Caller-built scenes: their definitions, ray sets and CPU conditions.

Every GPU parity test used to trace the bundled room or one of its three
variants.  The scenes below are built in numpy, go through
oracle.OracleScene.custom (orc_scene_create_custom: the reference's own steps
on caller buffers) and reach the branches of the host re-layout
(csrc/host/scene_upload.hip) that the room never takes.
tests/test_gpu_custom_scenes.py imports them and compares the kernels with the
oracle bit for bit; this file pins, on the CPU alone, what those tests stand on:

  * the new oracle entry rebuilds the bundled room byte for byte;
  * ExportedScene (the product side: a scene descriptor over the oracle's ten
    exported buffers) describes what the oracle exported;
  * what the reference's walk guarantees against brute force on every scene's
    rays, and the pinned number of rays on which the two differ (not on C-nan:
    a NaN has no brute-force answer);
  * each scene reaches the re-layout branch it is named for, every instance is
    the closest hit of at least 20 rays, 20 % - 80 % of the silhouette rays hit,
    and at least 50 rays tie on t in the duplicates scene.

Scenes (instance counts include A's / B's enclosure, see enclosed()):

  A      19 instances of one 512-triangle sphere under 16 matrix classes in a
         single-leaf TLAS: identity, skew rotation, scale (0.05, 1, 20), shear,
         mirror, translate 1e4 * scale 1e-2, scale 1e3, condition 1e6,
         w = 2, a projective row (0, 0, 0.01, 1), two whose f32 inverse has an
         inexact row 3 (divide path, never culled), ...
  A2     (A') the same 16 without the enclosure: the TLAS splits.
  Aalt   A's meshes and counts under other matrices (the re-upload target).
  B1     root leaves of 1, 2, 3, 4, 127, 128, 200 triangles, a mesh whose child
         leaves hold 1..40, 127, 128 and 130 triangles (packLeaf, which only
         sees the children of interior nodes, gives up at 128), and 40
         consecutive plane copies at TLAS positions 11..50 (a leaf run of 32
         and one of 8).
  B2     the same with a projective plane copy in the middle (runs of 17 and 22).
  B64    64 instances in one TLAS leaf: LDS tables; planes at 11..63, runs of
         32 and 20 up to position 62, position 63 outside (kLeafRunPositions).
  B65    65 instances: global tables, no runs; planes at 11..64.
  C      zero-area triangles among good ones, a sphere doubled onto itself,
         a flat axis-aligned grid, a mesh at coordinates of 1e18 and one of 1e-18.
  Cnan   C's soup with one NaN vertex: non-finite node boxes.
  Ddeep  a BLAS of depth 101 (stack 102 > 64: no wave engine).
  Dtoo   a BLAS of depth 121 (stack 122 > 120: the upload is refused).
  E0/E1  a 34,676-triangle soup last, single-triangle fillers before it:
         65,534 and 65,536 BLAS nodes.  A node total is always even (a BLAS
         uses 2 + 2 * splits nodes, bvh.cpp:77), so 65,535 cannot be built;
         these two are the two sides of the `< 65536` selections.
  L1     A2's geometry with one small emitter mesh instanced twice (staged).
  L2     two emitters over different meshes, one projective (not staged).
  L1c/L2c  L1 and L2 inside A's scale-1e3 mirror sphere: no path sees the sky, so
         paths are still in flight when a replay ends and the drains take them.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle
import surf_amd

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
UNSET = 0xFFFFFFFF
F = np.float32
ASSETS = oracle.ASSETS_DIR

# device/types.h and host/surf_ctx.h: the thresholds the scenes straddle
K_LEAF_IN_W, K_PACK_LEAF, K_RUN_MAX, K_RUN_POSITIONS, K_LDS_TABLES, K_SK16, K_WAVE_STACK, K_MAX_STACK = 3, 128, 32, 63, 64, 65536, 64, 120


# ---- matrices (mathematical layout M[row][column], float64 until cast) ---------

def T(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def Sc(x, y=None, z=None):
    y, z = (x, x) if y is None else (y, z)
    return np.diag([x, y, z, 1.0])


def Rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    m = np.eye(4)
    m[:3, :3] = c * np.eye(3) + s * K + (1 - c) * np.outer(a, a)
    return m


def Shear(xy=0.0, xz=0.0, yz=0.0):
    m = np.eye(4)
    m[0, 1], m[0, 2], m[1, 2] = xy, xz, yz
    return m


def Row3(m, row):
    m = m.copy()
    m[3] = row
    return m


def f32(m):
    return np.asarray(m, np.float64).astype(np.float32)


# ---- meshes: (vertices (n, 3, 3), normals (n, 3, 3)) float32 --------------------

def face_normals(V):
    V = np.asarray(V, np.float64)
    with np.errstate(all="ignore"):
        n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0])
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
    n = np.where(np.isfinite(n), n, [0.0, 1.0, 0.0])
    return np.repeat(n[:, None, :], 3, axis=1).astype(np.float32)


def octa(level):
    """A unit sphere from an octahedron subdivided `level` times (8 * 4^level
    triangles); the six axis vertices stay exactly +-1, so its box is [-1, 1]^3."""
    ax = np.eye(3)
    tris = [(sx * ax[0], sy * ax[1], sz * ax[2]) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    for _ in range(level):
        nxt = []
        for a, b, c in tris:
            ab, bc, ca = ((a + b) / np.linalg.norm(a + b), (b + c) / np.linalg.norm(b + c), (c + a) / np.linalg.norm(c + a))
            nxt += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        tris = nxt
    V = np.array(tris, np.float64)
    return V.astype(np.float32), V.astype(np.float32)      # a unit sphere's normals are its points


def soup(seed, n, size, spread=1.0):
    r = np.random.default_rng(seed)
    V = (r.uniform(-spread, spread, (n, 1, 3)) + r.normal(size=(n, 3, 3)) * size).astype(np.float32)
    return V, face_normals(V)


def fan(seed, n):
    """n triangles whose stored centroid is exactly (0, 0, 0): v2 = -(v0 + v1) in
    f32, so (v0 + v1 + v2) * 0.333f is zero on every axis, no axis has two keys
    and BvhBLAS::build leaves one root leaf of n triangles."""
    r = np.random.default_rng(seed)
    v0 = (r.normal(size=(n, 3)) * r.uniform(0.3, 1.0, (n, 1))).astype(np.float32)
    v1 = (r.normal(size=(n, 3)) * r.uniform(0.3, 1.0, (n, 1))).astype(np.float32)
    V = np.stack([v0, v1, -(v0 + v1)], axis=1).astype(np.float32)
    return V, face_normals(V)


def clusters(seed, sizes):
    """An ordinary mesh with mixed leaf sizes: group g is a fan of sizes[g] triangles
    around its own lattice point.  Vertices are multiples of 2^-6 below 2 and the
    lattice points are integers, so every sum is exact, the centroids of a group
    are equal bit for bit and the builder separates the groups but never splits
    one: the leaves are the groups."""
    r = np.random.default_rng(seed)
    out = []
    for g, n in enumerate(sizes):
        v0 = np.round(r.uniform(-1.0, 1.0, (n, 3)) * 64) / 64
        v1 = np.round(r.uniform(-1.0, 1.0, (n, 3)) * 64) / 64
        c = np.array([3 * (g % 3) - 3, 3 * ((g // 3) % 3) - 3, 3 * (g // 9) - 3], np.float64)
        out.append(np.stack([v0 + c, v1 + c, -(v0 + v1) + c], axis=1))
    V = np.concatenate(out).astype(np.float32)
    return V, face_normals(V)


def obj(name):
    t, e = oracle.obj_load(os.path.join(ASSETS, name + ".obj.gz"))
    return (np.ascontiguousarray(t.reshape(-1, 4, 4)[:, :3, :3]), np.ascontiguousarray(e[:, :12].reshape(-1, 3, 4)[:, :, :3]),
            np.ascontiguousarray(e[:, 12:18]))


def plane2():
    v, n, _ = obj("plane")
    return v, n


def grid(n):
    """A flat grid of 2 n^2 triangles in the plane y = 0 over [-1, 1]^2: zero-extent boxes."""
    x = np.linspace(-1.0, 1.0, n + 1)
    tris = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = (x[i], 0, x[j]), (x[i + 1], 0, x[j]), (x[i + 1], 0, x[j + 1]), (x[i], 0, x[j + 1])
            tris += [(a, b, c), (a, c, d)]
    V = np.array(tris, np.float32)
    N = np.zeros_like(V)
    N[..., 1] = 1.0
    return V, N


def with_zero_area(seed, n, every=5):
    """A soup in which every `every`-th triangle has no area: two equal vertices,
    three equal vertices, or three collinear ones."""
    V, _ = soup(seed, n, 0.15)
    for k in range(0, n, every):
        kind = (k // every) % 3
        if kind == 0:
            V[k, 2] = V[k, 1]
        elif kind == 1:
            V[k, 1] = V[k, 0]
            V[k, 2] = V[k, 0]
        else:
            V[k, 2] = V[k, 0] + F(2.0) * (V[k, 1] - V[k, 0])
    return V, face_normals(V)


def plates(n1, n2, n3, ratio=8.5, grow=1.04):
    """Nested plates that the binned SAH peels one per level: plate k is a
    triangle of size grow^k in a plane x = x0 * ratio^j (then y, then z, for the
    smaller ones), its other two centroid keys exactly zero.  With ratio > 8 the
    plate with the largest key is alone in bin 7 and all others are in bin 0, so
    the only split offered takes one plate off; it pays, since the rest's box
    is smaller.  Keys stay above FLT_MIN (splitPlane's `hi` starts there,
    bvh.cpp:303-304) and the area below FLT_MAX, which bounds one axis to
    about 75 plates: depth = n1 + n2 + n3 - 1."""
    tris, k = [], 0
    for j in range(n3):
        h, z = grow ** k, 2.0 ** -124 * ratio ** j
        tris.append([(-h, -h, z), (h, -h, z), (0, 2 * h, z)])
        k += 1
    for j in range(n2):
        h, y = grow ** k, 2.0 ** -124 * ratio ** j
        tris.append([(-h, y, -h), (h, y, -h), (0, y, 2 * h)])
        k += 1
    for j in range(n1):
        h, x = grow ** k, 2.0 ** -120 * ratio ** j
        tris.append([(x, -h, -h), (x, h, -h), (x, 0, 2 * h)])
        k += 1
    V = np.array(tris, np.float64).astype(np.float32)
    return V, face_normals(V)


# ---- materials ----------------------------------------------------------------

GREY = {"albedo": (0.7, 0.7, 0.7)}
RED = {"albedo": (0.9, 0.2, 0.2)}
MIRROR = {"albedo": (0.9, 0.9, 0.9), "refl": 0.9}
GLASS = {"albedo": (0.9, 0.9, 0.9), "refr": 1.0, "ior": 1.4, "absorption": (0.02, 0.03, 0.02)}
LAMP = {"emit": 6.0, "emit_color": (1.0, 0.9, 0.7)}
LAMP2 = {"emit": 4.0, "emit_color": (0.4, 0.6, 1.0)}
MATERIALS = [GREY, RED, MIRROR, GLASS, LAMP]      # scenes A and B light one instance with the last
SKY = {"type": 1, "a": (0.8, 0.8, 0.8), "b": (0.1, 0.4, 0.6)}

BIG = 16384.0            # the enclosure's scale, a power of two
TINY = 2.0 ** -7


def enclosed(instances, mesh, mat=0, first=False):
    """`instances` plus three that keep BvhTLAS::build from splitting: one copy of
    `mesh` (octa(0): box exactly [-1, 1]^3, and faces large enough that
    Triangle::intersect's |a| >= kEps still holds for a ray direction scaled by
    1 / BIG, mesh.cpp:31) scaled by BIG, whose bounds are the root's, and
    two copies scaled by TINY that touch the root's opposite corners.  The TLAS
    key is the half extent: on every axis the tiny ones lie in the first bin
    and the big one in the last, so each side of every candidate plane spans
    the root box and costs count * area(root): no plane beats the parent
    (cost >= parentCost, bvh.cpp:915).  BIG and TINY are powers of two: the
    bounds and the costs are exact.  The caller's instances keep their order;
    the three follow, or come first."""
    far = BIG - TINY
    three = [(mesh, mat, f32(Sc(BIG))), (mesh, mat, f32(T(far, far, far) @ Sc(TINY))), (mesh, mat, f32(T(-far, -far, -far) @ Sc(TINY)))]
    return three + list(instances) if first else list(instances) + three


def transforms(alt=False):
    """Scene A's sixteen matrices around a ring of radius 60 (their translations
    first, the class second).  alt: the re-upload's second set -- the same count,
    other angles and factors, affine rows turned projective and back."""
    k = 1.3 if alt else 1.0
    cls = [
        np.eye(4),
        Rot((1, 2, 3), 37.3 * k),
        Sc(0.05, 1.0, 20.0) if not alt else Sc(20.0, 0.05, 1.0),
        Shear(0.7 * k, -0.4, 1.1),
        Sc(-1.0, 1.0, 1.0) @ Rot((0, 1, 1), 20.0 * k),
        Sc(1e-2),                                   # moved to 1e4 below
        Sc(1e3) if not alt else Sc(7e2),
        Rot((1, 1, 0), 31.0 * k) @ Sc(1e-3, 1.0, 1e3) @ Rot((0, 1, 2), 17.0),      # condition ~ 1e6
        Row3(Sc(1.0), (0, 0, 0, 2.0)) if not alt else Rot((1, 0, 0), 12.0),        # uniform w
        Row3(Rot((0, 0, 1), 11.0), (0, 0, 0.01, 1.0)) if not alt else Sc(1.5),     # projective
        Rot((3, 1, 2), 63.1 * k) @ Sc(0.3, 0.7, 1.9) @ Shear(0.31, 0.17, -0.23),   # affine; in A its f32 inverse is not
        Row3(Rot((2, 1, 3), 23.7) @ Sc(0.37, 1.13, 0.71), (0, 0, 0, 3.0)),         # w = 3: row 3 of the inverse is inexact
        Row3(Rot((1, 3, 2), 51.9) @ Sc(1.7, 0.9, 0.53), (0.003, -0.002, 0.001, 1.3)),
        Rot((0, 1, 0), 90.0) @ Sc(2.0),
        Shear(0.0, 2.5 * k, 0.0) @ Sc(1.0, 3.0, 0.2),
        Sc(1.0) if not alt else Row3(Rot((0, 1, 0), 33.0), (0, 0.01, 0, 1.0)),     # affine in A, projective in Aalt
    ]
    out = []
    for i, m in enumerate(cls):
        ang = 2 * np.pi * (i + (0.37 if alt else 0.0)) / len(cls)
        pos = (1e4, 1e4 * 0.5, -1e4 * 0.25) if i == 5 else (60.0 * np.cos(ang), 7.0 * ((i % 3) - 1), 60.0 * np.sin(ang))
        if i == 6:
            pos = (0.0, 0.0, 0.0)                   # the scale-1e3 sphere surrounds the ring
        out.append(f32(T(*pos) @ m))
    return out


def spread(n, step=10.0, per_row=9):
    """n positions on a grid `step` apart, multiples of 0.5: translations by them are exact."""
    return [((i % per_row - per_row // 2) * step, ((i // per_row) % 3 - 1) * step, (i // (3 * per_row) - 1) * step + 0.5 * (i // per_row))
            for i in range(n)]


def leaf_meshes():
    return [fan(100 + n, n) for n in (1, 2, 3, 4, 127, 128, 200)] + [clusters(7, [1, 2, 3, 4, 5, 6, 9, 17, 40] * 2 + [127, 128, 130])]


def scene_B(n_planes, projective_at=None, total=None):
    """Mesh 0: the sphere (enclosure), 1..7 the root leaves, 8 the soup, 9 the
    2-triangle plane.  The enclosure (positions 0..2), the eight meshes (3..10),
    then the plane copies from position 11 on (consecutive TLAS positions: a root
    leaf keeps instance order)."""
    meshes = [octa(0)] + leaf_meshes() + [plane2()]
    n_inst = 8 + n_planes
    pos = spread(n_inst)
    inst = [(1 + k, 4 if k == 7 else k % 4, f32(T(*pos[k]) @ Rot((1, k, 2), 13.0 * k))) for k in range(8)]      # the last one is lit
    for k in range(n_planes):
        # signed axis permutations, shears and scales by powers of two: the f32 inverse is exact (row 3 = 0, 0, 0, 1)
        perm = np.eye(4)[[(k % 3), ((k + 1) % 3), ((k + 2) % 3), 3]] @ np.diag([1.0, -1.0 if k % 2 else 1.0, 1.0, 1.0])
        m = T(*pos[8 + k]) @ Shear(0.5 * (k % 3), 0.25 * (k % 2), 0.0) @ perm @ Sc(2.0 if k % 4 else 1.0)
        if k == projective_at:
            m = Row3(m, (0.0, 0.004, 0.0, 1.0))
        inst.append((9, (k + 1) % 4, f32(m)))
    inst = enclosed(inst, mesh=0, first=True)
    assert total is None or len(inst) == total
    return {"meshes": meshes, "materials": MATERIALS, "instances": inst}


def scene_C(nan=False):
    zero = with_zero_area(21, 400)
    if nan:
        zero[0][137, 2, 2] = np.nan        # the last vertex grown into its leaf box: the box keeps the NaN (tmin / tmax)
    sphere = octa(2)
    doubled = (np.concatenate([sphere[0], sphere[0]]), np.concatenate([sphere[1], sphere[1]]))
    big = octa(2)
    big = ((big[0].astype(np.float64) * 1e13 + 1e18).astype(np.float32), big[1])
    small = octa(2)
    small = ((small[0].astype(np.float64) * 1e-18).astype(np.float32), small[1])
    inst = [(0, 0, f32(T(-4, 0, 0))), (1, 1, f32(T(0, 0.5, 0) @ Rot((1, 1, 0), 25.0))), (2, 2, f32(T(4, 0, 0) @ Sc(1.5))),
            (3, 0, f32(np.eye(4))), (4, 1, f32(T(0, -4, 0) @ Sc(1e18)))]
    return {"meshes": [zero, doubled, grid(12), big, small], "materials": MATERIALS, "instances": inst}


def scene_E(fillers):
    tri = (np.array([[(-0.5, -0.5, 0), (0.5, -0.5, 0), (0, 0.5, 0)]], np.float32), face_normals([[(-0.5, -0.5, 0), (0.5, -0.5, 0), (0, 0.5, 0)]]))
    meshes = [tri] * fillers + [soup(3, 35000, 0.01)]
    meshes[-1] = (meshes[-1][0][:34676], meshes[-1][1][:34676])
    inst = [(k, k % 4, f32(T(-3.0 + k, 2.0, 0.0) @ Rot((0, 1, 0), 20.0 * k))) for k in range(fillers)]
    inst.append((fillers, 0, f32(np.eye(4))))
    return {"meshes": meshes, "materials": MATERIALS, "instances": inst,
            "view": {"pos": (0.0, 0.3, -2.2), "target": (0.0, 0.0, 0.0), "fov_y": 55.0, "focal": 2.2, "defocus": 0.2}}


VIEW_RING = {"pos": (0.0, 25.0, -95.0), "target": (0.0, 0.0, 0.0), "fov_y": 60.0, "focal": 95.0, "defocus": 0.5}
VIEW_B = {"pos": (0.0, 4.0, -60.0), "target": (0.0, 0.0, 0.0), "fov_y": 60.0, "focal": 60.0, "defocus": 0.3}


def scene_L(two_meshes, closed=False):
    """A2's ring with emitters: L1 one 32-triangle sphere instanced twice as a lamp
    (one BLAS of 64-B records and 48-B triangles well under 20 KiB: staged); L2 that
    sphere and a 128-triangle one (two BLASes: never staged), the second under a
    projective matrix.  Mirror, glass and diffuse spheres around them, a diffuse
    floor below, the gradient sky above."""
    meshes = [octa(3), octa(1), octa(2), plane2()]
    mats = MATERIALS[:4] + [LAMP, LAMP2]
    inst = [(0, i % 4, m) for i, m in enumerate(transforms()) if i not in (5, 6)]
    inst.append((1, 4, f32(T(0, 30, 0) @ Sc(6.0))))
    second = Row3(T(25, 20, -20) @ Sc(5.0), (0.0, 0.002, 0.0, 1.0)) if two_meshes else T(25, 20, -20) @ Sc(5.0)
    inst.append((2 if two_meshes else 1, 5 if two_meshes else 4, f32(second)))
    inst.append((3, 0, f32(T(0, -12, 0) @ Sc(90.0))))            # a diffuse floor under the ring: most shadow rays start here
    if closed:
        inst.append((0, 2, f32(Sc(1e3))))                        # A's mirror sphere around everything: no path sees the sky
    return {"meshes": meshes, "materials": mats, "instances": inst, "view": VIEW_RING, "background": SKY}


def _spec(name):
    if name in ("A", "Aalt"):
        return {"meshes": [octa(3), octa(0)], "materials": MATERIALS, "view": VIEW_RING,
                "instances": enclosed([(0, 4 if i == 13 else i % 4, m) for i, m in enumerate(transforms(name == "Aalt"))], mesh=1)}
    if name == "A2":
        return {"meshes": [octa(3)], "materials": MATERIALS, "view": VIEW_RING,
                "instances": [(0, 4 if i == 13 else i % 4, m) for i, m in enumerate(transforms())]}
    if name == "B1":
        return dict(scene_B(40), view=VIEW_B)
    if name == "B2":
        return dict(scene_B(40, projective_at=17), view=VIEW_B)
    if name == "B64":
        return dict(scene_B(53, total=64), view=VIEW_B)
    if name == "B65":
        return dict(scene_B(54, total=65), view=VIEW_B)
    if name in ("C", "Cnan"):
        return dict(scene_C(name == "Cnan"), view={"pos": (0.0, 1.5, -5.0), "target": (0.0, 0.0, 0.0), "fov_y": 75.0, "focal": 5.0, "defocus": 0.3})
    if name == "Ddeep":
        return {"meshes": [plates(72, 30, 0)], "materials": MATERIALS, "instances": [(0, 0, f32(np.eye(4)))]}
    if name == "Dtoo":
        return {"meshes": [plates(72, 30, 20)], "materials": MATERIALS, "instances": [(0, 0, f32(np.eye(4)))]}
    if name == "E0":
        return scene_E(6)
    if name == "E1":
        return scene_E(7)
    if name in ("L1", "L2", "L1c", "L2c"):
        return scene_L(name[:2] == "L2", closed=name.endswith("c"))
    raise KeyError(name)


ALL = ["A", "A2", "Aalt", "B1", "B2", "B64", "B65", "C", "Cnan", "Ddeep", "Dtoo", "E0", "E1", "L1", "L2", "L1c", "L2c"]
TRACED = [n for n in ALL if n != "Dtoo"]                  # scenes the product can upload
BRUTE = [n for n in TRACED if n != "Cnan"]                # ... and whose rays have a brute-force answer
NO_HIT_NEEDED = {"C": {4}}     # the 1e-18 mesh: |a| = |e1 . (d x e2)| < kEps for every ray (mesh.cpp:31), a defined miss


# ---- the product side --------------------------------------------------------

REC = {"triangles": 64, "tri_ext": 80, "blas_indices": 4, "blas_nodes": 48, "materials": 64, "instances": 160, "tlas_indices": 4,
       "tlas_nodes": 48, "lights": 8, "background": 64}
COUNT = {"triangles": "triangle_count", "blas_indices": "blas_index_count", "blas_nodes": "blas_node_count", "materials": "material_count",
         "instances": "instance_count", "tlas_nodes": "tlas_node_count", "lights": "light_count"}


class ExportedScene:
    """What Renderer.__init__ and Renderer.update_instances need of a scene
    (desc(), buffers(), camera()), over the oracle's ten exported buffers
    (GPUBatcher's layout, include/surf_hip.h).  It owns the arrays the
    descriptor points into; the camera is the oracle's camera_ubo."""

    def __init__(self, oracle_scene):
        self._o = oracle_scene
        self._arrays = {k: np.frombuffer(v, np.uint8).copy() for k, v in oracle_scene.export().items()}
        d = surf_amd.SceneDesc()
        for name, a in self._arrays.items():
            assert a.size % REC[name] == 0, name
            setattr(d, name, a.ctypes.data if a.size else None)
            if name in COUNT:
                setattr(d, COUNT[name], a.size // REC[name])
        assert self._arrays["tri_ext"].size // 80 == d.triangle_count and self._arrays["tlas_indices"].size // 4 == d.instance_count
        self._desc = d

    def desc(self):
        return self._desc

    def buffers(self):
        return {k: v.tobytes() for k, v in self._arrays.items()}

    def camera(self, width, height):
        return self._o.camera_ubo(width, height)


# ---- geometry read back from an export, and the ray sets -----------------------

class Geometry:
    def __init__(self, ex):
        inst = np.frombuffer(ex["instances"], np.uint32).reshape(-1, 40)
        self.n = len(inst)
        self.tri_offset, self.node_offset = inst[:, 0].astype(np.int64), inst[:, 2].astype(np.int64)
        self.M = inst[:, 8:24].copy().view(np.float32).reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)
        self.Minv = inst[:, 24:40].copy().view(np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)
        self.blas_nodes = np.frombuffer(ex["blas_nodes"], np.float32).reshape(-1, 12)
        self.blas_u = np.frombuffer(ex["blas_nodes"], np.uint32).reshape(-1, 12)
        self.tlas_nodes = np.frombuffer(ex["tlas_nodes"], np.float32).reshape(-1, 12)
        self.tlas_u = np.frombuffer(ex["tlas_nodes"], np.uint32).reshape(-1, 12)
        self.tlas_idx = np.frombuffer(ex["tlas_indices"], np.uint32)
        self.tris = np.frombuffer(ex["triangles"], np.float32).reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
        starts = np.unique(np.append(self.tri_offset, len(self.tris)))
        self.tri_count = starts[np.searchsorted(starts, self.tri_offset) + 1] - self.tri_offset
        self.root_lo = self.blas_nodes[self.node_offset, 4:7].astype(np.float64)
        self.root_hi = self.blas_nodes[self.node_offset, 8:11].astype(np.float64)
        self.root_count = self.blas_u[self.node_offset, 1]

    def world(self, i, p):
        """M_i * (p, 1) with the w divide, float64 (p: (k, 3) object-space points)."""
        with np.errstate(all="ignore"):
            q = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ self.M[i].T
            return q[:, :3] / q[:, 3:4]

    def corners(self, i, about=1.0):
        lo, hi = self.root_lo[i], self.root_hi[i]
        mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo) * about
        c = np.array([[mid[a] + (half[a] if (k >> a) & 1 else -half[a]) for a in range(3)] for k in range(8)])
        return self.world(i, c)

    def blas_node_counts(self):
        """Nodes of each instance's BLAS: the next BLAS's offset, or the total, minus its own."""
        starts = np.unique(np.append(self.node_offset, len(self.blas_nodes)))
        return starts[np.searchsorted(starts, self.node_offset) + 1] - self.node_offset

    def leaf_counts(self, i):
        n = self.blas_node_counts()[i]
        c = self.blas_u[self.node_offset[i]:self.node_offset[i] + n, 1]
        keep = np.ones(n, bool)
        if n > 1:
            keep[1] = False              # node 1 of a BLAS is never used (bvh.cpp:77)
        return c[keep & (c > 0)]


def _unit(v):
    with np.errstate(all="ignore"):
        return v / np.linalg.norm(v, axis=1, keepdims=True)


def _clean(o, d):
    """float32 rays; a ray with a non-finite component (sources near a NaN or
    overflowing target) is replaced by one from the origin along +z."""
    with np.errstate(all="ignore"):
        o, d = np.asarray(o, np.float64).astype(np.float32), np.asarray(d, np.float64).astype(np.float32)
    bad = ~(np.isfinite(o).all(1) & np.isfinite(d).all(1) & (np.abs(d).sum(1) > 0))
    o[bad], d[bad] = (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)
    return o, d


def ray_sets(ex, seed, extra=None):
    """name -> (o, d) float32, built in float64 from the export; "silhouette" also
    carries the f32 distance to its target (the any-hit tmax), and the instance aimed at."""
    g = Geometry(ex)
    rng = np.random.default_rng(seed)
    out = {}
    with np.errstate(all="ignore"):
        lo, hi = g.tlas_nodes[0, 4:7].astype(np.float64), g.tlas_nodes[0, 8:11].astype(np.float64)
        ext = np.where(np.isfinite(hi - lo), hi - lo, 1.0)
        lo, hi = np.where(np.isfinite(lo), lo, -1.0), np.where(np.isfinite(hi), hi, 1.0)
        # random rays through the scene's box: half from box point to box point, half toward an instance's box
        a = rng.uniform(lo - 0.2 * ext, hi + 0.2 * ext, (1000, 3))
        b = rng.uniform(lo, hi, (1000, 3))
        pick = rng.integers(0, g.n, 500)
        b[:500] = np.concatenate([g.world(i, rng.uniform(g.root_lo[i], g.root_hi[i], (1, 3))) for i in pick])
        out["random"] = _clean(a, _unit(b - a))
        # silhouette rays: at transformed vertices and edge midpoints of every instance, and just inside and
        # just outside its world box; sources a few triangle sizes, or a few instance sizes, away
        per = int(np.clip(3200 // g.n, 48, 400))
        tg, src, who = [], [], []
        for i in range(g.n):
            t = g.tris[g.tri_offset[i] + rng.integers(0, g.tri_count[i], per)]
            k = rng.integers(0, 6, per)
            va, vb = t[np.arange(per), k % 3], t[np.arange(per), (k + 1) % 3]
            p = g.world(i, np.where((k < 3)[:, None], va, 0.5 * (va + vb)))
            local = np.linalg.norm(g.world(i, va) - g.world(i, vb), axis=1)
            box = g.corners(i)
            size = 0.5 * np.nanmax(box.max(0) - box.min(0))
            nb = max(16, per // 2)               # a third of the targets: the box's corners, seen from many sides
            p = np.concatenate([p, np.concatenate([g.corners(i, 0.99), g.corners(i, 1.01)])[np.arange(nb) % 16]])
            scale = np.concatenate([np.where(np.arange(per) % 2 == 0, local, size), np.full(nb, size)])
            tg.append(p)
            src.append(p + _unit(rng.normal(size=p.shape)) * (scale * rng.uniform(1.5, 4.0, len(p)))[:, None])
            who.append(np.full(len(p), i))
        tg, src, who = np.concatenate(tg), np.concatenate(src), np.concatenate(who)
        s32 = src.astype(np.float32)
        dv = (tg.astype(np.float32) - s32).astype(np.float32)
        dist = np.linalg.norm(dv, axis=1).astype(np.float32)
        o, d = _clean(s32, dv / dist[:, None])
        dist = np.where(np.isfinite(dist), dist, F(1.0)).astype(np.float32)
        out["silhouette"] = (o, d, dist, who)
        # origins inside instance boxes: random directions, and axis-parallel ones with exact zeros
        pick = rng.integers(0, g.n, 1200)
        inside = np.concatenate([g.world(i, rng.uniform(g.root_lo[i], g.root_hi[i], (1, 3))) for i in pick])
        out["inside"] = _clean(inside[:600], _unit(rng.normal(size=(600, 3))))
        axis = np.zeros((600, 3))
        axis[np.arange(600), rng.integers(0, 3, 600)] = rng.choice([-1.0, 1.0], 600)
        back = np.where(np.arange(600)[:, None] % 2 == 0, 0.0, axis * ext.max() * 0.01)   # half of them start outside
        out["axis"] = _clean(inside[600:] - back, axis)
    if extra is not None:
        out["extra"] = _clean(*extra(g, rng))
    return out


def grid_rays(g, rng):
    """Scene C's flat grid (instance 2): rays inside its plane and along its edges.
    The grid lies in the object plane y = 0; M_2 is a translation and a uniform
    scale, so the world plane is y = M[1][3] and the edges stay axis-parallel."""
    M = g.M[2]
    y, s = M[1, 3], M[0, 0]
    xs = M[0, 3] + s * np.linspace(-1.0, 1.0, 13)
    zs = M[2, 3] + s * np.linspace(-1.0, 1.0, 13)
    o, d = [], []
    for x in xs:                                              # along the edges x = const, both ways, from outside and inside
        for z0, dz in ((zs[0] - 1.0, 1.0), (zs[-1] + 1.0, -1.0), (zs[5], 1.0)):
            o.append((x, y, z0)); d.append((0.0, 0.0, dz))
    for z in zs:
        for x0, dx in ((xs[0] - 1.0, 1.0), (xs[-1] + 1.0, -1.0), (xs[7], -1.0)):
            o.append((x0, y, z)); d.append((dx, 0.0, 0.0))
    ang = rng.uniform(0, 2 * np.pi, 300)                      # inside the plane, any heading
    for a in ang:
        o.append((rng.uniform(xs[0] - 1, xs[-1] + 1), y, rng.uniform(zs[0] - 1, zs[-1] + 1))); d.append((np.cos(a), 0.0, np.sin(a)))
    for a in ang[:100]:                                       # grazing: a small slope toward the plane
        o.append((rng.uniform(xs[0], xs[-1]), y + 0.01, rng.uniform(zs[0], zs[-1]))); d.append((np.cos(a), -1e-3, np.sin(a)))
    o, d = np.array(o), np.array(d)
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


class Case:
    def __init__(self, name):
        self.name = name
        spec = _spec(name)
        self.spec = spec
        self.oracle = oracle.OracleScene.custom(spec["meshes"], spec["materials"], spec["instances"],
                                                background=spec.get("background"), view=spec.get("view"))
        self.export = self.oracle.export()
        self.geometry = Geometry(self.export)
        self._rays = None

    @property
    def rays(self):
        if self._rays is None:
            seed = 1000 + ALL.index(self.name)
            self._rays = ray_sets(self.export, seed, grid_rays if self.name in ("C", "Cnan") else None)
        return self._rays

    def all_rays(self):
        """Every ray set, concatenated: (o, d)."""
        sets = [v[:2] for v in self.rays.values()]
        return np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])

    def product(self):
        return ExportedScene(self.oracle)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(name)


def run_layout(g: Geometry):
    """(run heads, run members) as buildInstanceTables lays them out, restated from
    the export: maximal sequences of consecutive positions of a root-leaf TLAS
    whose instances have an exact affine inverse row 3 and a root leaf of 1 or 2
    triangles over one triangle range; at most 32 long, none of one, only
    positions below 63 and only up to 64 instances."""
    head, member = [], []
    n = int(g.tlas_u[0, 1])
    if n == 0 or n > 64 or g.tlas_u[0, 0] != 0:
        return head, member
    affine = (g.Minv[:, 3] == np.array([0, 0, 0, 1], np.float32)).all(1)
    ok = lambda k: affine[g.tlas_idx[k]] and 1 <= g.root_count[g.tlas_idx[k]] <= 2
    same = lambda k, j: g.tri_offset[g.tlas_idx[k]] == g.tri_offset[g.tlas_idx[j]]
    end, k = min(n, K_RUN_POSITIONS), 0
    while k < end:
        ln = 0
        if ok(k):
            ln = 1
            while k + ln < end and ln < K_RUN_MAX and ok(k + ln) and same(k, k + ln):
                ln += 1
        if ln >= 2:
            head.append(k)
            member += list(range(k, k + ln))
        k += max(ln, 1)
    return head, member


# ============================ the CPU checks =====================================

def glm_f32():
    """glm 0.9.9's translate / rotate / scale in float32, operation for operation
    (matrix_transform.inl), with this machine's cosf / sinf: the matrices of
    examples/indoor_scene.hpp as the reference computes them."""
    libm = C.CDLL("libm.so.6")
    for fn in (libm.cosf, libm.sinf):
        fn.argtypes, fn.restype = [C.c_float], C.c_float

    def translate(m, v):
        r = m.copy()
        r[:, 3] = ((m[:, 0] * F(v[0]) + m[:, 1] * F(v[1])) + m[:, 2] * F(v[2])) + m[:, 3]
        return r

    def scale(m, v):
        r = m.copy()
        for k in range(3):
            r[:, k] = m[:, k] * F(v[k])
        return r

    def rotate(m, angle, v):
        c, s = F(libm.cosf(angle)), F(libm.sinf(angle))
        v = np.asarray(v, np.float32)
        inv = F(1.0) / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ax = v * inv
        tp = (F(1.0) - c) * ax
        R = np.zeros((3, 3), np.float32)
        R[0] = (c + tp[0] * ax[0], tp[0] * ax[1] + s * ax[2], tp[0] * ax[2] - s * ax[1])
        R[1] = (tp[1] * ax[0] - s * ax[2], c + tp[1] * ax[1], tp[1] * ax[2] + s * ax[0])
        R[2] = (tp[2] * ax[0] + s * ax[1], tp[2] * ax[1] - s * ax[0], c + tp[2] * ax[2])
        r = m.copy()
        for k in range(3):
            r[:, k] = (m[:, 0] * R[k, 0] + m[:, 1] * R[k, 1]) + m[:, 2] * R[k, 2]
        return r
    return translate, rotate, scale


def bundled_room_spec():
    translate, rotate, scale = glm_f32()
    I = np.eye(4, dtype=np.float32)
    quarter = F(F(F(90.0) * F(3.14159265358979323846264)) * F(0.005555555555555))      # radians(90.0f), surf_math.h:231
    fwd, right = (0.0, 0.0, -1.0), (1.0, 0.0, 0.0)
    sus, cube, lens, plane = 0, 1, 2, 3
    mats = [{"albedo": (0.8, 0.8, 0.8), "refl": 0.01}, {"albedo": (1.0, 0.0, 0.0)}, {"albedo": (0.0, 1.0, 0.0)}, {"albedo": (1.0, 0.0, 0.0)},
            {"albedo": (0.7, 0.7, 0.2), "absorption": (0.03, 0.04, 0.03), "refr": 1.0, "ior": 1.42}, {"albedo": (0.2, 0.9, 1.0), "refl": 0.8},
            {"emit_color": (1.0, 0.8, 0.6), "emit": 5.0}, {"emit_color": (1.0, 0.5, 0.2), "emit": 5.0}]
    floor_m, red, green, diff, diel, spec, soft, redl = range(8)
    inst = [
        (plane, floor_m, scale(translate(I, (0, -1, 0)), (10, 10, 10))),
        (cube, soft, scale(translate(I, (-8, 7, 5)), (0.5, 0.5, 0.5))),
        (cube, redl, scale(translate(I, (9, 5, -5)), (1, 1, 1))),
        (sus, diff, translate(I, (0, 0, -1))),
        (sus, spec, translate(I, (3, 0, -1))),
        (lens, diel, translate(I, (-3, 0, -1))),
        (plane, red, scale(rotate(translate(I, (-10, 4, 0)), quarter, fwd), (5, 10, 10))),
        (plane, green, scale(rotate(translate(I, (10, 4, 0)), quarter, fwd), (5, 10, 10))),
        (plane, floor_m, scale(translate(I, (0, 9, 0)), (10, 10, 10))),
        (plane, floor_m, scale(rotate(translate(I, (0, 4, -10)), quarter, right), (10, 10, 5))),
        (plane, floor_m, scale(rotate(translate(I, (0, 4, 10)), quarter, right), (10, 10, 5))),
    ]
    return [obj(n) for n in ("susanne", "cube", "lens", "plane")], mats, inst


def test_custom_entry_rebuilds_the_bundled_room_byte_for_byte(oracle_scene):
    """The four OBJ meshes through oracle.obj_load and the eleven matrices of
    examples/indoor_scene.hpp through OracleScene.custom: all ten exported
    buffers, the camera and a 32 x 24 x 2 render equal OracleScene(variant=0)'s."""
    meshes, mats, inst = bundled_room_spec()
    o = oracle.OracleScene.custom(meshes, mats, inst)
    try:
        want, got = oracle_scene.export(), o.export()
        assert list(got) == oracle.EXPORT_ORDER
        for k in want:
            assert got[k] == want[k], k
        assert o.camera_ubo(32, 24) == oracle_scene.camera_ubo(32, 24)
        assert o.bvh_depths() == oracle_scene.bvh_depths() and o.light_count() == 2 and o.instance_count() == 11
        g = np.load(os.path.join(GOLDEN, "oracle_32x24x2.npz"))
        acc, cnt, _ = o.render(32, 24, 2)
        assert np.array_equal(acc.view(np.uint32), g["acc"].view(np.uint32))
        assert [cnt[k] for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")] == list(g["counts"])
    finally:
        o.close()


def test_custom_entry_refuses_what_it_must():
    v, n = octa(0)
    ok = [(0, 0, np.eye(4))]
    oracle.OracleScene.custom([(v, n)], [GREY], ok).close()
    bad = np.eye(4)
    bad[1, 2] = np.inf
    nan = np.eye(4)
    nan[3, 3] = np.nan
    for meshes, mats, inst in [([(v, n)], [GREY], [(1, 0, np.eye(4))]), ([(v, n)], [GREY], [(0, 1, np.eye(4))]),
                               ([(v, n)], [GREY], [(0, 0, bad)]), ([(v, n)], [GREY], [(0, 0, nan)]), ([(v, n)], [GREY], []),
                               ([(v[:0], n[:0])], [GREY], ok), ([(v, n)], [], ok), ([(v, n)], [GREY], [(-1, 0, np.eye(4))])]:
        with pytest.raises(ValueError):
            oracle.OracleScene.custom(meshes, mats, inst)
    with pytest.raises(TypeError):
        oracle.OracleScene.custom([(v, n)], [{"colour": (1, 1, 1)}], ok)
    # a NaN vertex is a scene (test_bvh_build pins the builder's answer); a tree deeper than 127 is none
    vn = v.copy()
    vn[3, 1, 0] = np.nan
    oracle.OracleScene.custom([(vn, n)], [GREY], ok).close()
    with pytest.raises(ValueError):
        oracle.OracleScene.custom([plates(75, 33, 33)], [GREY], ok)      # depth 140


def test_material_defaults_view_and_background_reach_the_export():
    o = oracle.OracleScene.custom([octa(0)], [{}, LAMP], [(0, 1, np.eye(4)), (0, 0, T(3, 0, 0))], background={"type": 0, "color": (0.1, 0.2, 0.3)},
                                  view={"pos": (0, 0, -9), "target": (0, 0, 0), "fov_y": 40.0, "focal": 9.0, "defocus": 0.0})
    try:
        ex = o.export()
        m = np.frombuffer(ex["materials"], np.float32).reshape(-1, 16)
        assert m[0].tolist() == [6.0, 0.0, 0.0, 1.0, 1.0, F(0.9), F(0.7), 0.0] + [0.0] * 8      # first use: the lamp
        assert m[1].tolist() == [0.0, 0.0, 0.0, 1.0] + [0.0] * 12                               # Material's defaults
        assert np.frombuffer(ex["lights"], np.uint32).tolist() == [0, 8]
        assert np.frombuffer(ex["background"], np.uint32)[0] == 0
        u = np.frombuffer(o.camera_ubo(8, 8), np.float32)
        assert tuple(u[0:3]) == (0.0, 0.0, -9.0) and tuple(u[28:32]) == (8.0, 8.0, 9.0, 0.0)
        assert np.frombuffer(ex["tri_ext"], np.float32).reshape(-1, 20)[:, 12:].any() == False      # zero UVs
        inst = np.frombuffer(ex["instances"], np.float32).reshape(-1, 40)
        assert inst[1, 8:24].reshape(4, 4)[3].tolist() == [3.0, 0.0, 0.0, 1.0]                  # column major: column 3 = translation
    finally:
        o.close()


@pytest.mark.parametrize("name", ["A", "B65", "C", "L2"])
def test_exported_scene_describes_the_export(name):
    c = case(name)
    p = c.product()
    d = p.desc()
    assert p.buffers() == c.export
    assert d.instance_count == c.oracle.instance_count() and d.light_count == c.oracle.light_count()
    assert d.triangle_count == sum(len(c.spec["meshes"][m][0]) for m in dict.fromkeys(i[0] for i in c.spec["instances"]))
    assert d.blas_index_count == d.triangle_count and d.tlas_node_count >= 2 and d.material_count <= len(c.spec["materials"])
    assert p.camera(32, 24) == c.oracle.camera_ubo(32, 24)


# Rays on which the walk's (hit, t) differs from brute force, per ray set, as measured; "room" is the bundled room
# through orc_scene_create with ray_sets(export, 5).  Every `inside` set (origins and directions in general position)
# agrees completely; the rest are rays aimed at vertices, edges and box corners, axis-parallel rays, and C's and the
# ring scenes' boxes at 1e3 to 1e18.
WALK_NE_BRUTE = {
    "room": {"random": 0, "silhouette": 15, "inside": 0, "axis": 0},
    "A": {"random": 0, "silhouette": 72, "inside": 0, "axis": 1},
    "A2": {"random": 36, "silhouette": 19, "inside": 0, "axis": 0},
    "Aalt": {"random": 3, "silhouette": 75, "inside": 0, "axis": 5},
    "B1": {"random": 0, "silhouette": 25, "inside": 0, "axis": 2},
    "B2": {"random": 0, "silhouette": 24, "inside": 0, "axis": 2},
    "B64": {"random": 0, "silhouette": 10, "inside": 0, "axis": 2},
    "B65": {"random": 0, "silhouette": 14, "inside": 0, "axis": 1},
    "C": {"random": 378, "silhouette": 70, "inside": 0, "axis": 228, "extra": 0},
    "Ddeep": {"random": 0, "silhouette": 2, "inside": 0, "axis": 0},
    "E0": {"random": 0, "silhouette": 92, "inside": 0, "axis": 0},
    "E1": {"random": 0, "silhouette": 99, "inside": 0, "axis": 0},
    "L1": {"random": 10, "silhouette": 70, "inside": 0, "axis": 0},
    "L2": {"random": 28, "silhouette": 64, "inside": 0, "axis": 0},
    "L1c": {"random": 20, "silhouette": 70, "inside": 0, "axis": 0},
    "L2c": {"random": 25, "silhouette": 46, "inside": 0, "axis": 0},
}


def walk_against_brute(o_scene, rays, what):
    """Asserts what the reference's walk guarantees against brute force on every
    ray -- a hit of the walk is a hit of brute force, and never a nearer one --
    and returns, per ray set, the rays on which (hit, t) differ."""
    out = {}
    for k, rs in rays.items():
        o, d = rs[:2]
        t, _, _, inst, _ = o_scene.trace_closest(o, d)
        tb, ib, _ = o_scene.trace_brute(o, d)
        hit, hb = inst != UNSET, ib != UNSET
        assert not (hit & ~hb).any(), f"{what} {k}: the walk hits what brute force misses on {np.nonzero(hit & ~hb)[0][:5]}"
        assert (tb[hit] <= t[hit]).all(), f"{what} {k}: the walk is nearer than brute force"
        out[k] = int(((hit != hb) | (t != tb)).sum())
    return out


def test_bundled_room_walk_is_not_brute_force_at_vertices(oracle_scene):
    """The reason the scenes below are not held to walk == brute force, pinned on
    the scene and entry that were there before: on 15 of the 4,785 rays aimed at
    the bundled room's vertices, edge midpoints and box corners the reference's
    walk ends on a farther triangle than brute force finds (AABB::intersect,
    bvh.cpp:40-66, rejects the nearer leaf's box), and on no ray of the other sets."""
    got = walk_against_brute(oracle_scene, ray_sets(oracle_scene.export(), 5), "room")
    assert got == WALK_NE_BRUTE["room"], got


@pytest.mark.parametrize("name", BRUTE)
def test_closest_against_brute_force_and_any_hit(name):
    """test_oracle.py::test_bvh_closest_equals_brute_force and
    ::test_any_hit_consistent_with_closest on every scene's own rays, as far as
    the reference's walk allows.

    Equality with brute force holds for the room's random rays, not in general:
    AABB::intersect (bvh.cpp:40-66) is not conservative.  A ray through a
    vertex or an edge that lies on a node's box face, a zero direction
    component inside a flat box (0 * inf), or a box at coordinates of 1e3 and
    more seen from far away can fail the slab test of a node whose triangle
    Triangle::intersect accepts, and the walk then skips that leaf.  The bundled
    room shows it through orc_scene_create as well
    (test_bundled_room_walk_is_not_brute_force_at_vertices), so it is the
    reference's behaviour, and what the GPU has to reproduce.  Asserted:
      * for every ray: a hit of the walk is a hit of brute force, never nearer;
      * per ray set, the number of rays on which they differ equals the pinned
        WALK_NE_BRUTE figure (0 for every set in general position), so a
        change of the builder or the walk shows;
      * an any-hit answer of 1 has a brute-force t below tmax, and with tmax
        away from the hit distances any-hit equals (closest t < tmax) exactly.
    (With tmax at a vertex the target's own leaf box starts at t0 = tmax up to
    rounding and `t0 < depth` may prune it: there any-hit is only printed.)"""
    c = case(name)
    got = walk_against_brute(c.oracle, c.rays, name)
    print(f"{name}: walk != brute force on {got}")
    assert got == WALK_NE_BRUTE[name], got
    o, d = c.all_rays()
    t = c.oracle.trace_closest(o, d)[0]
    tb = c.oracle.trace_brute(o, d)[0]
    names = list(c.rays)
    at = sum(len(c.rays[k][0]) for k in names[:names.index("silhouette")])
    sil = slice(at, at + len(c.rays["silhouette"][0]))
    dist = c.rays["silhouette"][2]
    with np.errstate(all="ignore"):
        half = (F(0.5) * np.minimum(t, F(1e20)) + F(0.25)).astype(np.float32)
    every = slice(0, len(o))
    checks = [(every, half, True), (every, np.full(len(o), 1e30, np.float32), True)]
    checks += [(sil, tm, False) for tm in (dist, np.nextafter(dist, F(0)), np.nextafter(dist, F(np.inf)))]
    for sl, tm, general in checks:
        occ = c.oracle.trace_any(o[sl], d[sl], tm).astype(bool)
        assert (tb[sl][occ] < tm[occ]).all(), f"{name}: any-hit reports a hit that brute force does not have below tmax"
        other = int((occ != (t[sl] < tm)).sum())
        print(f"{name}: any-hit != (closest t < tmax) on {other} of {len(occ)} rays" + ("" if general else " (tmax at the target)"))
        assert not general or other == 0


def hit_figures(name):
    c = case(name)
    o, d = c.all_rays()
    inst = c.oracle.trace_closest(o, d)[3]
    per = np.bincount(inst[inst != UNSET], minlength=c.geometry.n)
    # a silhouette ray counts as a hit when it ends on the instance it was aimed at: inside A's and B's enclosure
    # (and scene A's scale-1e3 sphere) every ray ends on something
    so, sd, _, who = c.rays["silhouette"]
    sil = float((c.oracle.trace_closest(so, sd)[3] == who).mean())
    return per, sil


@pytest.mark.parametrize("name", BRUTE)
def test_every_instance_is_hit_and_silhouettes_are_silhouettes(name):
    """Every instance is the closest hit of at least 20 rays and 20 % - 80 % of the
    silhouette rays end on the instance they were aimed at (inside A's and B's
    enclosure every ray ends on something, so hitting anything says nothing).
    Achieved (fewest closest hits of an instance, that share): A 81 / 0.640,
    A2 112 / 0.649, Aalt 89 / 0.639, B1 21 / 0.580, B2 36 / 0.578, B64 20 / 0.622,
    B65 21 / 0.624, C 189 / 0.453 (its 1e-18 mesh: 0 hits, a defined miss: |a| <
    kEps for every ray, mesh.cpp:31), Ddeep 607 / 0.248, E0 295 / 0.399,
    E1 300 / 0.377, L1 145 / 0.634, L2 151 / 0.644, L1c 93 / 0.623, L2c 83 / 0.637."""
    per, sil = hit_figures(name)
    need = np.ones(len(per), bool)
    need[list(NO_HIT_NEEDED.get(name, ()))] = False
    print(f"{name}: fewest closest hits of an instance {per[need].min()}, silhouette hit share {sil:.3f}")
    assert per[need].min() >= 20, f"{name}: instance {int(np.argmin(np.where(need, per, 1 << 30)))} is the closest hit of {per[need].min()} rays"
    for i in NO_HIT_NEEDED.get(name, ()):
        assert per[i] == 0
    assert 0.2 <= sil <= 0.8, f"{name}: {sil:.3f} of the silhouette rays hit"


def test_duplicates_tie_on_t():
    """Scene C's instance 1 is a 128-triangle sphere stored twice: triangles p and
    p + 128 are equal, so every hit of one ties with the other and traversal
    order decides.  Brute force keeps the first (depthInBounds is strict);
    the BVH walk keeps whichever leaf it visits first.  Achieved: 630 rays end on
    the instance with brute force's t, 372 of them on another primitive than
    brute force's, 358 on the same triangle's second copy."""
    c = case("C")
    o, d = c.all_rays()
    t, _, _, inst, prim = c.oracle.trace_closest(o, d)
    tb, ib, pb = c.oracle.trace_brute(o, d)
    dup = (inst == 1) & (ib == 1) & (t == tb)
    assert (pb[dup] < 128).all()              # brute force keeps the first of equal depths
    tie = dup & (prim != pb)                  # two primitives, one t: the walk ended on the other one
    second = dup & (prim == pb + 128)
    print(f"duplicates: {dup.sum()} rays end on the doubled sphere, {tie.sum()} on another primitive than brute force, "
          f"{second.sum()} on the same triangle's second copy")
    assert tie.sum() >= 50 and second.sum() >= 50 and (dup & (prim == pb)).sum() >= 50


def _stack(c):
    t, b = c.oracle.bvh_depths()
    return t + b + 1


def test_each_scene_reaches_its_branch():
    """Read from the export and bvh_depths(): what each scene is named for."""
    row3 = np.array([0, 0, 0, 1], np.float32)
    # A: single-leaf TLAS; affine, projective and inexact-inverse rows; a condition number of ~1e6
    for name in ("A", "Aalt"):
        g = case(name).geometry
        assert case(name).oracle.bvh_depths()[0] == 0 and g.tlas_u[0, 1] == g.n == 19 and g.tlas_u[0, 0] == 0
        assert np.array_equal(g.tlas_idx, np.arange(19))
    g = case("A").geometry
    exact = (g.Minv[:, 3] == row3).all(1)
    m_affine = (g.M[:, 3] == row3).all(1)
    assert exact[[0, 1, 2, 3, 4, 5, 6, 7, 13, 14, 15, 16, 17, 18]].all(), exact
    assert not exact[[8, 9, 10, 11, 12]].any()
    assert not m_affine[[8, 9, 11, 12]].any() and m_affine[:8].all() and m_affine[10]
    # 10 is an affine M (rotation * scale * shear) whose f32 inverse is not: compute_inverse's cofactors of row 3
    # are exact zeros, but its last element is det3 * (1 / det), which rounds to 1 - 2^-24 here: instanceRay
    # divides, and the instance gets no cull box
    assert (g.Minv[10, 3, :3] == 0).all() and g.Minv[10, 3, 3] != 1.0 and abs(g.Minv[10, 3, 3] - 1.0) < 1e-6
    # 8 and 11 have row 3 = (0, 0, 0, w): the inverse has (0, 0, 0, 1 / w), 0.5 and 1/3 rounded; 9 and 12 are projective
    assert (g.Minv[8, 3] == np.array([0, 0, 0, 0.5], np.float32)).all()
    assert (g.Minv[11, 3, :3] == 0).all() and g.Minv[11, 3, 3] != 1.0
    assert np.abs(g.Minv[12, 3, :3]).min() > 0 and g.Minv[9, 3, 2] != 0
    lin = g.M[7][:3, :3]
    assert 3e5 < np.linalg.cond(lin) < 3e6
    assert np.linalg.det(g.M[4][:3, :3]) < 0
    galt = case("Aalt").geometry
    ealt = (galt.Minv[:, 3] == row3).all(1)
    assert exact[15] and not ealt[15] and not exact[8] and ealt[8] and not exact[9] and ealt[9]      # rows turn projective and back
    assert case("A").export["triangles"] == case("Aalt").export["triangles"] and case("A").export["blas_nodes"] == case("Aalt").export["blas_nodes"]
    assert case("A").export["instances"] != case("Aalt").export["instances"]
    # A2: the TLAS splits
    assert case("A2").oracle.bvh_depths()[0] >= 2 and case("A2").geometry.n == 16
    # B: root leaves of every size class, mixed leaves, runs
    for name, n, heads, members in (("B1", 51, [11, 43], 40), ("B2", 51, [11, 29], 39), ("B64", 64, [11, 43], 52), ("B65", 65, [], 0)):
        c = case(name)
        g = c.geometry
        assert c.oracle.bvh_depths()[0] == 0 and g.tlas_u[0, 1] == g.n == n and np.array_equal(g.tlas_idx, np.arange(n)), name
        assert g.root_count[3:10].tolist() == [1, 2, 3, 4, 127, 128, 200], name         # one root leaf each
        assert K_LEAF_IN_W in g.root_count[3:10] and K_LEAF_IN_W + 1 in g.root_count[3:10]
        assert K_PACK_LEAF - 1 in g.root_count[3:10] and K_PACK_LEAF in g.root_count[3:10]
        leaves = g.leaf_counts(10)                                                        # the ordinary mesh: mixed leaf sizes
        assert g.root_count[10] == 0 and sorted(np.unique(leaves).tolist()) == [1, 2, 3, 4, 5, 6, 9, 17, 40, 127, 128, 130], leaves
        # packLeaf (scene_upload.hip) packs a child leaf of fewer than 128 triangles and gives up above: both sides,
        # on leaves that are children of interior nodes (a root leaf never goes through it)
        assert (leaves == K_PACK_LEAF - 1).any() and (leaves >= K_PACK_LEAF).sum() == 2
        assert (g.root_count[11:] == 2).all()
        h, m = run_layout(g)
        assert h == heads and len(m) == members, (name, h, len(m))
    assert run_layout(case("B1").geometry)[1] == list(range(11, 51))             # 32 + 8
    # B1 -> B2 is the re-upload with another run layout: the same meshes and counts, other heads and members
    assert run_layout(case("B1").geometry) != run_layout(case("B2").geometry)
    for k in ("triangles", "tri_ext", "blas_indices", "blas_nodes", "materials", "lights"):
        assert case("B1").export[k] == case("B2").export[k], k
    assert len(case("B1").export["tlas_nodes"]) == len(case("B2").export["tlas_nodes"])
    assert case("B1").export["instances"] != case("B2").export["instances"]
    assert 28 not in run_layout(case("B2").geometry)[1]                          # the projective copy (plane 17) breaks the run
    assert not (case("B2").geometry.Minv[28, 3] == row3).all()
    assert max(run_layout(case("B64").geometry)[1]) == K_RUN_POSITIONS - 1 and case("B64").geometry.root_count[63] == 2
    assert case("B64").geometry.n <= K_LDS_TABLES < case("B65").geometry.n
    # C: zero-area triangles, zero-extent boxes, the ends of the f32 range; Cnan: a non-finite box
    g = case("C").geometry
    z = g.tris[:400]
    assert (np.linalg.norm(np.cross(z[:, 1] - z[:, 0], z[:, 2] - z[:, 0]), axis=1) == 0).sum() >= 60
    flat = g.blas_nodes[g.node_offset[2]:g.node_offset[3]]
    assert (flat[:, 5] == 0).all() and (flat[:, 9] == 0).all() and len(flat) > 50           # every box of the grid has no height
    assert g.root_hi[3].max() > 1e18 and 0 < np.abs(g.tris[g.tri_offset[4]:]).max() < 2e-18
    assert np.isfinite(np.frombuffer(case("C").export["blas_nodes"], np.float32)).all()
    nodes = np.frombuffer(case("Cnan").export["blas_nodes"], np.float32).reshape(-1, 12)
    assert not np.isfinite(nodes[:, [4, 5, 6, 8, 9, 10]]).all()
    assert np.isnan(np.frombuffer(case("Cnan").export["triangles"], np.float32)).sum() == 2      # the vertex and its centroid
    # D: stack depth past the wave engines' 64 and within the upload's 120; past 120
    assert case("Ddeep").oracle.bvh_depths() == (0, 101) and K_WAVE_STACK < _stack(case("Ddeep")) <= K_MAX_STACK
    assert case("Dtoo").oracle.bvh_depths() == (0, 121) and K_MAX_STACK < _stack(case("Dtoo")) <= 128
    # E: the two sides of `< 65536` BLAS nodes, the soup's nodes the highest
    for name, total in (("E0", K_SK16 - 2), ("E1", K_SK16)):
        g = case(name).geometry
        assert len(g.blas_nodes) == total and g.node_offset[-1] == total - 65522 and g.tri_count[-1] == 34676, name
        assert (g.blas_node_counts()[:-1] == 2).all()
    # L: one shared emitter BLAS small enough to stage; two emitter BLASes
    for name, same in (("L1", True), ("L2", False), ("L1c", True), ("L2c", False)):
        c = case(name)
        g = c.geometry
        lights = np.frombuffer(c.export["lights"], np.uint32).reshape(-1, 2)
        assert lights[:, 0].tolist() == [14, 15] and c.oracle.bvh_depths()[0] >= 1
        assert (g.node_offset[14] == g.node_offset[15]) == same
        interior = int((g.blas_u[g.node_offset[14]:g.node_offset[14] + g.blas_node_counts()[14], 1] == 0).sum())
        assert interior * 64 + int(lights[0, 1]) * 48 <= 20480
        assert (g.Minv[15, 3] == row3).all() == same
