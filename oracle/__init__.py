"""ctypes binding of the CPU oracle (oracle/liboracle.so).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and the
cpu_baseline leg of bench.py -- never by the product package.  Parity status:
UNPINNED against a run of the reference (see oracle/cpu_ref.h).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "liboracle.so")
BENCH_BIN = os.path.join(HERE, "cpu_ref_bench")
ASSETS_DIR = os.path.join(os.path.dirname(HERE), "assets")


def build():
    subprocess.run(["make", "-s", "-C", HERE, "-j4"], check=True)


class Counters(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("n_ext", C.c_uint64), ("n_hit", C.c_uint64), ("n_cont", C.c_uint64),
                ("n_shadow", C.c_uint64), ("n_acc", C.c_uint64), ("n_unocc", C.c_uint64), ("max_segments", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        build()
    lib = C.CDLL(LIB_PATH)
    P, U32, I32, F, D = C.c_void_p, C.c_uint32, C.c_int, C.c_float, C.c_double
    sig = {
        "orc_scene_create": ([C.c_char_p, I32], P), "orc_scene_destroy": ([P], None),
        "orc_scene_create_custom": ([U32, P, P, P, P, U32, P, U32, P, P, P], P),
        "orc_scene_mesh_tris": ([P, P, I32], I32),
        "orc_scene_instance_count": ([P], U32), "orc_scene_light_count": ([P], U32),
        "orc_scene_set_camera": ([P, U32, U32], None), "orc_camera_ubo": ([P, P], None),
        "orc_scene_set_view": ([P, P, P, F, F, F], None),
        "orc_scene_set_background": ([P, I32, P, P, P], None),
        "orc_scene_set_material": ([P, U32, P, P, P, F, F, F, F], I32),
        "orc_scene_export": ([P, I32, P], C.c_uint64),
        "orc_render": ([P, U32, U32, U32, U32, U32, U32, U32, I32, P, C.POINTER(Counters)], D),
        "orc_render_spp": ([P, U32, U32, U32, U32, U32, U32, U32, U32, I32, P, C.POINTER(Counters)], D),
        "orc_trace_closest": ([P, U32, P, P, P, P, P, P, P], None),
        "orc_trace_any": ([P, U32, P, P, P, P], None),
        "orc_trace_brute": ([P, U32, P, P, P, P, P], None),
        "orc_trace_visits": ([P, U32, P, P, P, P], None),
        "orc_path_lengths": ([P, U32, U32, U32, P], None),
        "orc_scene_update": ([P, F], None),
        "orc_record_rays": ([P, U32, U32, U32, U32, U32, U32, P, P, P, U32, P, P, P, P], None),
        "orc_bvh_depths": ([P, C.POINTER(U32), C.POINTER(U32)], None),
        "orc_init_seed": ([U32], U32), "orc_random_u32": ([C.POINTER(U32)], U32),
        "orc_random_f32": ([C.POINTER(U32)], F),
        "orc_finalize_rgba8": ([P, U32, F, P], None),
        "orc_set_zero_cutoff": ([I32], None),
        "orc_bvh_build": ([P, U32, P, P], U32),
        "orc_obj_load": ([C.c_char_p, P, P, C.c_uint64], C.c_long),
        "orc_shade_census": ([P], None),
        "orc_trace_paths": ([P, U32, P, P, P, U32, P], None),
        "orc_libm_map": ([I32, C.c_uint64, P, P], I32),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data


def _f3(v):
    a = np.ascontiguousarray(v, np.float32)
    if a.shape != (3,):
        raise ValueError(f"{v!r} is not three floats")
    return a


# main.cpp:141-149 and :343-346
DEFAULT_VIEW = {"pos": (0.0, 0.0, -7.0), "target": (0.0, 0.0, 0.0), "fov_y": 70.0, "focal": 7.0, "defocus": 0.5}
DEFAULT_BACKGROUND = {"type": 1, "color": (0.0, 0.0, 0.0), "a": (0.8, 0.8, 0.8), "b": (0.1, 0.4, 0.6)}

EXPORT_ORDER = ["triangles", "tri_ext", "blas_indices", "blas_nodes", "materials", "instances",
                "tlas_indices", "tlas_nodes", "lights", "background"]


class OracleScene:
    def __init__(self, assets_dir: str = ASSETS_DIR, variant: int = 0):
        lib = load()
        self._h = lib.orc_scene_create(assets_dir.encode(), variant)
        if not self._h:
            raise RuntimeError(f"oracle could not load the scene from {assets_dir}")

    @classmethod
    def custom(cls, meshes, materials, instances, background=None, view=None) -> "OracleScene":
        """A caller's scene (orc_scene_create_custom).  meshes: per mesh (verts,
        normals), two (n, 3, 3) float32 arrays: the stored v0, v1, v2 of each
        triangle (a Triangle record's order) and n0, n1, n2; UVs are zero unless
        every mesh brings a third (n, 6) array.
        materials: dicts of materials()' seven fields (missing ones take
        Material's defaults, material.h:6-19).  instances: (mesh index, material
        index, M) with M a 4 x 4 array in mathematical layout (M[row][column]; it
        is stored column major as glm does).  background / view: the keyword
        arguments of set_background / set_view.  ValueError when the oracle
        refuses the scene (an index out of range, a non-finite matrix, an empty
        mesh, a tree deeper than 127)."""
        lib = load()
        cat = lambda k, w: (np.concatenate([np.asarray(m[k], np.float32).reshape(-1, w) for m in meshes]) if len(meshes)
                            else np.zeros((0, w), np.float32))
        tris = np.array([len(np.asarray(m[0]).reshape(-1, 3, 3)) for m in meshes], np.uint32)
        verts, norms = cat(0, 9), cat(1, 9)
        uvs = np.ascontiguousarray(cat(2, 6)) if len(meshes) and all(len(m) > 2 for m in meshes) else None
        if uvs is not None and len(uvs) != len(verts):
            raise ValueError("a mesh's vertex and UV arrays differ in length")
        if verts.shape != norms.shape:
            raise ValueError("a mesh's vertex and normal arrays differ in shape")
        verts, norms = np.ascontiguousarray(verts), np.ascontiguousarray(norms)
        mats = np.zeros((len(materials), 16), np.float32)
        for r, m in zip(mats, materials):
            unknown = [k for k in m if k not in ("emit", "refl", "refr", "ior", "emit_color", "albedo", "absorption")]
            if unknown:
                raise TypeError(f"unknown material field {unknown[0]!r}")
            r[0], r[1], r[2], r[3] = m.get("emit", 0.0), m.get("refl", 0.0), m.get("refr", 0.0), m.get("ior", 1.0)
            r[4:7], r[8:11], r[12:15] = (_f3(m.get(k, (0.0, 0.0, 0.0))) for k in ("emit_color", "albedo", "absorption"))
        im = np.array([i[0] for i in instances], np.int64)
        ia = np.array([i[1] for i in instances], np.int64)
        if len(instances) and (im.min() < 0 or ia.min() < 0 or im.max() > 0xFFFFFFFF or ia.max() > 0xFFFFFFFF):
            raise ValueError("instance index out of range")
        im, ia = im.astype(np.uint32), ia.astype(np.uint32)
        # M[row][column] -> column-major storage: element 4 * column + row
        mm = np.ascontiguousarray(np.array([np.asarray(i[2], np.float32).reshape(4, 4).T for i in instances], np.float32).reshape(-1, 16))
        h = lib.orc_scene_create_custom(len(tris), _p(tris), _p(verts), _p(norms), None if uvs is None else _p(uvs), len(mats), _p(mats), len(im), _p(im), _p(ia), _p(mm))
        if not h:
            raise ValueError("oracle refused the custom scene")
        self = cls.__new__(cls)
        self._h = h
        if background is not None:
            self.set_background(**background)
        if view is not None:
            self.set_view(**view)
        return self

    def mesh_tris(self):
        out = np.zeros(8, np.uint32)
        n = load().orc_scene_mesh_tris(self._h, _p(out), 8)
        return [int(x) for x in out[:n]]

    def instance_count(self):
        return load().orc_scene_instance_count(self._h)

    def light_count(self):
        return load().orc_scene_light_count(self._h)

    def camera_ubo(self, width, height) -> bytes:
        load().orc_scene_set_camera(self._h, width, height)
        buf = (C.c_uint8 * 128)()
        load().orc_camera_ubo(self._h, buf)
        return bytes(buf)

    def set_view(self, pos=DEFAULT_VIEW["pos"], target=DEFAULT_VIEW["target"], fov_y=DEFAULT_VIEW["fov_y"],
                 focal=DEFAULT_VIEW["focal"], defocus=DEFAULT_VIEW["defocus"]):
        """Camera::Camera's arguments (camera.h:31); kept for every later camera_ubo()
        and render, of any resolution.  The defaults are main.cpp:141-149."""
        pos, target = _f3(pos), _f3(target)
        load().orc_scene_set_view(self._h, _p(pos), _p(target), fov_y, focal, defocus)

    def set_background(self, type=DEFAULT_BACKGROUND["type"], color=DEFAULT_BACKGROUND["color"],
                       a=DEFAULT_BACKGROUND["a"], b=DEFAULT_BACKGROUND["b"]):
        """SceneBackground (scene.h:18-26): type 0 solid colour, 1 gradient from a to b,
        other black.  The defaults are main.cpp:343-346."""
        color, a, b = _f3(color), _f3(a), _f3(b)
        load().orc_scene_set_background(self._h, int(type), _p(color), _p(a), _p(b))

    def materials(self) -> list[dict]:
        """The Material records (material.h:6-19) in export()'s first-use order."""
        m = np.frombuffer(self.export()["materials"], np.float32).reshape(-1, 16)
        return [{"emit": float(r[0]), "refl": float(r[1]), "refr": float(r[2]), "ior": float(r[3]),
                 "emit_color": tuple(map(float, r[4:7])), "albedo": tuple(map(float, r[8:11])),
                 "absorption": tuple(map(float, r[12:15]))} for r in m]

    def set_material(self, index, **fields):
        """Replaces the given fields (materials()' names) of material `index` in export()'s
        first-use order; the light list is collected again (scene.cpp:22-32)."""
        cur = self.materials()
        if not 0 <= index < len(cur):
            raise IndexError(f"material {index}: the scene uses {len(cur)}")
        unknown = [k for k in fields if k not in cur[index]]
        if unknown:
            raise TypeError(f"unknown material field {unknown[0]!r}")
        m = dict(cur[index], **fields)
        albedo, absorption, emit_color = _f3(m["albedo"]), _f3(m["absorption"]), _f3(m["emit_color"])
        rc = load().orc_scene_set_material(self._h, index, _p(albedo), _p(absorption), _p(emit_color),
                                           m["emit"], m["refl"], m["refr"], m["ior"])
        assert rc == 0, rc

    def export(self) -> dict[str, bytes]:
        out = {}
        for i, k in enumerate(EXPORT_ORDER):
            n = load().orc_scene_export(self._h, i, None)
            buf = (C.c_uint8 * max(int(n), 1))()
            load().orc_scene_export(self._h, i, buf)
            out[k] = bytes(buf)[: int(n)]
        return out

    def render(self, width, height, frames, first_frame=0, rows=None, max_segments=0, threads=0, spp=1):
        """`frames` frames of `spp` samples per pixel (Renderer::render with
        samplesPerFrame = spp); first_frame is the sample count before the first
        frame (the accumulator's totalSamples; the frame index when spp = 1)."""
        r0, r1 = (0, height) if rows is None else rows
        acc = np.zeros((r1 - r0, width, 4), np.float32)
        cnt = Counters()
        secs = load().orc_render_spp(self._h, width, height, r0, r1, first_frame, frames, spp, max_segments, threads,
                                     _p(acc), C.byref(cnt))
        return acc, cnt.as_dict(), secs

    def trace_closest(self, o, d):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        t, u, v = (np.zeros(n, np.float32) for _ in range(3))
        inst, prim = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        load().orc_trace_closest(self._h, n, _p(o), _p(d), _p(t), _p(u), _p(v), _p(inst), _p(prim))
        return t, u, v, inst, prim

    def trace_any(self, o, d, tmax):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        tmax = np.ascontiguousarray(tmax, np.float32)
        occ = np.zeros(len(o), np.uint8)
        load().orc_trace_any(self._h, len(o), _p(o), _p(d), _p(tmax), _p(occ))
        return occ

    def trace_brute(self, o, d):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        n = len(o)
        t = np.zeros(n, np.float32)
        inst, prim = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        load().orc_trace_brute(self._h, n, _p(o), _p(d), _p(t), _p(inst), _p(prim))
        return t, inst, prim

    def trace_visits(self, o, d):
        """Per ray and instance: BLAS node visits and triangle tests of the closest-hit traversal."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        ni = self.instance_count()
        nodes, tris = np.zeros((len(o), ni), np.uint32), np.zeros((len(o), ni), np.uint32)
        load().orc_trace_visits(self._h, len(o), _p(o), _p(d), _p(nodes), _p(tris))
        return nodes, tris

    def trace_paths(self, o, d, seeds, max_segments=0):
        """Planted paths (orc_trace_paths): trace() from each origin, direction
        and RNG state.  Returns (energy (n, 3) float32, segments (n,) uint32,
        final seeds (n,) uint32); follows set_zero_cutoff."""
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        s = np.array(seeds, np.uint32).reshape(-1)
        if not (len(o) == len(d) == len(s)):
            raise ValueError("trace_paths: origins, directions and seeds differ in length")
        out = np.zeros((len(o), 4), np.float32)
        load().orc_trace_paths(self._h, len(o), _p(o), _p(d), _p(s), max_segments, _p(out))
        return out[:, :3].copy(), out[:, 3].copy().view(np.uint32), s

    def update(self, dt: float):
        """GPUScene::update: rotate instance 3 by dt radians about +y, refit the TLAS."""
        load().orc_scene_update(self._h, dt)

    def path_lengths(self, width, height, frame):
        """Extension rays per pixel path of one frame (diagnostics)."""
        out = np.zeros(width * height, np.uint32)
        load().orc_path_lengths(self._h, width, height, frame, _p(out))
        return out.reshape(height, width)

    def record_rays(self, width, height, frame, pix_begin, pix_end, max_ext=1 << 20, max_shadow=1 << 20):
        eo, ed = np.zeros((max_ext, 3), np.float32), np.zeros((max_ext, 3), np.float32)
        so, sd = np.zeros((max_shadow, 3), np.float32), np.zeros((max_shadow, 3), np.float32)
        st = np.zeros(max_shadow, np.float32)
        ne, ns = C.c_uint32(), C.c_uint32()
        load().orc_record_rays(self._h, width, height, frame, pix_begin, pix_end, max_ext, _p(eo), _p(ed), C.byref(ne),
                               max_shadow, _p(so), _p(sd), _p(st), C.byref(ns))
        return (eo[: ne.value], ed[: ne.value]), (so[: ns.value], sd[: ns.value], st[: ns.value])

    def bvh_depths(self):
        t, b = C.c_uint32(), C.c_uint32()
        load().orc_bvh_depths(self._h, C.byref(t), C.byref(b))
        return t.value, b.value

    def close(self):
        if self._h:
            load().orc_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def set_zero_cutoff(on: bool):
    """Radiance-neutral early end of zero-throughput paths (default off = reference)."""
    load().orc_set_zero_cutoff(1 if on else 0)


CENSUS = ("medium_segments", "exp_below_60", "exp_denormal", "exp_zero", "dielectric_outside", "tir_outside", "tir_inside",
          "fresnel_reflect", "refract", "mirror", "diffuse", "rr_clamped", "rr_zero", "cutoff_kills", "cosine_retries")


def shade_census() -> dict:
    """The shading census (orc_shade_census) of every trace since the last call,
    by name; reading resets it."""
    out = np.zeros(len(CENSUS), np.uint64)
    load().orc_shade_census(_p(out))
    return {k: int(v) for k, v in zip(CENSUS, out)}


LIBM_OPS = ("expf", "sinf", "cosf")


def libm(op: str, x) -> np.ndarray:
    """This machine's glibc expf / sinf / cosf over a float32 array (orc_libm_map)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.empty_like(x)
    rc = load().orc_libm_map(LIBM_OPS.index(op), len(x), _p(x), _p(out))
    assert rc == 0, rc
    return out


def init_seed(s: int) -> int:
    return load().orc_init_seed(s)


def random_u32_stream(seed: int, n: int) -> list[int]:
    s = C.c_uint32(seed)
    return [load().orc_random_u32(C.byref(s)) for _ in range(n)]


def finalize_rgba8(acc: np.ndarray, inv_samples: float) -> np.ndarray:
    acc = np.ascontiguousarray(acc, np.float32).reshape(-1, 4)
    out = np.zeros(len(acc), np.uint32)
    load().orc_finalize_rgba8(_p(acc), len(acc), inv_samples, _p(out))
    return out


def bvh_build(tris: np.ndarray):
    """Sequential reference BLAS build over (n, 16) float32 Triangle records
    (v0, v1, v2, centroid at 16-B strides).  Returns (indices (n,) u32,
    nodes (used, 12) float32 view of the 48-B BvhNode records)."""
    tris = np.ascontiguousarray(tris, dtype=np.float32)
    n = tris.shape[0]
    idx = np.empty(n, np.uint32)
    nodes = np.zeros((2 * n, 12), np.float32)
    used = load().orc_bvh_build(_p(tris), n, _p(idx), _p(nodes))
    return idx, nodes[:used]


def obj_load(path: str):
    """Mesh(path) with tinyobj semantics: ((n, 16) float32 Triangle records,
    (n, 20) float32 TriExtension records)."""
    n = load().orc_obj_load(path.encode(), None, None, 0)
    if n < 0:
        raise OSError(f"oracle: cannot read {path}")
    tris = np.zeros((n, 16), np.float32)
    ext = np.zeros((n, 20), np.float32)
    load().orc_obj_load(path.encode(), _p(tris), _p(ext), n)
    return tris, ext

