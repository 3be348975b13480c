"""The oracle's scene edits (orc_scene_set_view / _set_background / _set_material)
and the scenarios built from them, on the CPU.

Every render parity test used to compare the GPU with the oracle on one
picture: the closed room from main.cpp's camera, where one sample in 600 slips
out between two walls and sees the gradient sky (15 of 9,216 at 64 x 48 x 3)
and no other ever misses, the lens is a pure dielectric and both lights are
12-triangle cubes.  The
scenarios below leave that picture; tests/test_gpu_scene_edges.py renders
them on the GPU.  This file pins what those tests stand on:

  * the setters with their default arguments change no bit;
  * the product-side patch (PatchedScene: the product's own ten buffers with
    the material, light and background records edited by the field offsets
    of include/surf_hip.h) and the oracle's setters give the same buffers;
  * the background expression, against a numpy float32 restatement that
    shares no code with the oracle;
  * BVH closest hit == brute force for a moved camera's rays;
  * each scenario reaches what it is there for (misses, shadow rays, light
    counts), and no path in it is long enough to stall a GPU.

The scenarios (material indices are the export's first-use order: 0 floor,
1 cubeL's light, 2 cubeR's light, 3 Suzanne 0, 4 Suzanne 1, 5 lens, 6 red
wall, 7 green wall):

  A  the view shifted by (0, 6, -12) -- from (0, 6, -19) toward (0, 6, -12),
     outside the room in front of its front wall -- defocus 0.5, gradient sky.
  B  the same position as a pinhole (defocus 0), fov 45, a solid orange sky;
     B2 the same with a background type that is neither 0 nor 1 (black).
  C  default view; the green wall becomes a clear pane (refr 1, ior 1,
     albedo 1), the lens refl 0.2 / refr 0.7 with its albedo, absorption and
     ior kept.
  D  C with both emitters switched off: no lights, a sky-lit room.
  E  default view; Suzanne 0 becomes an emitter (strength 2, colour
     (1, 0.6, 0.3)): three lights, one with a 15,744-triangle BLAS.
  F .. J  material extremes under the default view (EXTREMES; what each is
     there for stands beside its floors in CENSUS_FLOORS): absorption that
     drives expf into its denormal and zero range, an ior below 1 and one of
     3, refl + refr > 1 and refl == 1, a medium inside a heavy BLAS, albedo
     channels above 1, at 0 and below 0, an emitter strength that is a
     denormal, and a non-emitter with emit > 0 and a black colour.  Their
     conditions are counts of the oracle's shading census (oracle.shade_census).
"""
import os

import numpy as np
import pytest

import oracle
import surf_amd
from test_host_scene import MASK

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
UNSET = 0xFFFFFFFF
F = np.float32

M_FLOOR, M_CUBE_L, M_CUBE_R, M_SUZANNE0, M_LENS, M_WALL_RED, M_WALL_GREEN = 0, 1, 2, 3, 5, 6, 7

OUTSIDE = {"pos": (0.0, 6.0, -19.0), "target": (0.0, 6.0, -12.0)}
PANE = {"refl": 0.0, "refr": 1.0, "ior": 1.0, "albedo": (1.0, 1.0, 1.0), "absorption": (0.0, 0.0, 0.0)}
MIXED_LENS = {"refl": 0.2, "refr": 0.7}
OFF = {"emit": 0.0}

SCENARIOS = {
    "A": {"view": dict(OUTSIDE, fov_y=70.0, focal=7.0, defocus=0.5)},
    "B": {"view": dict(OUTSIDE, fov_y=45.0, focal=7.0, defocus=0.0),
          "background": {"type": 0, "color": (0.9, 0.5, 0.2)}},
    "B2": {"view": dict(OUTSIDE, fov_y=45.0, focal=7.0, defocus=0.0),
           "background": {"type": 2, "color": (0.9, 0.5, 0.2)}},
    "C": {"materials": {M_WALL_GREEN: PANE, M_LENS: MIXED_LENS}},
    "D": {"materials": {M_WALL_GREEN: PANE, M_LENS: MIXED_LENS, M_CUBE_L: OFF, M_CUBE_R: OFF}},
    "E": {"materials": {M_SUZANNE0: {"emit": 2.0, "emit_color": (1.0, 0.6, 0.3)}}},
    # material extremes (default view): what each is there for is in CENSUS_FLOORS
    "F": {"materials": {M_LENS: {"absorption": (40.0, 8.0, 200.0)}}},
    "G": {"materials": {M_LENS: {"ior": 0.6}}},
    "G2": {"materials": {M_LENS: {"ior": 3.0}}},
    "H": {"materials": {M_LENS: {"refl": 0.6, "refr": 0.9}, M_SUZANNE0: {"refl": 1.0},
                        M_WALL_RED: {"refl": 0.3, "refr": 0.3, "ior": 1.0}}},
    "H2": {"materials": {M_SUZANNE0: {"refl": 0.1, "refr": 0.9, "ior": 1.5, "albedo": (0.9, 0.9, 0.9),
                                      "absorption": (30.0, 3.0, 120.0)}}},
    "H3": {"materials": {M_SUZANNE0: {"refr": 1.0, "ior": 0.7, "absorption": (1.0, 0.1, 5.0)}}},
    "I": {"materials": {M_SUZANNE0: {"albedo": (1.6, 1.2, 0.0)}, M_WALL_RED: {"albedo": (1.3, 0.1, 0.1)}}},
    "I2": {"materials": {M_SUZANNE0: {"albedo": (-0.5, 0.5, 0.0)}, M_FLOOR: {"albedo": (0.0, 0.0, 0.0)}}},
    "J": {"materials": {M_SUZANNE0: {"emit": 3.0, "emit_color": (0.0, 0.0, 0.0)},
                        M_WALL_RED: {"emit": 1e-40, "emit_color": (1.0, 1.0, 1.0)}}},
}
EXTREMES = ("F", "G", "G2", "H", "H2", "H3", "I", "I2", "J")

# include/surf_hip.h: surf_material and surf_background, byte offsets
MATERIAL_AT = {"emit": (0, 1), "refl": (4, 1), "refr": (8, 1), "ior": (12, 1), "emit_color": (16, 3), "albedo": (32, 3),
               "absorption": (48, 3)}
BACKGROUND_AT = {"color": (16, 3), "a": (32, 3), "b": (48, 3)}


def edited_oracle(spec) -> "oracle.OracleScene":
    """A fresh oracle scene with the scenario's setters applied."""
    o = oracle.OracleScene()
    if "view" in spec:
        o.set_view(**spec["view"])
    if "background" in spec:
        o.set_background(**spec["background"])
    for index, fields in spec.get("materials", {}).items():
        o.set_material(index, **fields)
    return o


class PatchedScene:
    """What Renderer.__init__ needs of a scene (desc()), over copies of the product
    scene's ten buffers with the scenario's material and background records
    edited in place and the light list collected again: every instance, in
    instance order, whose material is an emitter (Material::isLight,
    material.h), with the triangle count of its mesh.  It owns the arrays the
    descriptor points into; the camera comes from the oracle (Renderer(camera=))."""

    def __init__(self, product_scene, spec):
        src = product_scene.desc()
        a = {k: np.frombuffer(v, np.uint8).copy() for k, v in product_scene.buffers().items()}
        mats = a["materials"].reshape(-1, 64)
        for index, fields in spec.get("materials", {}).items():
            for name, value in fields.items():
                at, n = MATERIAL_AT[name]
                mats[index, at:at + 4 * n] = np.asarray(value, np.float32).reshape(n).view(np.uint8)
        bg = spec.get("background", {})
        if "type" in bg:
            a["background"][0:4] = np.array([bg["type"]], np.uint32).view(np.uint8)
        for name, (at, n) in BACKGROUND_AT.items():
            if name in bg:
                a["background"][at:at + 4 * n] = np.asarray(bg[name], np.float32).reshape(n).view(np.uint8)
        inst = a["instances"].view(np.uint32).reshape(-1, 40)          # tri_offset @0, material_offset @12
        m = mats.view(np.float32).reshape(-1, 16)
        starts = np.unique(np.append(inst[:, 0], src.triangle_count))  # each mesh's first triangle, and the end
        lights = []
        for i, rec in enumerate(inst):
            strength, colour = m[rec[3], 0], m[rec[3], 4:7]
            if strength > 0.0 and (colour > 0.0).any():
                lights.append((i, starts[np.searchsorted(starts, rec[0]) + 1] - rec[0]))
        a["lights"] = np.array(lights, np.uint32).reshape(-1, 2).view(np.uint8).reshape(-1)
        self._arrays = a
        d = surf_amd.SceneDesc()
        for name, _ in surf_amd.SceneDesc._fields_:
            if name.endswith("_count"):
                setattr(d, name, getattr(src, name))
            else:
                setattr(d, name, a[name].ctypes.data if a[name].size else None)
        d.light_count = len(lights)
        self._desc = d

    def desc(self):
        return self._desc

    def buffers(self):
        return {k: v.tobytes() for k, v in self._arrays.items()}


def assert_buffers_equal(a, b, what):
    for buf, (rec, ranges) in MASK.items():
        assert len(a[buf]) == len(b[buf]) and len(a[buf]) % rec == 0, f"{what}: {buf}: {len(a[buf])} vs {len(b[buf])} bytes"
        x = np.frombuffer(a[buf], np.uint8).reshape(-1, rec)
        y = np.frombuffer(b[buf], np.uint8).reshape(-1, rec)
        for lo, hi in ranges:
            assert np.array_equal(x[:, lo:hi], y[:, lo:hi]), f"{what}: {buf} bytes {lo}:{hi}"


def render_counted(o, W, H, frames, spp=1):
    """The oracle's render with the throughput cutoff on (what the GPU traces by
    default): (acc, counters).  counters["census"] is the shading census
    (oracle.shade_census) of this render alone."""
    oracle.set_zero_cutoff(True)
    try:
        oracle.shade_census()                       # reading resets it
        acc, cnt, _ = o.render(W, H, frames, spp=spp)
        cnt["census"] = oracle.shade_census()
    finally:
        oracle.set_zero_cutoff(False)
    return acc, cnt


# Census floors of the material-extreme scenarios: (what the scenario is there
# for, the value the committed oracle reports at 64 x 48 x 3 with the cutoff on,
# the floor asserted -- about half of it, so that the branch is well taken in
# any render the GPU tests ask for; the 2 x 4-sample renders of F, H2 and H3
# count more than the 3-frame ones in every row).
CENSUS_FLOORS = {
    # expf into the denormal and zero range: lens absorption (40, 8, 200)
    "F": {"exp_denormal": (113, 50), "exp_zero": (400, 200), "exp_below_60": (636, 300)},
    # total internal reflection on entry: an ior below 1
    "G": {"tir_outside": (307, 150), "refract": (160, 80)},
    "G2": {"tir_inside": (1468, 700), "fresnel_reflect": (197, 100)},
    # refl + refr > 1 (the dielectric branch takes what the mirror leaves) and refl == 1
    "H": {"mirror": (6675, 3000), "dielectric_outside": (1702, 800)},
    # a medium inside a heavy BLAS
    "H2": {"medium_segments": (1751, 800), "exp_zero": (433, 200), "tir_inside": (802, 400)},
    "H3": {"tir_outside": (336, 150), "tir_inside": (330, 150)},
    # albedo above 1: the roulette probability pinned at 1 under a growing throughput
    # (cutoff_kills 0, brightest accumulator value 246)
    "I": {"rr_clamped": (10595, 5000)},
    # negative and zero albedo channels (negative radiance, asserted below)
    "I2": {"cutoff_kills": (8874, 4000)},
    # J: isLight's edge cases, asserted from the light list below
    "J": {},
}
assert all(0 < floor <= seen for rows in CENSUS_FLOORS.values() for seen, floor in rows.values())


def check_conditions(name, o, cnt, acc):
    """The conditions a scenario's render must meet to be worth a GPU run, from
    the oracle's counters and census: what it is there to reach, a finite
    accumulator, and no path past 4096 segments (one that never ends must not
    reach a GPU).

    No scenario puts a NaN in a material field: a NaN made by x86 arithmetic
    and one made by gfx950 arithmetic differ in sign, so bit-for-bit equality
    is undefined there."""
    miss = (cnt["n_ext"] - cnt["n_hit"]) / cnt["samples"]
    assert cnt["max_segments"] <= 4096, f"{name}: longest path {cnt['max_segments']} segments"
    assert np.isfinite(acc).all(), f"{name}: a non-finite accumulator word"
    if name in CENSUS_FLOORS:
        census = cnt["census"]
        for key, (_, floor) in CENSUS_FLOORS[name].items():
            assert census[key] >= floor, f"{name}: {key} {census[key]} < {floor} ({census})"
    if name == "I2":
        assert (acc[..., :3] < 0).any(), "I2: no negative accumulator word"
    if name == "J":
        lights = np.frombuffer(o.export()["lights"], np.uint32).reshape(-1, 2)[:, 0].tolist()
        assert o.light_count() == 3 and 3 not in lights and 6 in lights, lights
    if name in ("A", "B", "B2"):
        assert miss >= 0.25, f"{name}: {miss:.3f} misses per sample"
    if name in ("C", "D"):
        assert miss >= 0.05, f"{name}: {miss:.3f} misses per sample"
    if name == "C":
        assert cnt["n_shadow"] > 0
    if name == "D":
        assert o.light_count() == 0 and cnt["n_shadow"] == 0 and cnt["n_unocc"] == 0
        assert (acc[..., :3] > 0).any(), "D: a black image"
    if name == "E":
        assert o.light_count() == 3 and cnt["n_unocc"] > 0
    return miss


# ---- 1. the setters' defaults change nothing ----------------------------------

def test_default_arguments_change_no_bit(oracle_scene):
    g = np.load(os.path.join(GOLDEN, "oracle_32x24x2.npz"))
    o = oracle.OracleScene()
    try:
        before = o.export()
        ubos = {wh: o.camera_ubo(*wh) for wh in ((1280, 720), (64, 48), (100, 37))}
        o.set_view()
        o.set_background()
        for index, m in enumerate(o.materials()):
            o.set_material(index, **m)
        o.set_material(M_LENS)
        after = o.export()
        assert list(after) == list(before)
        for k in before:
            assert after[k] == before[k], k
        assert after == oracle_scene.export()
        for wh, ubo in ubos.items():
            assert o.camera_ubo(*wh) == ubo == oracle_scene.camera_ubo(*wh), wh
        acc, cnt, _ = o.render(32, 24, 2)
        assert np.array_equal(acc.view(np.uint32), g["acc"].view(np.uint32))
        assert [cnt[k] for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")] == list(g["counts"])
        with pytest.raises(IndexError):
            o.set_material(8)
        with pytest.raises(TypeError):
            o.set_material(0, colour=(1, 1, 1))
    finally:
        o.close()


def test_view_persists_across_resolutions_and_returns():
    """The stored view builds every later camera (camera_ubo and the renders'
    own resolution switch), takes effect at the current resolution at once, and
    setting the defaults again gives the default picture back."""
    o = oracle.OracleScene()
    try:
        plain, _, _ = o.render(32, 24, 1)
        default_ubo = o.camera_ubo(32, 24)
        o.set_view(**SCENARIOS["B"]["view"])        # the resolution is still 32 x 24: no setCamera in render
        moved, _, _ = o.render(32, 24, 1)
        assert not np.array_equal(moved, plain)
        u = np.frombuffer(o.camera_ubo(48, 40), np.float32)
        assert tuple(u[0:3]) == OUTSIDE["pos"] and tuple(u[8:11]) == (0.0, 0.0, 1.0)
        assert tuple(u[28:32]) == (48.0, 40.0, 7.0, 0.0)
        # camera.cpp:28-46: the view plane's height is 2 tan(fovY / 2) focal, its centre focal ahead
        assert abs(np.linalg.norm(u[24:27]) - 2.0 * np.tan(np.radians(45.0) / 2.0) * 7.0) < 1e-5
        centre = u[16:19] + 0.5 * (u[20:23] * (1 - 1 / 48) + u[24:27] * (1 - 1 / 40))
        assert np.allclose(centre, (0.0, 6.0, -12.0), atol=1e-5)
        again, _, _ = o.render(32, 24, 1)           # back from 48 x 40: rebuilt from the stored view
        assert np.array_equal(again.view(np.uint32), moved.view(np.uint32))
        o.set_view()
        assert o.camera_ubo(32, 24) == default_ubo
        back, _, _ = o.render(32, 24, 1)
        assert np.array_equal(back.view(np.uint32), plain.view(np.uint32))
    finally:
        o.close()


# ---- 2. the product-side patch and the oracle's setters agree ------------------

@pytest.mark.parametrize("name", list(SCENARIOS))
def test_patched_buffers_equal_the_edited_export(product_scene, name):
    spec = SCENARIOS[name]
    o = edited_oracle(spec)
    try:
        p = PatchedScene(product_scene, spec)
        want, got = o.export(), p.buffers()
        assert_buffers_equal(want, got, name)
        d = p.desc()
        assert d.light_count == o.light_count() == len(want["lights"]) // 8
        assert (d.triangle_count, d.instance_count, d.material_count) == (16894, 11, 8)
        mats = np.frombuffer(want["materials"], np.float32).reshape(-1, 16)
        for index, fields in spec.get("materials", {}).items():
            for k, v in fields.items():
                at, n = MATERIAL_AT[k]
                assert np.array_equal(mats[index, at // 4:at // 4 + n], np.asarray(v, np.float32).reshape(n)), (index, k)
        lights = np.frombuffer(want["lights"], np.uint32).reshape(-1, 2).tolist()
        # J: Suzanne 0 (instance 3, emit 3 with a black colour) is no light; the red wall (instance 6, a
        # denormal strength with colour 1) is one
        assert lights == {"D": [], "E": [[1, 188], [2, 188], [3, 15744]],
                          "J": [[1, 188], [2, 188], [6, 2]]}.get(name, [[1, 188], [2, 188]])
        bg = np.frombuffer(want["background"], np.uint32)
        assert bg[0] == spec.get("background", {}).get("type", 1)
    finally:
        o.close()
    # the unedited scene is untouched by the patch
    assert_buffers_equal(product_scene.buffers(), oracle.OracleScene().export(), "after the patch")


# ---- 3. the background, independent of the oracle's expression -----------------

SKY = {"pos": (0.0, 30.0, -19.0), "target": (0.0, 60.0, -12.0), "fov_y": 45.0, "focal": 7.0, "defocus": 0.0}


@pytest.mark.parametrize("bg", [{"type": 0, "color": (0.9, 0.5, 0.2)}, {"type": 1, "a": (0.7, 0.9, 0.3), "b": (0.2, 0.1, 0.8)},
                                {"type": 2, "color": (0.9, 0.5, 0.2)}], ids=["colour", "gradient", "black"])
def test_background_radiance_of_a_view_of_the_sky(bg):
    """A pinhole above the room that looks up: every path is one missed segment,
    so a pixel's radiance is the background along its primary ray -- the
    expression of scene.cpp:35-51 restated in numpy float32 on the rays
    record_rays returns -- and an spp = 3 frame sums three of them in order."""
    W, H = 40, 30
    o = oracle.OracleScene()
    try:
        o.set_view(**SKY)
        o.set_background(**bg)
        a, b, colour = (np.asarray(bg.get(k, oracle.DEFAULT_BACKGROUND[k]), np.float32) for k in ("a", "b", "color"))

        def sky(d):
            if bg["type"] == 0:
                return np.broadcast_to(colour, d.shape)
            if bg["type"] == 1:
                alpha = F(0.5) * (F(1.0) + d[:, 1])
                return alpha[:, None] * b + (F(1.0) - alpha)[:, None] * a
            return np.zeros_like(d)

        acc, cnt, _ = o.render(W, H, 1)
        assert cnt["n_ext"] == cnt["samples"] == W * H and cnt["n_hit"] == 0 and cnt["n_acc"] == W * H
        (eo, ed), (so, _, _) = o.record_rays(W, H, 0, 0, W * H)
        assert len(eo) == W * H and len(so) == 0
        assert (eo == np.asarray(SKY["pos"], np.float32)).all() and (ed[:, 1] > 0.5).all()
        want = sky(ed)
        assert want.dtype == np.float32
        assert np.array_equal(acc[..., :3].reshape(-1, 3).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))
        assert np.all(acc[..., 3] == 1.0)
        if bg["type"] != 2:
            assert (acc[..., :3] > 0).all()
        if bg["type"] == 1:
            assert len(np.unique(acc[..., 0])) > H // 2, "the gradient should vary down the image"
        # spp = 3: one frame of three chained samples, summed in sample order (the gradient's
        # sum is rebuilt exactly in test_spp_chain_of_a_pinhole_sky_view_equals_numpy)
        acc3, cnt3, _ = o.render(W, H, 1, spp=3)
        assert cnt3["samples"] == 3 * W * H == cnt3["n_ext"] and cnt3["n_hit"] == 0
        assert np.all(acc3[..., 3] == 3.0)
        if bg["type"] == 0:
            three = (np.zeros(3, np.float32) + colour + colour) + colour
            assert (acc3[..., :3] == three).all()
        elif bg["type"] == 2:
            assert (acc3[..., :3] == 0).all()
    finally:
        o.close()


def test_spp_chain_of_a_pinhole_sky_view_equals_numpy():
    """spp = 3 on the gradient sky, exactly: the three samples of a pixel draw two
    jitters each from one xorshift stream (surf_math.cpp:44-63, renderer.cpp:169-177:
    y first), so their rays can be rebuilt from the camera UBO in numpy float32."""
    W, H = 16, 10
    o = oracle.OracleScene()
    try:
        o.set_view(**SKY)
        bgA, bgB = (np.asarray(oracle.DEFAULT_BACKGROUND[k], np.float32) for k in ("a", "b"))
        u = np.frombuffer(o.camera_ubo(W, H), np.float32)
        pos, first, uvec, vvec = u[0:3], u[16:19], u[20:23], u[24:27]
        inv_w, inv_h = F(1.0) / F(W), F(1.0) / F(H)
        acc3, _, _ = o.render(W, H, 1, spp=3)
        for p in range(0, W * H, 7):
            x, y = p % W, p // W
            seed = oracle.init_seed(p)
            draws = oracle.random_u32_stream(seed, 6)
            e = np.zeros(3, np.float32)
            for s in range(3):
                r = [F(d) * F(2.3283064365387e-10) for d in draws[2 * s:2 * s + 2]]
                jy, jx = r[0] * (F(0.5) - F(-0.5)) + F(-0.5), r[1] * (F(0.5) - F(-0.5)) + F(-0.5)
                uu, vv = (F(x) + jx) * inv_w, (F(y) + jy) * inv_h
                d = ((first + uu * uvec) + vv * vvec) - pos
                d = d * (F(1.0) / np.sqrt(((F(0.0) + d[0] * d[0]) + d[1] * d[1]) + d[2] * d[2]))
                alpha = F(0.5) * (F(1.0) + d[1])
                e = e + (alpha * bgB + (F(1.0) - alpha) * bgA)
            assert e.dtype == np.float32
            assert np.array_equal(acc3[y, x, :3].view(np.uint32), e.view(np.uint32)), (p, acc3[y, x, :3], e)
    finally:
        o.close()


# ---- 4. BVH closest hit == brute force for a moved camera's rays ---------------

def test_moved_camera_rays_closest_equals_brute_force():
    o = edited_oracle(SCENARIOS["A"])
    try:
        (eo, ed), _ = o.record_rays(64, 48, 0, 0, 64 * 48)
        assert len(eo) > 64 * 48, "some paths go on after their first segment"
        t, u, v, inst, prim = o.trace_closest(eo, ed)
        tb, ib, pb = o.trace_brute(eo, ed)
        hit = inst != UNSET
        assert 0.2 < hit.mean() < 0.8, hit.mean()
        assert np.array_equal(hit, ib != UNSET)
        assert np.array_equal(t[hit], tb[hit])
        assert ((inst == ib) & (prim == pb))[hit].mean() > 0.999
    finally:
        o.close()


# ---- 5. the scenarios reach what they are there for ----------------------------

RUNS = ([(n, 64, 48, 3, 1) for n in SCENARIOS] + [(n, 64, 48, 2, 4) for n in ("A", "C", "F", "H2", "H3")] +
        [("A", 96, 64, 8, 1), ("C", 96, 64, 8, 1)])


@pytest.mark.parametrize("name,W,H,frames,spp", RUNS, ids=[f"{r[0]}-{r[1]}x{r[2]}x{r[3]}-spp{r[4]}" for r in RUNS])
def test_scenario_conditions(name, W, H, frames, spp):
    """The renders tests/test_gpu_scene_edges.py asks of the GPU, on the oracle
    alone: each meets its scenario's conditions."""
    o = edited_oracle(SCENARIOS[name])
    try:
        acc, cnt = render_counted(o, W, H, frames, spp)
        check_conditions(name, o, cnt, acc)
        assert np.isfinite(acc).all()
        assert name == "I2" or (acc[..., :3] >= 0).all()      # I2's albedo has a negative channel
        if name in EXTREMES and spp == 1:
            # what the GPU tests stand on: the cutoff leaves the radiance bits alone
            plain, _, _ = o.render(W, H, frames)
            assert np.array_equal(plain.view(np.uint32), acc.view(np.uint32)), f"{name}: the cutoff changed the oracle's radiance"
    finally:
        o.close()
