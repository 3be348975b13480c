"""The light-map atlas on the device (include/surf_hip.h, "the light-map atlas"): surf_atlas_build, surf_atlas_finish and
surf_atlas_dilate against the CPU twins and against the numpy restatement of tests/test_atlas_host.py, bit for bit, under
both work mappings of the cover kernel (SURF_ATLAS_MAP, read when a context is created: each mapping has a context of its
own); the device-pointer forms; and bake_atlas end to end against Renderer.bake fed the same planes through the host."""
import ctypes as C
import os

import numpy as np
import pytest

import surf_amd
from test_atlas_host import (CASES, DILATE_ITERATIONS, Case, F, IDENTITY, U, WHITE, assert_atlas_equal, assert_mirror_image, check_case_properties,
                             dilate_expected, dilate_planes, expected, finish_planes, instance_records, material_records, np_atlas_finish)

pytestmark = pytest.mark.gpu

MAPS = {"tiles": "1", "triangles": "0"}


def renderer_with_map(scene, value, w=32, h=24):
    old = os.environ.get("SURF_ATLAS_MAP")
    os.environ["SURF_ATLAS_MAP"] = value
    try:
        return surf_amd.Renderer(scene, w, h)
    finally:
        if old is None:
            del os.environ["SURF_ATLAS_MAP"]
        else:
            os.environ["SURF_ATLAS_MAP"] = old


@pytest.fixture(scope="module")
def renderers(product_scene):
    """A context per mapping; the atlas's size is its own, so one small frame serves every case."""
    rs = {name: renderer_with_map(product_scene, value) for name, value in MAPS.items()}
    yield rs
    for r in rs.values():
        r.close()


class DeviceBuffers:
    """Buffers from the HIP runtime the library itself runs on (already mapped into this process)."""

    def __init__(self):
        with open("/proc/self/maps") as maps:
            path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
        self.hip = C.CDLL(path)
        self.hip.hipMalloc.argtypes, self.hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], [C.c_void_p]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.ptrs = []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        self.ptrs.append(p)
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p

    def download(self, p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.hip.hipFree(p)
        self.ptrs = []


@pytest.fixture
def dev():
    d = DeviceBuffers()
    yield d
    d.close()


# ---- 1. the rasterizer -----------------------------------------------------------------------------------

@pytest.mark.parametrize("mapping", list(MAPS))
@pytest.mark.parametrize("name", list(CASES))
def test_build_equals_numpy_and_the_twin(renderers, name, mapping):
    case, want = expected(name)
    r = renderers[mapping]
    got = r.atlas_build(case.desc(), case.charts, case.W, case.H)
    assert r.debug_atlas_time()["tile_map"] == (mapping == "tiles")
    assert_atlas_equal(got, want, f"{name}, {mapping}: device against numpy")
    assert_atlas_equal(got, surf_amd.atlas_build_host(case.desc(), case.charts, case.W, case.H), f"{name}, {mapping}: device against the twin")
    check_case_properties(name, case, got)


@pytest.mark.parametrize("mapping", list(MAPS))
def test_mirrored_chart_owns_the_mirror_image(renderers, mapping):
    (off, _), (on, _) = expected("mirror-off"), expected("mirror-on")
    r = renderers[mapping]
    assert_mirror_image(r.atlas_build(off.desc(), off.charts, off.W, off.H), r.atlas_build(on.desc(), on.charts, on.W, on.H),
                        f"the device, {mapping}")


def test_susanne_equals_the_twin(renderers):
    """The bundled susanne (15,744 small triangles) through obj_load at 256 x 256: both mappings against the CPU twin."""
    tris, ext = surf_amd.obj_load(os.path.join(surf_amd.ASSETS_DIR, "susanne.obj.gz"))
    case = Case(tris, ext, instance_records([(0, 0, IDENTITY)]), material_records(WHITE), [(0, 0, 1.0, 1.0, 0.0, 0.0)], 256, 256)
    want = surf_amd.atlas_build_host(case.desc(), case.charts, 256, 256)
    assert want["summary"]["triangles"] == 15744 and want["summary"]["covered"] > 256 * 256 // 4
    for mapping, r in renderers.items():
        assert_atlas_equal(r.atlas_build(case.desc(), case.charts, 256, 256), want, f"susanne, {mapping}")


def test_build_to_device_planes(renderers, dev):
    """surf_atlas_build_device writes the same planes in place; a NULL plane is left out."""
    case, want = expected("soup-37x29")
    n = case.W * case.H * 16
    for mapping, r in renderers.items():
        ptrs = [dev.alloc(n) for _ in range(4)]
        s = r.atlas_build_to(case.desc(), case.charts, case.W, case.H, *ptrs)
        got = {k: dev.download(p, (case.H, case.W, 4), U if k == "ids" else F) for k, p in zip(surf_amd.ATLAS_PLANES, ptrs)}
        got["summary"] = s
        assert_atlas_equal(got, want, f"device planes, {mapping}")
        assert r.atlas_build_to(case.desc(), case.charts, case.W, case.H, 0, ptrs[1], 0, 0) == want["summary"]
        assert np.array_equal(dev.download(ptrs[1], (case.H, case.W, 4), U), want["normal"].view(U))


def test_build_refuses_what_the_twin_refuses(renderers):
    r = renderers["tiles"]
    case, _ = expected("quad-32x32")
    projective = CASES["posed-flip"]()
    projective.inst[0, 8:24].view(F)[7] = 0.25                     # row 3 of M is (0, 0.25, 0, 1)
    for c, charts, W, H in ((case, case.charts, 0, 8), (case, case.charts, 8, 16385), (case, [], 8, 8), (case, [(3, 0, 1.0, 1.0, 0.0, 0.0)], 8, 8),
                            (case, [(0, 0, float("nan"), 1.0, 0.0, 0.0)], 8, 8), (projective, projective.charts, 8, 8)):
        with pytest.raises(surf_amd.SurfError) as e:
            r.atlas_build(c.desc(), charts, W, H)
        assert e.value.code == -1


# ---- 2. finish and dilate --------------------------------------------------------------------------------

def test_finish_equals_numpy_and_the_twin(renderers, dev):
    acc, alb = finish_planes()
    H, W = acc.shape[:2]
    want, want_valid = np_atlas_finish(acc, alb)
    r = renderers["tiles"]
    got, valid = r.atlas_finish(acc, alb)
    twin, twin_valid = surf_amd.atlas_finish_host(acc, alb)
    assert np.array_equal(got.view(U), want.view(U)) and np.array_equal(valid, want_valid)
    assert np.array_equal(got.view(U), twin.view(U)) and np.array_equal(valid, twin_valid)
    out, ov = dev.alloc(W * H * 16), dev.alloc(W * H)
    r.atlas_finish_to(W, H, dev.upload(acc), dev.upload(alb), out, ov)
    assert np.array_equal(dev.download(out, (H, W, 4), U), want.view(U)) and np.array_equal(dev.download(ov, (H, W), np.uint8), want_valid)


@pytest.mark.parametrize("iterations", DILATE_ITERATIONS)
def test_dilate_equals_numpy_and_the_twin(renderers, dev, iterations):
    rgba, valid = dilate_planes()
    H, W = valid.shape
    want, want_valid = dilate_expected(iterations)
    r = renderers["tiles"]
    got, got_valid = r.atlas_dilate(rgba, valid, iterations)
    twin, twin_valid = surf_amd.atlas_dilate_host(rgba, valid, iterations)
    assert np.array_equal(got.view(U), want.view(U)) and np.array_equal(got_valid, want_valid)
    assert np.array_equal(got.view(U), twin.view(U)) and np.array_equal(got_valid, twin_valid)
    out, ov = dev.alloc(W * H * 16), dev.alloc(W * H)
    r.atlas_dilate_to(W, H, dev.upload(rgba), dev.upload(valid), iterations, out, ov)
    assert np.array_equal(dev.download(out, (H, W, 4), U), want.view(U)) and np.array_equal(dev.download(ov, (H, W), np.uint8), want_valid)


@pytest.mark.parametrize("fill", [0, 1])
def test_dilate_leaves_uniform_masks_alone(renderers, fill):
    rgba, _ = dilate_planes()
    valid = np.full(rgba.shape[:2], fill, np.uint8)
    if not fill:
        rgba = np.zeros_like(rgba)
    got, got_valid = renderers["tiles"].atlas_dilate(rgba, valid, 3)
    assert np.array_equal(got.view(U), rgba.view(U)) and np.array_equal(got_valid, valid)


# ---- 3. end to end ---------------------------------------------------------------------------------------

def test_bake_atlas_equals_bake_through_the_host(product_scene):
    """bake_atlas -- build on the device, the sensor set from its planes, 4 frames, finish, dilate -- against Renderer.bake
    fed atlas_build's planes through the host (tests/test_gpu_surfel_sensor.py pins that path to the oracle)."""
    W, H = 32, 24
    charts = surf_amd.atlas_grid_charts(product_scene.desc().instance_count, W, H, 1)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        baked = r.bake_atlas(product_scene, charts, 4, iterations=2)
        assert r.sensor() == (surf_amd.SENSOR_CAMERA, W * H)                       # the camera is back
        planes = r.atlas_build(product_scene, charts, W, H)
        assert baked["summary"] == planes["summary"] and planes["summary"]["covered"] > 0
        assert np.array_equal(r.accumulator().view(U), baked["accumulator"].view(U))   # the accumulator keeps the bake
        want = r.bake(planes["position"], planes["normal"], 4)
        assert np.array_equal(baked["accumulator"].view(U), want.view(U))
        owned = planes["ids"][..., 3] >= 1
        assert (baked["accumulator"][~owned].view(U) == 0).all() and (~owned).any()    # empty texels: never traced, w == 0
        assert (baked["accumulator"][owned][:, 3] == F(4)).all()
        lit, lit_valid = surf_amd.atlas_finish_host(want, planes["albedo"])
        assert np.array_equal(lit_valid.astype(bool), owned)
        out, out_valid = surf_amd.atlas_dilate_host(lit, lit_valid, 2)
        assert np.array_equal(baked["lightmap"].view(U), out.view(U)) and np.array_equal(baked["valid"], out_valid)
        assert r.sensor() == (surf_amd.SENSOR_CAMERA, W * H)
        with pytest.raises(ValueError):
            r.bake_atlas(product_scene, charts, 4, iterations=65)
    finally:
        r.close()
    shard = surf_amd.Renderer(product_scene, W, H, shard=surf_amd.ShardSpec(0, 2, 0))
    try:
        with pytest.raises(ValueError):
            shard.bake_atlas(product_scene, charts, 1)
    finally:
        shard.close()
