"""The edge-avoiding a-trous denoiser on the device (surf_denoise,
surf_denoise_image; Renderer.denoise / .denoise_image) against the numpy
restatement of tests/test_denoise_host.py.

Bar: bit-exact, images compared as uint32 words.  The expected image never
comes from the code under test: np_denoise restates the header's arithmetic in
float32 numpy with glibc's expf.  Both kernel variants are run: taps from
global memory (SURF_DENOISE_LDS=0) and from the staged LDS tile
(SURF_DENOISE_LDS=16: every step the library can stage; the steps past its
limit of 4 take the direct kernel in both runs).

Rendered frames are 100 x 37: 100 is no multiple of the 32-wide tile, 37 none
of its 8 rows, and the fifth iteration's step of 16 reaches past the 37 rows.
"""
import os
import subprocess

import numpy as np
import pytest

import surf_amd
from test_denoise_host import W, H, assert_images_equal, denoise_frames, expected_image, np_denoise  # noqa: F401
from test_gpu_aov import read_pfm

pytestmark = pytest.mark.gpu
F = np.float32
LDS_VARIANTS = ["0", "16"]


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def rendered(product_scene, **kw):
    r = surf_amd.Renderer(product_scene, W, H, **kw)
    r.render(1, spp=4)
    return r


_want = {}


def want_of(acc, planes, **params):
    """np_denoise of a device frame, computed once per (frame bits, parameters)."""
    key = (acc.tobytes(), planes["position"].tobytes(), tuple(sorted(params.items())))
    if key not in _want:
        _want[key] = np_denoise(acc, planes["position"], planes["normal"], planes["albedo"], **params)
    return _want[key]


# ---- 1. the render path ---------------------------------------------------------

@pytest.mark.parametrize("lds", LDS_VARIANTS)
def test_render_path_bitexact(product_scene, monkeypatch, lds):
    monkeypatch.setenv("SURF_DENOISE_LDS", lds)
    r = rendered(product_scene)
    try:
        acc, planes = r.accumulator(), r.aov()
        assert (acc[..., 3] == 4.0).all()
        for iterations in (1, 3, 5):
            for demodulate in (0, 1):
                want = want_of(acc, planes, iterations=iterations, demodulate=demodulate)
                got = r.denoise(iterations=iterations, demodulate=demodulate)
                assert_images_equal(got, want, f"LDS {lds}, {iterations} iterations, demodulate {demodulate}")
                ms = r.debug_denoise_time()
                assert len(ms) == 7 and sum(ms[: iterations + 1]) > 0.0 and all(t == 0.0 for t in ms[iterations + 1:]), ms
        assert not np.array_equal(r.denoise()[..., :3], acc[..., :3] * F(0.25))
    finally:
        r.close()


# ---- 2. the image path ----------------------------------------------------------

@pytest.mark.parametrize("lds", LDS_VARIANTS)
@pytest.mark.parametrize("name", ["b", "c", "tile"])
def test_image_path_bitexact(product_scene, denoise_frames, monkeypatch, name, lds):
    monkeypatch.setenv("SURF_DENOISE_LDS", lds)
    acc, planes = denoise_frames[name]
    r = surf_amd.Renderer(product_scene, 8, 8)          # the frame's size is the image's, not the context's
    try:
        for iterations, demodulate in ((5, 1), (2, 0)):
            want = expected_image(denoise_frames, name, iterations=iterations, demodulate=demodulate)
            got = r.denoise_image(acc, planes, iterations=iterations, demodulate=demodulate)
            assert_images_equal(got, want, f"frame {name}, LDS {lds}, {iterations} iterations: device vs numpy")
            host = surf_amd.denoise_image_host(acc, planes, iterations=iterations, demodulate=demodulate)
            assert_images_equal(got, host, f"frame {name}, LDS {lds}, {iterations} iterations: device vs host twin")
    finally:
        r.close()


def test_image_path_needs_no_scene(denoise_frames):
    import ctypes as C
    lib = surf_amd.load()
    acc, planes = denoise_frames["c"]
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        p = surf_amd.denoise_params()
        out = np.zeros_like(acc)
        assert lib.surf_denoise(h, C.byref(p), out.ctypes.data) == -4           # SURF_ERR_NO_SCENE
        a = [np.ascontiguousarray(x) for x in (acc, planes["position"], planes["normal"], planes["albedo"])]
        assert lib.surf_denoise_image(h, 5, 3, *[x.ctypes.data for x in a], C.byref(p), out.ctypes.data) == 0
        assert_images_equal(out, expected_image(denoise_frames, "c"), "context without a scene")
        assert lib.surf_denoise_image(h, 0, 3, *[x.ctypes.data for x in a], C.byref(p), out.ctypes.data) == -1
    finally:
        lib.surf_destroy(h)


# ---- 3. neutrality ----------------------------------------------------------------

def test_denoise_is_neutral_to_the_sample_stream(product_scene):
    out = []
    for filt in (True, False):
        r = surf_amd.Renderer(product_scene, W, H)
        r.render(2, 0)
        if filt:
            before = r.accumulator()
            img = r.denoise()
            assert np.array_equal(r.accumulator().view(np.uint32), before.view(np.uint32))
            assert not np.array_equal(img[..., :3], before[..., :3] * F(0.5))
        r.render(2, 2)
        out.append((r.accumulator(), r.stats()))
        r.close()
    (acc_a, st_a), (acc_b, st_b) = out
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc", "samples"):
        assert st_a[k] == st_b[k], k
    assert st_a["samples"] == 4 * W * H


# ---- 4. row shards ------------------------------------------------------------------

def test_shards_refuse_and_assemble(product_scene):
    specs = [surf_amd.ShardSpec(k, 2, 2) for k in range(2)]              # interleaved blocks of 2 rows
    whole = rendered(product_scene)
    full = whole.denoise()
    accs, planes = [], []
    for s in specs:
        r = rendered(product_scene, shard=s)
        with pytest.raises(surf_amd.SurfError) as e:
            r.denoise()
        assert e.value.code == -1 and "surf_denoise_image" in str(e.value)
        accs.append(r.accumulator())
        planes.append(r.aov())
        r.close()
    acc = surf_amd.assemble_shards(W, H, accs, specs)
    pl = {k: surf_amd.assemble_shards(W, H, [p[k] for p in planes], specs) for k in ("position", "normal", "albedo")}
    got = whole.denoise_image(acc, pl)
    whole.close()
    assert_images_equal(got, full, "assembled shards through denoise_image vs the full frame's denoise")


# ---- 5. the cached planes follow the camera -------------------------------------------

def test_denoise_follows_set_camera(oracle_scene, product_scene):
    ubo = np.frombuffer(oracle_scene.camera_ubo(W, H), np.float32).copy()
    shift = np.array([0.0, 6.0, -12.0], np.float32)
    ubo[0:3] = ubo[0:3] + shift              # position
    ubo[16:19] = ubo[16:19] + shift          # first_pixel
    r = rendered(product_scene)
    try:
        first = r.denoise(iterations=2)                       # fills the plane cache
        r.set_camera(ubo.tobytes())
        r.clear_accumulator()
        r.render(1, spp=4)
        acc, planes = r.accumulator(), r.aov()
        miss = (planes["albedo"][..., 3] == 0).mean()
        assert 0.3 <= miss <= 0.8, f"{miss:.3f} of the pixels miss"
        got = r.denoise(iterations=2)
        assert_images_equal(got, want_of(acc, planes, iterations=2), "moved camera")
        assert not np.array_equal(got, first)
    finally:
        r.close()


# ---- 6. the C++ API and the example -----------------------------------------------------

def test_cpp_example_matches_python(product_scene, tmp_path):
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    prefix = str(tmp_path / "dn")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "4", prefix], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = rendered(product_scene)
    acc, want = r.accumulator(), r.denoise()
    r.close()
    got = read_pfm(prefix + "_denoised.pfm")
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32))
    noisy = read_pfm(prefix + "_noisy.pfm")
    assert np.array_equal(np.ascontiguousarray(noisy).view(np.uint32),
                          np.ascontiguousarray(acc[..., :3] * (F(1.0) / acc[..., 3:4])).view(np.uint32))
    png = open(prefix + "_denoised.png", "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
