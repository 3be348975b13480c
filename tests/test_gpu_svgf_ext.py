"""The variance-guided filter's two optional stages on the device (k_firefly, the
feedback instantiation of k_atrous_var; surf_firefly_image, surf_svgf_*_ex) against
the host twins and the numpy restatement of tests/test_svgf_ext_host.py.

Bar: bit-exact, images compared as uint32 words.  The expected images never come
from the code under test on the device: they are np_firefly's and np_svgf_ext's,
and the _ex twin's fed the same planes (the twin itself is held to numpy in
tests/test_svgf_ext_host.py).

Frames are 100 x 37 -- partial tiles on both axes, four tile columns and five tile
rows, so most k_firefly blocks have halo texels inside and outside the frame --
33 x 9 (one pixel past a tile both ways) and 1 x 1.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from test_denoise_host import assert_images_equal
from test_gpu_temporal import device_frame, step
from test_svgf_ext_host import firefly_fixtures, np_firefly, np_svgf_ext  # noqa: F401
from test_svgf_host import assert_outputs_equal, svgf_frames, with_moments  # noqa: F401
from test_temporal_host import W, H, as_prev, np_temporal, temporal_frames  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
EXT = dict(firefly_scale=4.0, feedback=True)


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def outputs(r, **params):
    """svgf() and what it left on the context, in np_svgf's order."""
    out = r.svgf(**params)
    return out, r.temporal_history(), r.svgf_moments(), r.svgf_variance()


# ---- 1. the clamp alone ---------------------------------------------------------------

@pytest.mark.parametrize("name,scale,demodulate", [("real", 1.0, 1), ("real", 2.0, 1), ("real", 4.0, 1), ("synthetic", 1.0, 1),
                                                   ("synthetic", 4.0, 0), ("one", 1.0, 1), ("tile", 1.0, 1), ("tile", 1.5, 0)])
def test_firefly_image_bitexact(product_scene, firefly_fixtures, name, scale, demodulate):
    acc, alb = firefly_fixtures[name]
    r = surf_amd.Renderer(product_scene, 8, 8)            # the frame's size is the image's, not the context's
    try:
        assert r.debug_firefly_time() == 0.0
        got = r.firefly_image(acc, alb, scale, demodulate)
        assert_images_equal(got, np_firefly(acc, alb, scale, demodulate)[0], f"{name}, scale {scale}: device vs numpy")
        assert_images_equal(got, surf_amd.firefly_image_host(acc, alb, scale, demodulate), f"{name}, scale {scale}: device vs host twin")
        assert r.debug_firefly_time() > 0.0
        with pytest.raises(surf_amd.SurfError) as e:
            r.firefly_image(acc, alb, 0.5)
        assert e.value.code == -1 and "scale" in str(e.value)
    finally:
        r.close()


# ---- 2. the render path over an animated chain ----------------------------------------------

def run_chain(lds=None, monkeypatch=None):
    if lds is not None:
        monkeypatch.setenv("SURF_DENOISE_LDS", lds)
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        cam = scene.camera(W, H)
        prev = None
        for k in range(3):
            step(r, scene, k)
            f = device_frame(r, scene, cam)
            got = outputs(r, **EXT)
            assert r.debug_firefly_time() > 0.0
            want = surf_amd.svgf_image_host(f, prev, **EXT)
            assert_outputs_equal(got, want, f"frame {k}: device vs the _ex twin")
            if lds is None:
                assert_outputs_equal(got, np_svgf_ext(f, prev, **EXT), f"frame {k}: device vs numpy")
            prev = with_moments(f, want[1], want[2])
        valid = f["albedo"][..., 3] != 0
        assert valid.sum() > 3000 and (got[1][..., 3][valid] > 1.0).sum() > 1000      # the fed-back history is reprojected and used
    finally:
        r.close()
        scene.close()


def test_render_path_bitexact():
    run_chain()


def test_render_path_without_staging(monkeypatch):
    """SURF_DENOISE_LDS=0: iteration 0 runs the feedback instantiation that reads its taps from global memory."""
    run_chain("0", monkeypatch)


def test_image_path_bitexact(product_scene, svgf_frames):
    r = surf_amd.Renderer(product_scene, 8, 8)
    try:
        for name, ext in (("tile", EXT), ("chain", dict(feedback=True)), ("chain", dict(firefly_scale=1.0))):
            prev = None
            for k, f in enumerate(svgf_frames[name][:2]):
                want = surf_amd.svgf_image_host(f, prev, **ext)
                assert_outputs_equal(r.svgf_image(f, prev, **ext), want, f"{name} {ext}, frame {k}: device vs the _ex twin")
                prev = with_moments(f, want[1], want[2])
    finally:
        r.close()


# ---- 3. off means the call without _ex ------------------------------------------------------

def test_ext_off_is_the_plain_call():
    scene = surf_amd.Scene.indoor()
    rs = [surf_amd.Renderer(scene, W, H) for _ in range(4)]
    offs = [{}, dict(ext=None), dict(ext=surf_amd.SvgfExt()), dict(firefly_scale=0.0, feedback=False)]
    try:
        for k in range(2):
            scene.update(0.1)
            res = []
            for r, off in zip(rs, offs):
                r.update_instances(scene)
                r.clear_accumulator()
                r.render(1, first_frame=k, spp=2)
                res.append(outputs(r, **off))
            for got, off in zip(res[1:], offs[1:]):
                assert_outputs_equal(got, res[0], f"frame {k}: {off} vs svgf()")
    finally:
        for r in rs:
            r.close()
        scene.close()


# ---- 4. mixed calls on the shared state ------------------------------------------------------

def test_mixed_calls_follow_the_twin_chain():
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        cam = scene.camera(W, H)
        step(r, scene, 0)
        f0 = device_frame(r, scene, cam)
        w0 = surf_amd.svgf_image_host(f0, None, **EXT)
        assert_outputs_equal(outputs(r, **EXT), w0, "svgf with ext, first frame")
        plain0 = surf_amd.svgf_image_host(f0, None)
        assert not np.array_equal(w0[1], plain0[1])                     # the stored history is the fed-back one
        step(r, scene, 1)
        f1 = device_frame(r, scene, cam)
        blend1 = r.temporal()                                           # the plain blend reads the fed-back history
        hist1 = r.temporal_history()
        want_blend, want_hist, _ = np_temporal(f1, as_prev(f0, w0[1]))
        assert_images_equal(blend1, want_blend, "temporal() after svgf(feedback): the blend")
        assert_images_equal(hist1, want_hist, "temporal() after svgf(feedback): the history")
        step(r, scene, 2)
        f2 = device_frame(r, scene, cam)
        w2 = surf_amd.svgf_image_host(f2, with_moments(f1, hist1, None))
        assert_outputs_equal(outputs(r), w2, "plain svgf() after temporal(): the history goes on, unfiltered again")
    finally:
        r.close()
        scene.close()


# ---- 5. neutrality ----------------------------------------------------------------------------

def test_ext_is_neutral_to_the_sample_stream(product_scene):
    out = []
    for filt in (True, False):
        r = surf_amd.Renderer(product_scene, W, H)
        r.render(2, 0)
        if filt:
            before = r.accumulator()
            img = r.svgf(**EXT)
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


# ---- 6. row shards, the device-to-device copy --------------------------------------------------

def test_a_row_shard_refuses(product_scene):
    r = surf_amd.Renderer(product_scene, W, H, shard=surf_amd.ShardSpec(0, 2, 2))
    try:
        r.render(1, spp=1)
        with pytest.raises(surf_amd.SurfError) as e:
            r.svgf(**EXT)
        assert e.value.code == -1 and "surf_svgf_image" in str(e.value)
    finally:
        r.close()


def test_copy_to_device(product_scene):
    with open("/proc/self/maps") as maps:
        hip_path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(hip_path)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    r = surf_amd.Renderer(product_scene, W, H)
    dev = C.c_void_p()
    try:
        r.render(1, spp=2)
        want = r.svgf(**EXT)
        want_hist = r.temporal_history()
        r.temporal_reset()
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        r.copy_svgf_to(dev.value, **EXT)
        got = np.zeros((H, W, 4), np.float32)
        assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0       # hipMemcpyDeviceToHost
        assert_images_equal(got, want, "copy_svgf_to with ext")
        assert_images_equal(r.temporal_history(), want_hist, "copy_svgf_to with ext: the stored history")
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()
