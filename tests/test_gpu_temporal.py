"""Temporal accumulation with reprojection on the device (surf_temporal_accumulate,
surf_temporal_image; Renderer.temporal / .temporal_image) against the numpy
restatement of tests/test_temporal_host.py.

Bar: bit-exact, images compared as uint32 words.  The expected images never
come from the code under test: np_temporal restates the header's arithmetic in
float32 numpy, on the device's own accumulators and feature planes (which
tests/test_gpu_parity.py and tests/test_gpu_aov.py check against the oracle).
The bundled scene has 11 instances; scene variant 3 runs the kernel with 91.

Rendered frames are 100 x 37 or smaller: 100 is no multiple of the 32-wide
tile, 37 none of its 8 rows.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surf_amd
from test_denoise_host import assert_images_equal, np_denoise
from test_gpu_aov import read_pfm
from test_temporal_host import (CASES, CHAIN, UNSET, W, H, as_prev, expected_chain, np_temporal, shifted,  # noqa: F401
                                temporal_frames)

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def device_frame(r, scene, camera):
    """The renderer's current frame as np_temporal takes it."""
    f = dict(r.aov())
    f["acc"] = r.accumulator()
    f["instances"] = scene.buffers()["instances"]
    f["camera"] = camera
    return f


def step(r, scene, k, dt=0.1, spp=2):
    """One displayed frame of the loop up to the blend: move, clear, render."""
    scene.update(dt)
    r.update_instances(scene)
    r.clear_accumulator()
    r.render(1, first_frame=k, spp=spp)


# ---- 1. the render path ---------------------------------------------------------

def test_render_path_bitexact():
    params = dict(max_history=3)
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        with pytest.raises(surf_amd.SurfError) as e:
            r.temporal_history()
        assert e.value.code == -1
        cam = scene.camera(W, H)
        prev, moved, clamped = None, 0, 0
        for k in range(5):
            if k == 4:
                cam = shifted(cam, (0.05, 0.02, 0.03))
                r.set_camera(cam)
            step(r, scene, k)
            f = device_frame(r, scene, cam)
            assert (f["acc"][..., 3] == 2.0).all()
            want_out, want_hist, cnt = np_temporal(f, prev, **params)
            got = r.temporal(**params)
            assert_images_equal(got, want_out, f"frame {k}: temporal()")
            assert_images_equal(r.temporal_history(), want_hist, f"frame {k}: temporal_history()")
            assert r.debug_temporal_time() > 0.0
            moved += cnt.get("moved", 0)
            clamped += cnt["history_clamped"]
            prev = as_prev(f, want_hist)
        assert moved > 100 and clamped > 1000, (moved, clamped)
        assert not np.array_equal(got[..., :3], f["acc"][..., :3] * F(0.5))
    finally:
        r.close()
        scene.close()


# ---- 2. the image path ----------------------------------------------------------

@pytest.mark.parametrize("name,params", CASES, ids=[c[0] for c in CASES])
def test_image_path_bitexact(product_scene, temporal_frames, name, params):
    want = expected_chain(temporal_frames, name, **params)
    r = surf_amd.Renderer(product_scene, 8, 8)          # the frame's size is the image's, not the context's
    try:
        prev = None
        for k, f in enumerate(temporal_frames[name]):
            out, hist = r.temporal_image(f, prev, **params)
            assert_images_equal(out, want[k][0], f"case {name}, frame {k}: device vs numpy")
            assert_images_equal(hist, want[k][1], f"case {name}, frame {k}: history, device vs numpy")
            host_out, host_hist = surf_amd.temporal_image_host(f, prev, **params)
            assert_images_equal(out, host_out, f"case {name}, frame {k}: device vs host twin")
            assert_images_equal(hist, host_hist, f"case {name}, frame {k}: history, device vs host twin")
            prev = as_prev(f, want[k][1])
        with pytest.raises(surf_amd.SurfError) as e:    # the image path leaves the context's own state alone
            r.temporal_history()
        assert e.value.code == -1
    finally:
        r.close()


def test_image_path_needs_no_scene(temporal_frames):
    lib = surf_amd.load()
    f0, f1 = temporal_frames["small"]
    want = expected_chain(temporal_frames, "small")
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        p = surf_amd.temporal_params()
        out, hist = np.zeros((3, 5, 4), np.float32), np.zeros((3, 5, 4), np.float32)
        assert lib.surf_temporal_accumulate(h, C.byref(p), None, out.ctypes.data) == -4            # SURF_ERR_NO_SCENE
        assert lib.surf_temporal_history(h, out.ctypes.data) == -1
        w, hh, cur, prev, keep = surf_amd._temporal_frames(f1, as_prev(f0, want[0][1]))
        assert lib.surf_temporal_image(h, w, hh, C.byref(cur), C.byref(prev), C.byref(p), out.ctypes.data, hist.ctypes.data) == 0
        assert_images_equal(out, want[1][0], "context without a scene")
        assert_images_equal(hist, want[1][1], "context without a scene: history")
        assert lib.surf_temporal_image(h, 0, hh, C.byref(cur), C.byref(prev), C.byref(p), out.ctypes.data, hist.ctypes.data) == -1
        assert lib.surf_temporal_image(h, w, hh, C.byref(cur), C.byref(prev), C.byref(p), None, hist.ctypes.data) == -1
        bad = surf_amd.temporal_params(snap=0.5)
        assert lib.surf_temporal_image(h, w, hh, C.byref(cur), C.byref(prev), C.byref(bad), out.ctypes.data, hist.ctypes.data) == -1
        ms = C.c_float(-1.0)
        assert lib.surf_debug_temporal_time(h, C.byref(ms)) == 0 and ms.value > 0.0
        del keep
    finally:
        lib.surf_destroy(h)


# ---- 3. spatial chaining, reset, re-upload ----------------------------------------

def test_spatial_chaining_reset_and_reupload():
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        cam = scene.camera(W, H)
        step(r, scene, 0)
        f0 = device_frame(r, scene, cam)
        first_out, first_hist, _ = np_temporal(f0, None)
        assert_images_equal(r.temporal(), first_out, "first frame")
        # the second frame through the spatial filter: np_denoise of (np_temporal's out, w = 1) with this frame's planes
        step(r, scene, 1)
        f1 = device_frame(r, scene, cam)
        out1, hist1, cnt = np_temporal(f1, as_prev(f0, first_hist))
        assert cnt["moved"] > 20
        spatial = dict(iterations=3, sigma_color=0.8)
        want = np_denoise(out1, f1["position"], f1["normal"], f1["albedo"], **{**dict(sigma_normal=0.3, sigma_plane=0.1, demodulate=1), **spatial})
        got = r.temporal(spatial=spatial)
        assert_images_equal(got, want, "temporal(spatial=...)")
        assert_images_equal(r.temporal_history(), hist1, "the history holds the unfiltered blend")
        with pytest.raises(surf_amd.SurfError) as e:
            r.temporal(spatial=dict(iterations=9))
        assert e.value.code == -1 and "iterations" in str(e.value)
        # reset: the next call is a first frame
        r.temporal_reset()
        with pytest.raises(surf_amd.SurfError):
            r.temporal_history()
        step(r, scene, 2)
        f2 = device_frame(r, scene, cam)
        out2, hist2, _ = np_temporal(f2, None)
        assert_images_equal(r.temporal(), out2, "after temporal_reset")
        assert_images_equal(r.temporal_history(), hist2, "after temporal_reset: history")
        # a scene re-upload drops the history as well
        d = scene.desc()
        assert surf_amd.load().surf_upload_scene(r.handle, C.byref(d)) == 0
        with pytest.raises(surf_amd.SurfError):
            r.temporal_history()
        r.clear_accumulator()
        r.render(1, first_frame=3, spp=2)
        f3 = device_frame(r, scene, cam)
        out3, _, _ = np_temporal(f3, None)
        assert_images_equal(r.temporal(), out3, "after a scene re-upload")
        # ... while clear_accumulator, set_camera and update_instances keep it (test_render_path_bitexact)
    finally:
        r.close()
        scene.close()


# ---- 4. neutrality ----------------------------------------------------------------

def test_temporal_is_neutral_to_the_sample_stream(product_scene):
    out = []
    for filt in (True, False):
        r = surf_amd.Renderer(product_scene, W, H)
        r.render(2, 0)
        if filt:
            before = r.accumulator()
            img = r.temporal()
            img2 = r.temporal(spatial=True)
            assert np.array_equal(r.accumulator().view(np.uint32), before.view(np.uint32))
            assert np.array_equal(img[..., :3], before[..., :3] * F(0.5)) and not np.array_equal(img2, img)
        r.render(2, 2)
        out.append((r.accumulator(), r.stats()))
        r.close()
    (acc_a, st_a), (acc_b, st_b) = out
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc", "samples"):
        assert st_a[k] == st_b[k], k
    assert st_a["samples"] == 4 * W * H


# ---- 5. row shards ------------------------------------------------------------------

def test_shards_refuse_and_assemble():
    specs = [surf_amd.ShardSpec(k, 2, 2) for k in range(2)]              # interleaved blocks of 2 rows
    scene = surf_amd.Scene.indoor()
    whole = surf_amd.Renderer(scene, W, H)
    parts = [surf_amd.Renderer(scene, W, H, shard=s) for s in specs]
    try:
        cam = scene.camera(W, H)
        prev = None
        for k in range(2):
            scene.update(0.1)
            shards = []
            for r in [whole] + parts:
                r.update_instances(scene)
                r.clear_accumulator()
                r.render(1, first_frame=k, spp=2)
            full = whole.temporal()
            full_hist = whole.temporal_history()
            for r in parts:
                with pytest.raises(surf_amd.SurfError) as e:
                    r.temporal()
                assert e.value.code == -1 and "surf_temporal_image" in str(e.value)
                f = dict(r.aov())
                f["acc"] = r.accumulator()
                shards.append(f)
            cur = {name: surf_amd.assemble_shards(W, H, [s[name].view(np.float32) for s in shards], specs)
                   for name in ("acc", "position", "normal", "id")}
            cur["id"] = cur["id"].view(np.uint32)
            cur["instances"], cur["camera"] = scene.buffers()["instances"], cam
            out, hist = whole.temporal_image(cur, prev)
            assert_images_equal(out, full, f"frame {k}: assembled shards through temporal_image vs the full frame's temporal()")
            assert_images_equal(hist, full_hist, f"frame {k}: history")
            prev = as_prev(cur, hist)
    finally:
        for r in [whole] + parts:
            r.close()
        scene.close()


# ---- 6. more than 64 instances (k_aov's tables in global memory, a motion table of 91 records) ---

def test_global_tables_bitexact():
    w, h = 48, 32
    scene = surf_amd.Scene.indoor(variant=3)
    r = surf_amd.Renderer(scene, w, h)
    try:
        assert scene.desc().instance_count > 64
        cam = scene.camera(w, h)
        prev, moved = None, 0
        for k in range(3):
            if k == 2:
                cam = shifted(cam, (0.05, 0.02, 0.03))
                r.set_camera(cam)
            step(r, scene, k)
            f = device_frame(r, scene, cam)
            want_out, want_hist, cnt = np_temporal(f, prev)
            assert_images_equal(r.temporal(), want_out, f"variant 3, frame {k}")
            assert_images_equal(r.temporal_history(), want_hist, f"variant 3, frame {k}: history")
            moved += cnt.get("moved", 0)
            prev = as_prev(f, want_hist)
        assert (f["id"][..., 0][f["id"][..., 0] != UNSET] >= 64).sum() >= 1, "no pixel sees an instance past the LDS table size"
        assert moved > 0, "the update moved nothing in view"
    finally:
        r.close()
        scene.close()


# ---- 7. the device-to-device copy ------------------------------------------------------

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
        want = r.temporal()
        r.temporal_reset()
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        r.copy_temporal_to(dev.value)
        got = np.zeros((H, W, 4), np.float32)
        assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0       # hipMemcpyDeviceToHost
        assert_images_equal(got, want, "copy_temporal_to")
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()


# ---- 8. the C++ API and the example -----------------------------------------------------

def test_cpp_example_matches_python(tmp_path):
    spp, frames = 2, 3
    exe = os.path.join(surf_amd._PKG, "build", "render_animated")
    prefix = str(tmp_path / "anim")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), str(spp), str(frames), prefix], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stderr
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        for k in range(frames):
            scene.update(0.05)
            r.update_instances(scene)
            r.clear_accumulator()
            r.render(1, first_frame=k * spp, spp=spp)
            img = r.temporal(spatial=True if k + 1 == frames else None)
        acc, blend = r.accumulator(), r.temporal_history()
    finally:
        r.close()
        scene.close()
    same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
    assert same(read_pfm(prefix + "_temporal_denoised.pfm"), img[..., :3])
    assert same(read_pfm(prefix + "_temporal.pfm"), blend[..., :3])
    assert same(read_pfm(prefix + "_noisy.pfm"), acc[..., :3] * (F(1.0) / acc[..., 3:4]))
    assert not same(blend[..., :3], acc[..., :3] * (F(1.0) / acc[..., 3:4]))
    png = open(prefix + "_temporal_denoised.png", "rb").read()
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
