"""The variance-guided filter on the device (surf_svgf_accumulate, surf_svgf_image;
Renderer.svgf / .svgf_image) against the numpy restatement of
tests/test_svgf_host.py.

Bar: bit-exact, images compared as uint32 words.  The expected images never
come from the code under test: np_svgf restates the header's arithmetic in
float32 numpy, on the device's own accumulators and feature planes (which
tests/test_gpu_parity.py and tests/test_gpu_aov.py check against the oracle).

Rendered frames are 100 x 37 or smaller: 100 is no multiple of the 32-wide
tile, 37 none of its 8 rows; 33 x 9 is one pixel past a tile both ways.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surf_amd
from test_denoise_host import assert_images_equal
from test_gpu_aov import read_pfm
from test_gpu_temporal import device_frame, step
from test_svgf_host import assert_outputs_equal, expected_chain, np_svgf, svgf_frames, with_moments  # noqa: F401
from test_temporal_host import CHAIN, UNSET, W, H, as_prev, np_temporal, shifted, temporal_frames  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def outputs(r, **params):
    """svgf() and what it left on the context, in np_svgf's order."""
    out = r.svgf(**params)
    return out, r.temporal_history(), r.svgf_moments(), r.svgf_variance()


# ---- 1. the render path ---------------------------------------------------------

@pytest.mark.parametrize("params", [{}, dict(max_history=3, spatial_below=4)], ids=["defaults", "always-spatial"])
def test_render_path_bitexact(params):
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        for read in (r.svgf_moments, r.svgf_variance):
            with pytest.raises(surf_amd.SurfError) as e:
                read()
            assert e.value.code == -1
        cam = scene.camera(W, H)
        prev, long, short = None, 0, 0
        for k in range(5):
            if k == 4:
                cam = shifted(cam, (0.05, 0.02, 0.03))
                r.set_camera(cam)
            step(r, scene, k)
            f = device_frame(r, scene, cam)
            want = np_svgf(f, prev, **params)
            assert_outputs_equal(outputs(r, **params), want, f"frame {k}")
            ms = r.debug_svgf_time()
            assert all(v > 0.0 for v in ms[:7]) and ms[7] == 0.0, ms
            long += want[4]["long"]
            short += want[4]["short"]
            prev = with_moments(f, want[1], want[2])
        assert short > 1000 and (long == 0 if params else long > 1000), (long, short)    # max_history 3 never reaches spatial_below 4
    finally:
        r.close()
        scene.close()


# ---- 2. the image path ----------------------------------------------------------

IMAGE_CASES = [("small", {}), ("tile", {}), ("b", {}), ("chain", CHAIN)]


@pytest.mark.parametrize("name,params", IMAGE_CASES, ids=[c[0] for c in IMAGE_CASES])
def test_image_path_bitexact(product_scene, svgf_frames, name, params):
    want = expected_chain(svgf_frames, name, **params)
    r = surf_amd.Renderer(product_scene, 8, 8)          # the frame's size is the image's, not the context's
    try:
        prev = None
        for k, f in enumerate(svgf_frames[name]):
            got = r.svgf_image(f, prev, **params)
            assert_outputs_equal(got, want[k], f"case {name}, frame {k}: device vs numpy")
            assert_outputs_equal(got, surf_amd.svgf_image_host(f, prev, **params), f"case {name}, frame {k}: device vs host twin")
            prev = with_moments(f, want[k][1], want[k][2])
        for read in (r.temporal_history, r.svgf_moments, r.svgf_variance):      # the image path leaves the context's own state alone
            with pytest.raises(surf_amd.SurfError) as e:
                read()
            assert e.value.code == -1
    finally:
        r.close()


def test_image_path_needs_no_scene(svgf_frames):
    lib = surf_amd.load()
    f0, f1 = svgf_frames["small"]
    want = expected_chain(svgf_frames, "small")
    h = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(h)) == 0
    try:
        p, sp = surf_amd.temporal_params(), surf_amd.svgf_params()
        o = [np.zeros((3, 5, 4), np.float32) for _ in range(4)]
        op = [a.ctypes.data for a in o]
        assert lib.surf_svgf_accumulate(h, C.byref(p), C.byref(sp), op[0]) == -4            # SURF_ERR_NO_SCENE
        assert lib.surf_svgf_moments(h, op[0]) == -1
        w, hh, cur, prev, keep = surf_amd._svgf_frames(f1, with_moments(f0, want[0][1], want[0][2]))
        assert lib.surf_svgf_image(h, w, hh, C.byref(cur), C.byref(prev), C.byref(p), C.byref(sp), *op) == 0
        assert_outputs_equal(o, want[1], "context without a scene")
        assert lib.surf_svgf_image(h, 0, hh, C.byref(cur), C.byref(prev), C.byref(p), C.byref(sp), *op) == -1
        assert lib.surf_svgf_image(h, w, hh, C.byref(cur), C.byref(prev), C.byref(p), C.byref(sp), op[0], op[1], None, op[3]) == -1
        bad = surf_amd.svgf_params(spatial_below=0)
        assert lib.surf_svgf_image(h, w, hh, C.byref(cur), C.byref(prev), C.byref(p), C.byref(bad), *op) == -1
        del keep
    finally:
        lib.surf_destroy(h)


# ---- 3. staging: the same bits from LDS and from global memory ----------------------

@pytest.mark.parametrize("name", ["chain", "tile"])
def test_staging_knobs_keep_the_bits(product_scene, svgf_frames, monkeypatch, name):
    """100 x 37 ('chain', frame 1) and 33 x 9 ('tile', frame 1), 6 iterations so that every
    step up to 32 runs; the knobs are read when the context is created."""
    params = dict(iterations=6, **(CHAIN if name == "chain" else {}))
    f0, f1 = svgf_frames[name][:2]
    first = np_svgf(f0, None, **params)
    prev = with_moments(f0, first[1], first[2])
    want = [first, np_svgf(f1, prev, **params)]
    for var_lds, dn_lds in (("1", "0"), ("1", "2"), ("1", "4"), ("0", "0"), ("0", "2"), ("0", "4")):
        monkeypatch.setenv("SURF_SVGF_LDS", var_lds)
        monkeypatch.setenv("SURF_DENOISE_LDS", dn_lds)
        r = surf_amd.Renderer(product_scene, 8, 8)
        try:
            assert_outputs_equal(r.svgf_image(f1, prev, **params), want[1], f"{name}: SURF_SVGF_LDS={var_lds} SURF_DENOISE_LDS={dn_lds}")
        finally:
            r.close()


# ---- 4. mixed calls, reset, re-upload ------------------------------------------------

def test_mixed_calls_reset_and_reupload():
    scene = surf_amd.Scene.indoor()
    r = surf_amd.Renderer(scene, W, H)
    try:
        cam = scene.camera(W, H)
        step(r, scene, 0)
        f0 = device_frame(r, scene, cam)
        w0 = np_svgf(f0, None)
        assert_outputs_equal(outputs(r), w0, "svgf, first frame")
        step(r, scene, 1)
        f1 = device_frame(r, scene, cam)
        blend1 = r.temporal()                                      # the plain blend on the same state ...
        hist1 = r.temporal_history()
        assert_images_equal(hist1, np_temporal(f1, as_prev(f0, w0[1]))[1], "temporal() after svgf(): the shared history")
        assert np.array_equal(blend1[..., :3], hist1[..., :3])
        with pytest.raises(surf_amd.SurfError) as e:               # ... leaves the moments marked absent
            r.svgf_moments()
        assert e.value.code == -1
        step(r, scene, 2)
        f2 = device_frame(r, scene, cam)
        w2 = np_svgf(f2, with_moments(f1, hist1, None))
        assert w2[4]["colour_without_moments"] > 1000
        assert_outputs_equal(outputs(r), w2, "svgf after temporal(): the colour history goes on, the moments start again")
        hit = (f2["id"][..., 0] != UNSET) & (f2["acc"][..., 3] > 0)
        assert (r.svgf_moments()[..., 2][hit] == 1.0).all()
        # reset: the next call is a first frame
        r.temporal_reset()
        for read in (r.svgf_moments, r.svgf_variance, r.temporal_history):
            with pytest.raises(surf_amd.SurfError):
                read()
        step(r, scene, 3)
        f3 = device_frame(r, scene, cam)
        assert_outputs_equal(outputs(r), np_svgf(f3, None), "after temporal_reset")
        # a scene re-upload drops the moments with the history
        d = scene.desc()
        assert surf_amd.load().surf_upload_scene(r.handle, C.byref(d)) == 0
        for read in (r.svgf_moments, r.temporal_history):
            with pytest.raises(surf_amd.SurfError):
                read()
        r.clear_accumulator()
        r.render(1, first_frame=4, spp=2)
        f4 = device_frame(r, scene, cam)
        assert_outputs_equal(outputs(r), np_svgf(f4, None), "after a scene re-upload")
        with pytest.raises(surf_amd.SurfError) as e:
            r.svgf(spatial_below=0)
        assert e.value.code == -1 and "spatial_below" in str(e.value)
    finally:
        r.close()
        scene.close()


# ---- 5. neutrality ----------------------------------------------------------------

def test_svgf_is_neutral_to_the_sample_stream(product_scene):
    out = []
    for filt in (True, False):
        r = surf_amd.Renderer(product_scene, W, H)
        r.render(2, 0)
        if filt:
            before = r.accumulator()
            img = r.svgf()
            img2 = r.svgf(iterations=2)
            assert np.array_equal(r.accumulator().view(np.uint32), before.view(np.uint32))
            assert not np.array_equal(img[..., :3], before[..., :3] * F(0.5)) and not np.array_equal(img2, img)
        r.render(2, 2)
        out.append((r.accumulator(), r.stats()))
        r.close()
    (acc_a, st_a), (acc_b, st_b) = out
    assert np.array_equal(acc_a.view(np.uint32), acc_b.view(np.uint32))
    for k in ("n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc", "samples"):
        assert st_a[k] == st_b[k], k
    assert st_a["samples"] == 4 * W * H


# ---- 6. row shards ------------------------------------------------------------------

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
            full = outputs(whole)
            for r in parts:
                with pytest.raises(surf_amd.SurfError) as e:
                    r.svgf()
                assert e.value.code == -1 and "surf_svgf_image" in str(e.value)
                f = dict(r.aov())
                f["acc"] = r.accumulator()
                shards.append(f)
            cur = {name: surf_amd.assemble_shards(W, H, [s[name].view(np.float32) for s in shards], specs)
                   for name in ("acc", "position", "normal", "albedo", "id")}
            cur["id"] = cur["id"].view(np.uint32)
            cur["instances"], cur["camera"] = scene.buffers()["instances"], cam
            got = whole.svgf_image(cur, prev)
            assert_outputs_equal(got, full, f"frame {k}: assembled shards through svgf_image vs the full frame's svgf()")
            prev = with_moments(cur, got[1], got[2])
    finally:
        for r in [whole] + parts:
            r.close()
        scene.close()


# ---- 7. more than 64 instances (global tables, a motion table of 91 records) ---------

def test_global_tables_bitexact():
    w, h = 48, 32
    scene = surf_amd.Scene.indoor(variant=3)
    r = surf_amd.Renderer(scene, w, h)
    try:
        assert scene.desc().instance_count > 64
        cam = scene.camera(w, h)
        prev = None
        for k in range(3):
            if k == 2:
                cam = shifted(cam, (0.05, 0.02, 0.03))
                r.set_camera(cam)
            step(r, scene, k)
            f = device_frame(r, scene, cam)
            want = np_svgf(f, prev, spatial_below=2)
            assert_outputs_equal(outputs(r, spatial_below=2), want, f"variant 3, frame {k}")
            prev = with_moments(f, want[1], want[2])
        assert want[4]["long"] > 0 and want[4]["short"] > 0
    finally:
        r.close()
        scene.close()


# ---- 8. the device-to-device copy, the C++ API and the example ---------------------------

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
        want = r.svgf()
        r.temporal_reset()
        assert hip.hipMalloc(C.byref(dev), W * H * 16) == 0
        r.copy_svgf_to(dev.value)
        got = np.zeros((H, W, 4), np.float32)
        assert hip.hipMemcpy(got.ctypes.data, dev, W * H * 16, 2) == 0       # hipMemcpyDeviceToHost
        assert_images_equal(got, want, "copy_svgf_to")
    finally:
        if dev.value:
            hip.hipFree(dev)
        r.close()


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
            plain = r.temporal(spatial=True if k + 1 == frames else None)
        img = r.svgf()                                                    # the last frame once more, on the state the loop left
    finally:
        r.close()
        scene.close()
    got = read_pfm(prefix + "_svgf.pfm")
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(img[..., :3]).view(np.uint32))
    assert not np.array_equal(got, plain[..., :3])
