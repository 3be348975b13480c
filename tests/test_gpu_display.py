"""The display stage on the device (surf_display*), against the numpy restatement of
tests/test_display_host.py.

Bar: bit-exact, RGBA8 words and every field of the meter's result.  The expected images
never come from the code under test: np_display restates the header's rules on the
oracle's samples summed in numpy, or on planes read back from the device.

Frames: 100 x 37, 33 x 9, 70 x 3, 1 x 1, a planted one and an all-black one -- no multiple
of the 32 x 8 tile, partial tiles either way, more than one block, frames lower and
narrower than the blur window.  Both pack kernels run: the fused one (no bloom) and the
blur's two passes (R = 1, 4, 16).
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from surf_amd import ShardSpec
from test_adaptive_host import LOOP, loop_case
from test_denoise_host import assert_images_equal
from test_display_host import CASES, PSETS, accumulator, assert_display_equal, expected, frame, np_display
from test_gpu_nlm import device_buffer_reader
from test_nlm_host import np_nlm
from test_robust_host import np_halves
from test_sampled_host import H, W

pytestmark = pytest.mark.gpu
SURF_ERR_INVALID = -1
COUNTERS = ("samples", "n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")
D2H, H2D = 2, 1                                   # hipMemcpyKind


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


class DeviceBuffers:
    """Device allocations of this process's HIP runtime, freed on exit."""

    def __init__(self):
        self.hip, self.ptrs = device_buffer_reader(), []

    def alloc(self, nbytes):
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), nbytes) == 0
        self.ptrs.append(p)
        return p

    def upload(self, a):
        p = self.alloc(a.nbytes)
        assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, H2D) == 0
        return p

    def read(self, p, shape, dtype):
        out = np.zeros(shape, dtype)
        assert self.hip.hipMemcpy(out.ctypes.data, p, out.nbytes, D2H) == 0
        return out

    def close(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


# ---- 1. the image forms ------------------------------------------------------------------------------

def test_image_form_bitexact(product_scene):
    """Every frame and parameter set of the host test on one context; the first call on a fresh context also shows the
    diagnostics zero before it, and afterwards positive for the stages that ran: the blur stage is 0 without bloom."""
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert r.debug_display_time() == [0.0, 0.0, 0.0, 0.0]
        for name, pset in CASES:
            assert_display_equal(r.display_image(frame(name), **PSETS[pset]), expected(name, pset), f"surf_display_image, {name}, {pset}")
            ms = r.debug_display_time()
            bloom = PSETS[pset].get("bloom_radius", 0) > 0
            assert ms[0] > 0.0 and ms[1] > 0.0 and ms[3] > 0.0 and ((ms[2] > 0.0) if bloom else (ms[2] == 0.0)), (name, pset, ms)
    finally:
        r.close()


def test_device_form_bitexact(product_scene):
    """surf_display_image_device from a plane on the device to words on the device: every frame and parameter set of the
    host test again; a smaller frame after a larger one reuses the scratch."""
    r = surf_amd.Renderer(product_scene, W, H)
    dev = DeviceBuffers()
    try:
        planes = {}
        for name, pset in CASES:
            a = frame(name)
            h, w = a.shape[:2]
            if name not in planes:
                planes[name] = (dev.upload(np.ascontiguousarray(a)), dev.alloc(w * h * 4))
            src, dst = planes[name]
            meter = r.display_image_device(src.value, w, h, dst.value, **PSETS[pset])
            assert_display_equal((dev.read(dst, (h, w), np.uint32), meter), expected(name, pset), f"surf_display_image_device, {name}, {pset}")
    finally:
        dev.close()
        r.close()


def test_device_equals_host_twin(product_scene):
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        for name in ("a", "planted"):
            for kw in ({}, dict(bloom_radius=8, bloom_threshold=0.5, bloom_strength=0.3, curve=1, white=3.0), dict(bloom_radius=16, transfer=1)):
                got, want = r.display_image(frame(name), **kw), surf_amd.display_image_host(frame(name), **kw)
                assert np.array_equal(got[0], want[0]), (name, kw)
                assert np.array_equal(got[1]["hist"], want[1]["hist"]) and all(got[1][k] == want[1][k] for k in ("counted", "black", "median_bin", "scale"))
    finally:
        r.close()


def test_image_form_status_codes(product_scene):
    lib = surf_amd.load()
    a = frame("b")
    h, w = a.shape[:2]
    out = np.zeros((h, w), np.uint32)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        p = surf_amd.display_params()
        args = lambda ww=w, hh=h, src=a.ctypes.data, pp=C.byref(p), o=out.ctypes.data: (r.handle, ww, hh, src, pp, o, None)
        assert lib.surf_display_image(*args()) == 0
        bad_params = [surf_amd.display_params(**kw) for kw in (dict(exposure_mode=2), dict(key=0.0), dict(min_scale=65.0), dict(bloom_radius=17),
                                                               dict(bloom_strength=-1.0), dict(curve=3), dict(white=float("nan")),
                                                               dict(transfer=3), dict(dither=2))]
        for bad in [args(ww=0), args(hh=0), args(src=None), args(pp=None), args(o=None)] + [args(pp=C.byref(q)) for q in bad_params]:
            assert lib.surf_display_image(*bad) == SURF_ERR_INVALID
            assert lib.surf_display_image_device(*bad) == SURF_ERR_INVALID
        assert lib.surf_display(r.handle, None, out.ctypes.data, None) == SURF_ERR_INVALID
        assert lib.surf_display(r.handle, C.byref(p), None, None) == SURF_ERR_INVALID
    finally:
        r.close()


# ---- 2. the context form -----------------------------------------------------------------------------

def test_context_form_bitexact(product_scene):
    """Four one-sample frames at 100 x 37: surf_display against np_display of the oracle's samples summed in numpy."""
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        r.render(4, 0)
        acc = accumulator(4)
        for kw in ({}, dict(bloom_radius=4, bloom_threshold=0.5), dict(exposure_mode=0, exposure=3.0, curve=1, transfer=1, dither=0)):
            assert_display_equal(r.display(**kw), np_display(acc, **kw), f"surf_display, {kw}")
    finally:
        r.close()


def test_context_form_after_an_adaptive_render(product_scene):
    """The pixels hold different sample counts: each is divided by its own."""
    want = loop_case()
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        r.set_sample_squares(True)
        r.render_adaptive(**LOOP)
        acc = np.ascontiguousarray(want["acc"], np.float32)
        assert len(np.unique(acc[..., 3])) > 1
        for kw in ({}, dict(bloom_radius=2, bloom_threshold=0.25)):
            assert_display_equal(r.display(**kw), np_display(acc, **kw), f"surf_display after render_adaptive, {kw}")
    finally:
        r.close()


def test_refusals(product_scene):
    shard = surf_amd.Renderer(product_scene, W, H, shard=ShardSpec(0, 2, 2))
    one = surf_amd.Renderer(product_scene, W, H)
    try:
        shard.render(2, 0)
        with pytest.raises(surf_amd.SurfError) as e:
            shard.display()
        assert e.value.code == SURF_ERR_INVALID and "surf_display_image" in str(e.value)
        assert_display_equal(shard.display_image(frame("b")), expected("b", "defaults"), "the image form on a shard's context")
        with pytest.raises(surf_amd.SurfError) as e:                                    # never rendered
            one.display()
        assert e.value.code == SURF_ERR_INVALID and "nothing rendered" in str(e.value)
        one.render(2, 0)
        one.display()
        one.clear_accumulator()
        with pytest.raises(surf_amd.SurfError) as e:                                    # cleared
            one.display()
        assert e.value.code == SURF_ERR_INVALID
        with pytest.raises(surf_amd.SurfError) as e:
            one.display(bloom_radius=17)
        assert e.value.code == SURF_ERR_INVALID and "bloom_radius" in str(e.value)
    finally:
        shard.close()
        one.close()


# ---- 3. chaining, reproducibility, purity ------------------------------------------------------------

def test_chained_after_a_filter_on_the_device(product_scene):
    """denoise_nlm's _copy_device form, then surf_display_image_device on that buffer: np_display(np_nlm(...))."""
    r = surf_amd.Renderer(product_scene, W, H)
    dev = DeviceBuffers()
    try:
        r.set_sample_buckets(4)
        r.render(8, 0)
        filtered = np_nlm(*np_halves(r.sample_buckets()), search_radius=3, patch_radius=1)[0]
        src, dst = dev.alloc(W * H * 16), dev.alloc(W * H * 4)
        r.copy_denoise_nlm_to(src.value, search_radius=3, patch_radius=1)
        for kw in ({}, dict(bloom_radius=4, bloom_threshold=0.5)):
            meter = r.display_image_device(src.value, W, H, dst.value, **kw)
            assert_display_equal((dev.read(dst, (H, W), np.uint32), meter), np_display(filtered, **kw), f"nlm then display, {kw}")
    finally:
        dev.close()
        r.close()


def test_two_runs_are_identical(product_scene):
    """The histogram is built with integer atomics only: the words and the meter's result do not depend on the order of
    arrival.  640 x 360: more blocks than one wave of them."""
    rng = np.random.default_rng(5)
    img = rng.random((360, 640, 4), np.float32) * np.float32(4.0)
    img[..., 3] = 3.0
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        runs = [r.display_image(img, bloom_radius=4, bloom_threshold=0.5) for _ in range(2)]
        assert np.array_equal(runs[0][0], runs[1][0])
        assert np.array_equal(runs[0][1]["hist"], runs[1][1]["hist"])
        assert all(runs[0][1][k] == runs[1][1][k] for k in ("counted", "black", "median_bin", "scale"))
        assert_display_equal(runs[0], np_display(img, bloom_radius=4, bloom_threshold=0.5), "640 x 360")
    finally:
        r.close()


def test_call_changes_nothing_else(product_scene):
    """Two contexts render the same frames, one calls the display stage in between: accumulator, squares, counters, the
    existing packs' words and a further render's result are word for word the same."""
    state = lambda r: (r.accumulator(), r.sample_squares(), [r.stats()[k] for k in COUNTERS])
    rs = [surf_amd.Renderer(product_scene, W, H) for _ in range(2)]
    try:
        for r in rs:
            r.set_sample_squares(True)
            r.render(6, 0)
        before = state(rs[0])
        packs = (rs[0].display_rgba8(), rs[0].finalize_rgba8(), rs[0].finalize_weighted())
        rs[0].display()
        rs[0].display(bloom_radius=4)
        rs[0].display_image(frame("b"))
        for what, a, b in zip(("accumulator", "squares"), state(rs[0]), before):
            assert_images_equal(a, b, f"{what} after the call")
        assert state(rs[0])[2] == before[2]
        for what, a, b in zip(("surf_display_rgba8", "surf_finalize_rgba8", "surf_finalize_rgba8_weighted"),
                              (rs[0].display_rgba8(), rs[0].finalize_rgba8(), rs[0].finalize_weighted()), packs):
            assert np.array_equal(a, b), what
        assert np.array_equal(packs[0], rs[1].display_rgba8())
        for r in rs:
            r.render(3, 6)
        for what, a, b in zip(("accumulator", "squares"), state(rs[0]), state(rs[1])):
            assert_images_equal(a, b, f"{what} after a further render")
        assert state(rs[0])[2] == state(rs[1])[2]
    finally:
        for r in rs:
            r.close()


# ---- 4. the example ----------------------------------------------------------------------------------

def test_cpp_example_writes_the_png(product_scene, tmp_path):
    """display_pfm IN.pfm OUT.png key=value: the PFM of an accumulator's mean through surf_display_image."""
    import os
    import subprocess
    from PIL import Image
    acc = accumulator(16)
    mean = np.ones_like(acc)
    mean[..., :3] = acc[..., :3] / acc[..., 3:]
    src, dst = str(tmp_path / "in.pfm"), str(tmp_path / "out.png")
    assert surf_amd.load().surf_write_pfm(src.encode(), W, H, mean.ctypes.data) == 0
    exe = os.path.join(surf_amd._PKG, "build", "display_pfm")
    run = subprocess.run([exe, src, dst, "bloom_radius=4", "bloom_threshold=0.5"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    want = np_display(mean, bloom_radius=4, bloom_threshold=0.5)
    png = np.asarray(Image.open(dst).convert("RGBA")).astype(np.uint32)
    words = png[..., 0] | (png[..., 1] << 8) | (png[..., 2] << 16) | (png[..., 3] << 24)
    assert np.array_equal(words, want[0])
    assert f"median bin {want[1]['median_bin']}" in run.stdout
    bad = subprocess.run([exe, src, dst, "gamma=2.2"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "gamma" in bad.stderr


CPP_PROGRAM = r"""
#include "surf/surf_host.hpp"
#include "indoor_scene.hpp"
#include <cstdio>
#include <cstdlib>
using namespace surf;
int main(int argc, char** argv) {
    const U32 W = (U32)std::atoi(argv[2]), H = (U32)std::atoi(argv[3]);
    try {
        RenderContext context;
        Camera worldCam = indoorCamera(W, H);
        IndoorScene indoor(&context, argv[1]);
        RendererConfig config;
        config.samplesPerFrame = (U32)std::atoi(argv[4]);
        WaveFrontRenderer renderer(&context, nullptr, config, FramebufferSize{W, H}, worldCam, *indoor.scene);
        renderer.render(0.0f);
        surf_display_params p;
        surf_display_default_params(&p);
        p.bloom_radius = 4;
        p.bloom_threshold = 0.5f;
        surf_display_meter_result meter;
        const std::vector<U32> words = renderer.display(p, &meter);
        FILE* f = std::fopen(argv[5], "wb");
        if (!f || std::fwrite(words.data(), sizeof(U32), words.size(), f) != words.size() || std::fclose(f) != 0) return 1;
        std::printf("%u %u %u %.9g\n", meter.counted, meter.black, meter.median_bin, (double)meter.scale);
        p.bloom_radius = 17;
        try { renderer.display(p); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
"""


def test_cpp_api_display(product_scene, tmp_path):
    """WaveFrontRenderer::display(params, &meter) in a program built against the installed headers and library: the words
    and the meter's result of one frame of 4 samples equal np_display of the accumulator of the same render."""
    import os
    import subprocess
    src, exe, out = tmp_path / "display_api.cpp", tmp_path / "display_api", tmp_path / "words.bin"
    src.write_text(CPP_PROGRAM)
    pkg = surf_amd._PKG
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(surf_amd.REPO_ROOT, "include"), "-I", os.path.join(pkg, "examples"), str(src),
                    "-o", str(exe), "-L", os.path.join(pkg, "lib"), "-lsurf_hip", "-Wl,-rpath," + os.path.join(pkg, "lib")], check=True)
    run = subprocess.run([str(exe), surf_amd.ASSETS_DIR, str(W), str(H), "4", str(out)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        r.render(1, 0, spp=4)
        want = np_display(r.accumulator(), bloom_radius=4, bloom_threshold=0.5)
    finally:
        r.close()
    assert np.array_equal(np.fromfile(out, np.uint32).reshape(H, W), want[0])
    first, second = run.stdout.splitlines()[:2]
    counted, black, median, scale = first.split()
    assert (int(counted), int(black), int(median)) == (want[1]["counted"], want[1]["black"], want[1]["median_bin"])
    assert np.float32(scale) == want[1]["scale"]
    assert second.startswith("refused:") and "bloom_radius" in second
