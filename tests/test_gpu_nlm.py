"""The dual-buffer non-local-means filter on the device (surf_denoise_nlm*), against
the numpy restatement of tests/test_nlm_host.py.

Bar: bit-exact, images compared as uint32 words.  The expected images never come
from the code under test: np_nlm restates the header's rules, the halves are summed
in numpy (np_halves) from the oracle's samples or from the bucket planes read back.

Both filter kernels are run: the staged one (the default, where its LDS layout
fits: r + f <= 10, so (r, f) = (1, 0), (3, 1), (5, 2) and the largest, (7, 3)) and the
global one (SURF_NLM_LDS=0 in a context created under that setting, and (8, 3) and
(10, 3) in either, whose layouts do not fit).
Frames: 100 x 37, 33 x 9, 70 x 3 and 1 x 1 -- no multiple of the 32 x 8 tile, partial
tiles either way, more than one block, a frame lower than the search window.
"""
import ctypes as C

import numpy as np
import pytest

import surf_amd
from surf_amd import ShardSpec
from test_denoise_host import assert_images_equal
from test_nlm_host import CASES, assert_nlm_equal, expected, frame, np_nlm
from test_robust_host import np_halves
from test_sampled_host import H, W

pytestmark = pytest.mark.gpu
SURF_ERR_INVALID = -1
COUNTERS = ("samples", "n_ext", "n_hit", "n_cont", "n_shadow", "n_acc", "n_unocc")
FRAMES = 19                                       # uneven counts: with M = 16 the halves hold 10 and 9 samples


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def renderer(scene, M, squares=False, **kw):
    r = surf_amd.Renderer(scene, W, H, **kw)
    if squares:
        r.set_sample_squares(True)
    if M:
        r.set_sample_buckets(M)
    return r


# ---- 1. the image form -------------------------------------------------------------------------------

@pytest.mark.parametrize("lds", ["1", "0"], ids=["staged", "global"])
def test_image_form_bitexact(product_scene, monkeypatch, lds):
    """Every frame and (r, f) of the host test, one context per variant; the first call on a fresh context
    also shows the diagnostics zero before it and nonzero after."""
    monkeypatch.setenv("SURF_NLM_LDS", lds)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert r.debug_nlm_time() == [0.0, 0.0, 0.0]
        for name, rf in CASES:
            h0, h1 = frame(name)
            got = r.denoise_nlm_image(h0, h1, search_radius=rf[0], patch_radius=rf[1])
            assert_nlm_equal(got, expected(name, rf), f"SURF_NLM_LDS={lds}, {name}, r {rf[0]}, f {rf[1]}")
            ms = r.debug_nlm_time()
            assert ms[1] > 0.0 and ms[2] > 0.0, ms
        h0, h1 = frame("b5")
        sp = dict(search_radius=3, patch_radius=1, k=0.2, alpha=2.0, eps=1e-4)
        assert_nlm_equal(r.denoise_nlm_image(h0, h1, **sp), np_nlm(h0, h1, **sp), f"SURF_NLM_LDS={lds}, other scalars")
        assert_nlm_equal(r.denoise_nlm_image(*frame("a")), surf_amd.denoise_nlm_image_host(*frame("a")), "device vs host twin")
    finally:
        r.close()


def test_either_side_of_the_fit_rule(product_scene):
    """(7, 3) is the largest layout the staged kernel takes (r + f = 10), (8, 3) the smallest it leaves to the global
    one; on a frame of partial tiles and on the planted one."""
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        for name in ("b5", "planted"):
            for rf in ((7, 3), (8, 3), (10, 0)):
                h0, h1 = frame(name)
                sp = dict(search_radius=rf[0], patch_radius=rf[1])
                assert_nlm_equal(r.denoise_nlm_image(h0, h1, **sp), np_nlm(h0, h1, **sp), f"{name}, r {rf[0]}, f {rf[1]}")
    finally:
        r.close()


def test_image_form_status_codes(product_scene):
    lib = surf_amd.load()
    h0, h1 = frame("b5")
    h, w = h0.shape[:2]
    out, err = np.zeros_like(h0), np.zeros_like(h0)
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        p = surf_amd.nlm_params(search_radius=1, patch_radius=0)
        args = lambda ww=w, hh=h, a=h0.ctypes.data, b=h1.ctypes.data, pp=C.byref(p), o=out.ctypes.data, e=err.ctypes.data: \
            (r.handle, ww, hh, a, b, pp, o, e)
        assert lib.surf_denoise_nlm_image(*args()) == 0
        assert lib.surf_denoise_nlm_image(*args(e=None)) == 0
        bad_params = [surf_amd.nlm_params(**kw) for kw in (dict(search_radius=0), dict(search_radius=11), dict(patch_radius=4), dict(k=0.0),
                                                           dict(k=float("nan")), dict(k=float("inf")), dict(alpha=-1.0), dict(eps=0.0))]
        for bad in [args(ww=0), args(hh=0), args(a=None), args(b=None), args(pp=None), args(o=None)] + [args(pp=C.byref(q)) for q in bad_params]:
            assert lib.surf_denoise_nlm_image(*bad) == SURF_ERR_INVALID
    finally:
        r.close()


# ---- 2. the context form -----------------------------------------------------------------------------

def device_buffer_reader():
    with open("/proc/self/maps") as maps:
        hip_path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
    hip = C.CDLL(hip_path)
    hip.hipMalloc.argtypes, hip.hipMemcpy.argtypes, hip.hipFree.argtypes = [C.POINTER(C.c_void_p), C.c_size_t], \
        [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], [C.c_void_p]
    return hip


@pytest.mark.parametrize("M", [4, 16])
def test_context_form_bitexact(product_scene, M):
    """19 one-sample frames: the halves of the context's own buckets, filtered; against np_nlm of the halves summed in
    numpy from the planes read back, against the image form, and through the copy to a device buffer."""
    hip = device_buffer_reader()
    r = renderer(product_scene, M)
    dev = [C.c_void_p(), C.c_void_p()]
    try:
        r.render(FRAMES, 0)
        h0, h1 = np_halves(r.sample_buckets())
        assert sorted({float(h0[0, 0, 3]), float(h1[0, 0, 3])}) == ([9.0, 10.0])
        want = np_nlm(h0, h1)
        got = r.denoise_nlm()
        assert_nlm_equal(got, want, f"surf_denoise_nlm, M = {M}")
        ms = r.debug_nlm_time()
        assert all(v > 0.0 for v in ms), ms
        assert_nlm_equal(r.denoise_nlm_image(h0, h1), want, f"surf_denoise_nlm_image on the summed halves, M = {M}")
        sp = dict(search_radius=3, patch_radius=1)
        assert_nlm_equal(r.denoise_nlm(**sp), np_nlm(h0, h1, **sp), f"surf_denoise_nlm r 3 f 1, M = {M}")
        for d in dev:
            assert hip.hipMalloc(C.byref(d), W * H * 16) == 0
        r.copy_denoise_nlm_to(dev[0].value, dev[1].value)
        back = [np.zeros((H, W, 4), np.float32) for _ in dev]
        for d, b in zip(dev, back):
            assert hip.hipMemcpy(b.ctypes.data, d, W * H * 16, 2) == 0              # hipMemcpyDeviceToHost
        assert_nlm_equal(back, want, "copy_denoise_nlm_to")
        back[0][:] = 0.0
        r.copy_denoise_nlm_to(dev[0].value)                                       # the error image is optional
        assert hip.hipMemcpy(back[0].ctypes.data, dev[0], W * H * 16, 2) == 0
        assert_images_equal(back[0], want[0], "copy_denoise_nlm_to without an error buffer")
    finally:
        for d in dev:
            if d.value:
                hip.hipFree(d)
        r.close()


# ---- 3. purity and lifecycle -------------------------------------------------------------------------

def test_call_changes_nothing_else(product_scene):
    """Two contexts render the same frames, one calls the filter in between: accumulator, buckets, squares, counters and
    a further render's result are word for word the same."""
    state = lambda r: (r.accumulator(), r.sample_buckets(), r.sample_squares(), [r.stats()[k] for k in COUNTERS])
    rs = [renderer(product_scene, 4, True) for _ in range(2)]
    try:
        for r in rs:
            r.render(8, 0)
        before = state(rs[0])
        rs[0].denoise_nlm()
        rs[0].denoise_nlm_image(*frame("b5"))
        for what, a, b in zip(("accumulator", "buckets", "squares"), state(rs[0]), before):
            assert_images_equal(a, b, f"{what} after the call")
        assert state(rs[0])[3] == before[3]
        for r in rs:
            r.render(5, 8)
        with_call, without = state(rs[0]), state(rs[1])
        for what, a, b in zip(("accumulator", "buckets", "squares"), with_call, without):
            assert_images_equal(a, b, f"{what} after a further render")
        assert with_call[3] == without[3]
    finally:
        for r in rs:
            r.close()


def test_lifecycle(product_scene):
    dev_err = lambda f, *a, **k: pytest.raises(surf_amd.SurfError, f, *a, **k).value
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        r.render(2, 0)
        e = dev_err(r.denoise_nlm)                                                  # buckets off
        assert e.code == SURF_ERR_INVALID and "surf_set_sample_buckets" in str(e)
        r.clear_accumulator()
        r.set_sample_buckets(4)
        r.render(6, 0)
        first = r.denoise_nlm()
        assert_nlm_equal(first, np_nlm(*np_halves(r.sample_buckets())), "after clear + enable")
        assert dev_err(r.denoise_nlm, search_radius=11).code == SURF_ERR_INVALID
        r.clear_accumulator()
        empty = r.denoise_nlm()                                                     # no samples: every pixel invalid, the plain mean of nothing
        assert not empty[0][..., :3].any() and (empty[0][..., 3] == 1).all() and not empty[1].any()
        r.render(6, 0)
        assert_nlm_equal(r.denoise_nlm(), first, "the same frames after surf_clear_accumulator")
    finally:
        r.close()


def test_row_shards(product_scene):
    """The context form is refused on a row shard; the image form on the halves assembled from two shards' buckets
    equals the one-context result."""
    M = 4
    specs = [ShardSpec(k, 2, 2) for k in range(2)]
    rs = [renderer(product_scene, M, shard=s) for s in specs]
    one = renderer(product_scene, M)
    try:
        for r in rs + [one]:
            r.render(FRAMES, 0)
        with pytest.raises(surf_amd.SurfError) as e:
            rs[0].denoise_nlm()
        assert e.value.code == SURF_ERR_INVALID and "surf_denoise_nlm_image" in str(e.value)
        parts = [r.sample_buckets() for r in rs]
        full = np.stack([surf_amd.assemble_shards(W, H, [p[j] for p in parts], specs) for j in range(M)])
        h0, h1 = surf_amd.bucket_halves(full)
        assert_nlm_equal(rs[1].denoise_nlm_image(h0, h1), one.denoise_nlm(), "assembled shards against one context")
    finally:
        for r in rs + [one]:
            r.close()


# ---- 4. the example ----------------------------------------------------------------------------------

def test_cpp_example_writes_the_filtered_image(product_scene, tmp_path):
    """render_denoised ... 0 8 1: one frame of 32 samples with 8 buckets, PREFIX_nlm.pfm beside the other outputs."""
    import os
    import subprocess
    from test_gpu_aov import read_pfm
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    prefix = str(tmp_path / "nl")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "32", prefix, "0", "8", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = renderer(product_scene, 8, True)
    try:
        r.render(1, 0, spp=32)
        want = r.denoise_nlm()[0]
        assert_images_equal(want, np_nlm(*np_halves(r.sample_buckets()))[0], "32 samples in one frame")
    finally:
        r.close()
    words = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(words(read_pfm(prefix + "_nlm.pfm")), words(want[..., :3]))
    for other in ("_noisy.pfm", "_robust.pfm", "_denoised.pfm", "_sampled.pfm"):
        assert os.path.exists(prefix + other), other
