"""The first-order feature regression filter on the device (surf_denoise_regress*), against
the numpy restatement of tests/test_regress_host.py.

Bar: bit-exact, images compared as uint32 words.  The expected images never come from the
code under test: np_regress restates the header's rules, the halves are summed in numpy
(np_halves) from the oracle's samples or from the bucket planes read back, the planes are the
oracle's, synthetic ones, or the context's own read back.

Both filter kernels are run: the staged one (the default: every (r, f) in range fits its
bound of 160 KiB, two workgroups a compute unit up to 80 KiB, one above) and the global one
(SURF_REGRESS_LDS=0 in a context created under that setting).
Frames: 100 x 37, 33 x 9, 70 x 3 and 1 x 1 -- no multiple of the 32 x 8 tile, partial tiles
either way, more than one block, a frame lower than the search window.
"""
import ctypes as C
import os

import numpy as np
import pytest

import surf_amd
from surf_amd import ShardSpec
from test_denoise_host import assert_images_equal
from test_gpu_nlm import COUNTERS, FRAMES, device_buffer_reader, renderer
from test_nlm_adaptive_host import NLM_SMALL, np_error_mask
from test_nlm_host import RADII, expected as nlm_expected, frame as nlm_frame, np_nlm
from test_regress_host import FRAMES as NAMES, OTHER_SCALARS, assert_regress_equal, case, expected, np_regress
from test_robust_host import np_buckets, np_halves
from test_sampled_host import H, W, oracle_samples

pytestmark = pytest.mark.gpu
SURF_ERR_INVALID = -1
PLANES = ("position", "normal", "albedo")


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


@pytest.fixture(scope="module")
def variants(product_scene):
    """One context per filter kernel: SURF_REGRESS_LDS is read when a context is created."""
    before = os.environ.get("SURF_REGRESS_LDS")
    rs = {}
    try:
        for lds in ("1", "0"):
            os.environ["SURF_REGRESS_LDS"] = lds
            rs[lds] = surf_amd.Renderer(product_scene, W, H)
    finally:
        if before is None:
            os.environ.pop("SURF_REGRESS_LDS", None)
        else:
            os.environ["SURF_REGRESS_LDS"] = before
    yield rs
    for r in rs.values():
        r.close()


# ---- 1. the image form -------------------------------------------------------------------------------

def test_diagnostics_are_zero_before_the_first_call(product_scene):
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        assert r.debug_regress_time() == [0.0, 0.0, 0.0]
        r.denoise_regress_image(*case("one"))
        ms = r.debug_regress_time()
        assert ms[1] > 0.0 and ms[2] > 0.0, ms
    finally:
        r.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("lds", ["1", "0"], ids=["staged", "global"])
def test_image_form_bitexact(variants, lds, name):
    """Every frame and (r, f) of the host test on either kernel."""
    r = variants[lds]
    h0, h1, planes = case(name)
    for rf in RADII:
        got = r.denoise_regress_image(h0, h1, planes, search_radius=rf[0], patch_radius=rf[1])
        assert_regress_equal(got, expected(name, rf), f"SURF_REGRESS_LDS={lds}, {name}, r {rf[0]}, f {rf[1]}")
        ms = r.debug_regress_time()
        assert ms[1] > 0.0 and ms[2] > 0.0, ms


@pytest.mark.parametrize("lds", ["1", "0"], ids=["staged", "global"])
def test_other_scalars_bitexact(variants, lds):
    h0, h1, planes = case("b5")
    for kw in OTHER_SCALARS:
        sp = dict(search_radius=3, patch_radius=1, **kw)
        assert_regress_equal(variants[lds].denoise_regress_image(h0, h1, planes, **sp), np_regress(h0, h1, planes, **sp),
                             f"SURF_REGRESS_LDS={lds}, {kw}")


@pytest.mark.parametrize("lds", ["1", "0"], ids=["staged", "global"])
def test_device_equals_host_twin(variants, lds):
    h0, h1, planes = case("a")
    assert_regress_equal(variants[lds].denoise_regress_image(h0, h1, planes), surf_amd.denoise_regress_image_host(h0, h1, planes),
                         "device vs host twin")


_fit = {}


def fit_rule_expected(name, rf):
    if (name, rf) not in _fit:
        _fit[name, rf] = np_regress(*case(name), search_radius=rf[0], patch_radius=rf[1])
    return _fit[name, rf]


def lds_bytes(r, f):
    """regressLdsBytes restated: 40 B a texel of the tile with its halo of r + f, 8 B with its halo of f, 32 B with its halo of r."""
    texels = lambda halo: (32 + 2 * halo) * (8 + 2 * halo)
    return 40 * texels(r + f) + 8 * texels(f) + 32 * texels(r)


LDS_MAX, LDS_TWO = 160 * 1024, 80 * 1024                  # the bound; up to half of it two workgroups share a compute unit
ALL_RF = [(r, f) for r in range(1, 11) for f in range(0, 4)]
LARGEST_STAGED = max((rf for rf in ALL_RF if lds_bytes(*rf) <= LDS_MAX), key=lambda rf: lds_bytes(*rf))
LEFT_TO_GLOBAL = [rf for rf in ALL_RF if lds_bytes(*rf) > LDS_MAX]
LARGEST_TWO = max((rf for rf in ALL_RF if lds_bytes(*rf) <= LDS_TWO), key=lambda rf: lds_bytes(*rf))
SMALLEST_ONE = min((rf for rf in ALL_RF if lds_bytes(*rf) > LDS_TWO), key=lambda rf: lds_bytes(*rf))
FIT_RULE = (LARGEST_STAGED, LARGEST_TWO, SMALLEST_ONE, (6, 2), (8, 0), (10, 0))


def test_the_fit_rule_is_what_the_header_says():
    """The bound leaves nothing in range to the global kernel; the sizes at which the staged kernel's residency changes."""
    assert LARGEST_STAGED == (10, 3) and LEFT_TO_GLOBAL == [] and LARGEST_TWO == (7, 1) and SMALLEST_ONE == (6, 3)
    assert lds_bytes(5, 2) == 68_128 and lds_bytes(7, 1) == 81_184 and lds_bytes(6, 3) == 84_416 and lds_bytes(10, 3) == 129_728


@pytest.mark.parametrize("name", ["b5", "planted_syn"])
@pytest.mark.parametrize("lds", ["1", "0"], ids=["staged", "global"])
def test_either_side_of_the_fit_rule(variants, lds, name):
    """The largest layout the staged kernel takes -- the largest there is: the bound leaves none to the global kernel,
    which runs them under SURF_REGRESS_LDS=0 -- the layouts either side of 80 KiB, where one workgroup a compute unit
    takes over from two, their neighbours and (10, 0); on a frame of partial tiles and on the planted one."""
    h0, h1, planes = case(name)
    for rf in FIT_RULE:
        sp = dict(search_radius=rf[0], patch_radius=rf[1])
        assert_regress_equal(variants[lds].denoise_regress_image(h0, h1, planes, **sp), fit_rule_expected(name, rf),
                             f"SURF_REGRESS_LDS={lds}, {name}, r {rf[0]}, f {rf[1]}")


def test_image_form_status_codes(product_scene, variants):
    lib = surf_amd.load()
    h0, h1, planes = case("b5")
    h, w = h0.shape[:2]
    out, err = np.zeros_like(h0), np.zeros_like(h0)
    pl = [np.ascontiguousarray(planes[k]) for k in PLANES]
    r = variants["1"]
    p = surf_amd.regress_params(search_radius=1, patch_radius=0)
    args = lambda ww=w, hh=h, a=h0.ctypes.data, b=h1.ctypes.data, P=pl[0].ctypes.data, N=pl[1].ctypes.data, A=pl[2].ctypes.data, \
        pp=C.byref(p), o=out.ctypes.data, e=err.ctypes.data: (r.handle, ww, hh, a, b, P, N, A, pp, o, e)
    assert lib.surf_denoise_regress_image(*args()) == 0
    assert lib.surf_denoise_regress_image(*args(e=None)) == 0
    bad_params = [surf_amd.regress_params(**kw) for kw in (dict(search_radius=0), dict(search_radius=11), dict(patch_radius=4), dict(k=0.0),
                                                           dict(k=float("nan")), dict(k=float("inf")), dict(alpha=-1.0), dict(eps=0.0),
                                                           dict(ridge=0.0), dict(ridge=float("nan")), dict(ridge=float("inf")))]
    for bad in [args(ww=0), args(hh=0), args(a=None), args(b=None), args(P=None), args(N=None), args(A=None), args(pp=None), args(o=None)] + \
            [args(pp=C.byref(q)) for q in bad_params]:
        assert lib.surf_denoise_regress_image(*bad) == SURF_ERR_INVALID


# ---- 2. the context form -----------------------------------------------------------------------------

@pytest.mark.parametrize("M", [4, 16])
def test_context_form_bitexact(product_scene, M):
    """19 one-sample frames: the halves of the context's own buckets and its own planes, first-hit and then the
    chain's; against np_regress of the halves summed in numpy from the planes read back, against the image form, and
    through the copy to a device buffer."""
    hip = device_buffer_reader()
    r = renderer(product_scene, M)
    dev = [C.c_void_p(), C.c_void_p()]
    try:
        r.render(FRAMES, 0)
        h0, h1 = np_halves(r.sample_buckets())
        assert sorted({float(h0[0, 0, 3]), float(h1[0, 0, 3])}) == ([9.0, 10.0])
        planes = r.aov()
        want = np_regress(h0, h1, planes)
        got = r.denoise_regress()
        assert_regress_equal(got, want, f"surf_denoise_regress, M = {M}")
        ms = r.debug_regress_time()
        assert all(v > 0.0 for v in ms), ms
        assert_regress_equal(r.denoise_regress_image(h0, h1, planes), want, f"surf_denoise_regress_image on the same inputs, M = {M}")
        for d in dev:
            assert hip.hipMalloc(C.byref(d), W * H * 16) == 0
        r.copy_denoise_regress_to(dev[0].value, dev[1].value)
        back = [np.zeros((H, W, 4), np.float32) for _ in dev]
        for d, b in zip(dev, back):
            assert hip.hipMemcpy(b.ctypes.data, d, W * H * 16, 2) == 0              # hipMemcpyDeviceToHost
        assert_regress_equal(back, want, "copy_denoise_regress_to")
        back[0][:] = 0.0
        r.copy_denoise_regress_to(dev[0].value)                                   # the error image is optional
        assert hip.hipMemcpy(back[0].ctypes.data, dev[0], W * H * 16, 2) == 0
        assert_images_equal(back[0], want[0], "copy_denoise_regress_to without an error buffer")
        # the chain's planes
        r.set_filter_guides("chain")
        chain = r.aov_chain()
        assert any(not np.array_equal(chain[k].view(np.uint32), planes[k].view(np.uint32)) for k in PLANES)
        sp = dict(search_radius=3, patch_radius=1)
        assert_regress_equal(r.denoise_regress(**sp), np_regress(h0, h1, chain, **sp), f"the chain's planes, M = {M}")
        assert_regress_equal(r.denoise_regress_image(h0, h1, chain, **sp), np_regress(h0, h1, chain, **sp), f"the image form on them, M = {M}")
        r.set_filter_guides("first_hit")
        assert_regress_equal(r.denoise_regress(**sp), np_regress(h0, h1, planes, **sp), f"back on the first-hit planes, M = {M}")
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
        rs[0].denoise_regress()
        rs[0].denoise_regress_image(*case("b5"))
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


def test_the_two_filters_share_one_set_of_planes(product_scene):
    """The regression runs in the non-local-means filter's seven planes.  On one context: the non-local-means image
    form on a 33 x 9 frame; the regression's image form on a 100 x 37 one, so that the shared planes grow under the
    first result; the first call again; the mask from the filter's run on the context's own buckets; the regression's
    context form.  Every result against its numpy restatement, and the non-local-means times untouched by a
    regression call."""
    rf = (5, 2)
    sp = dict(search_radius=rf[0], patch_radius=rf[1])
    small = dict(search_radius=3, patch_radius=1)
    samples, _, _ = oracle_samples(16)
    M = 4
    A, B = np_buckets(samples[:8], M)
    r = renderer(product_scene, M)
    try:
        r.render(8, 0)
        assert_regress_equal(r.denoise_nlm_image(*nlm_frame("b5"), **sp), nlm_expected("b5", rf)[:2], "1. non-local means, 33 x 9")
        ms = r.debug_nlm_time()
        assert ms[1] > 0.0 and ms[2] > 0.0, ms
        assert_regress_equal(r.denoise_regress_image(*case("a"), **sp), expected("a", rf), "2. regression, 100 x 37")
        assert r.debug_nlm_time() == ms, "a regression call changed surf_debug_nlm_time"
        assert_regress_equal(r.denoise_nlm_image(*nlm_frame("b5"), **sp), nlm_expected("b5", rf)[:2], "3. non-local means again")
        out, err, _ = np_nlm(*np_halves(B), **NLM_SMALL)
        p = dict(threshold=0.12, min_samples=4, max_samples=36, smooth=1, dilate=1)
        want_mask, want_list, _, _ = np_error_mask(out, err, A, **p)
        assert 0 < len(want_list) < W * H
        assert r.mask_from_nlm(nlm=NLM_SMALL, **p) == len(want_list), "4. the mask's count"
        m, n = r.pixel_mask()
        assert np.array_equal(m, want_mask) and n == len(want_list), "4. the mask"
        h0, h1 = np_halves(r.sample_buckets())
        assert_images_equal(h0, np_halves(B)[0], "the context's half 0")
        assert_images_equal(h1, np_halves(B)[1], "the context's half 1")
        assert_regress_equal(r.denoise_regress(**small), np_regress(h0, h1, r.aov(), **small), "5. regression on the context")
    finally:
        r.close()


def test_lifecycle(product_scene):
    dev_err = lambda f, *a, **k: pytest.raises(surf_amd.SurfError, f, *a, **k).value
    r = surf_amd.Renderer(product_scene, W, H)
    try:
        r.render(2, 0)
        e = dev_err(r.denoise_regress)                                              # buckets off
        assert e.code == SURF_ERR_INVALID and "surf_set_sample_buckets" in str(e)
        r.clear_accumulator()
        r.set_sample_buckets(4)
        r.render(6, 0)
        first = r.denoise_regress()
        assert_regress_equal(first, np_regress(*np_halves(r.sample_buckets()), r.aov()), "after clear + enable")
        assert dev_err(r.denoise_regress, search_radius=11).code == SURF_ERR_INVALID
        e = dev_err(r.denoise_regress, ridge=0.0)
        assert e.code == SURF_ERR_INVALID and "ridge" in str(e)
        r.clear_accumulator()
        empty = r.denoise_regress()                                                 # no samples: every pixel invalid, the plain mean of nothing
        assert not empty[0][..., :3].any() and (empty[0][..., 3] == 1).all() and not empty[1].any()
        r.render(6, 0)
        assert_regress_equal(r.denoise_regress(), first, "the same frames after surf_clear_accumulator")
    finally:
        r.close()


def test_row_shards(product_scene):
    """The context form is refused on a row shard; the image form on the halves and planes assembled from two shards
    equals the one-context result."""
    M = 4
    specs = [ShardSpec(k, 2, 2) for k in range(2)]
    rs = [renderer(product_scene, M, shard=s) for s in specs]
    one = renderer(product_scene, M)
    try:
        for r in rs + [one]:
            r.render(FRAMES, 0)
        with pytest.raises(surf_amd.SurfError) as e:
            rs[0].denoise_regress()
        assert e.value.code == SURF_ERR_INVALID and "surf_denoise_regress_image" in str(e.value)
        parts = [r.sample_buckets() for r in rs]
        full = np.stack([surf_amd.assemble_shards(W, H, [p[j] for p in parts], specs) for j in range(M)])
        h0, h1 = surf_amd.bucket_halves(full)
        aovs = [r.aov() for r in rs]
        planes = [surf_amd.assemble_shards(W, H, [a[k] for a in aovs], specs) for k in PLANES]
        assert_regress_equal(rs[1].denoise_regress_image(h0, h1, planes), one.denoise_regress(), "assembled shards against one context")
    finally:
        for r in rs + [one]:
            r.close()


# ---- 4. the example ----------------------------------------------------------------------------------

def test_cpp_example_writes_the_fitted_image(product_scene, tmp_path):
    """render_denoised ... 0 8 3: one frame of 32 samples with 8 buckets, PREFIX_regress.pfm beside the other outputs."""
    import subprocess
    from test_gpu_aov import read_pfm
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    prefix = str(tmp_path / "rg")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "32", prefix, "0", "8", "3"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = renderer(product_scene, 8, True)
    try:
        r.render(1, 0, spp=32)
        want = r.denoise_regress()[0]
        assert_images_equal(want, np_regress(*np_halves(r.sample_buckets()), r.aov())[0], "32 samples in one frame")
    finally:
        r.close()
    words = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert np.array_equal(words(read_pfm(prefix + "_regress.pfm")), words(want[..., :3]))
    for other in ("_noisy.pfm", "_robust.pfm", "_denoised.pfm", "_sampled.pfm", "_nlm.pfm"):
        assert os.path.exists(prefix + other), other
    assert not os.path.exists(prefix + "_nlm_adaptive.pfm")
