"""The mask from the non-local-means filter's error estimate and the adaptive loop on it, on the
device: the mask kernels and the compaction (surf_error_mask_image), the context form
(surf_mask_from_nlm) and the loop (surf_render_adaptive_nlm), against the oracle's per-sample
radiance and the numpy restatements of tests/test_nlm_adaptive_host.py.

Bar: bit-exact, planes compared as uint32 words, masks, lists and counters as integers.
The expected values never come from the code under test.

No rendered frame exceeds 100 x 37; the one large case, 2048 x 600, is three synthetic planes
through the mask kernels alone (4,800 blocks behind the cross-block scan), no render.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import surf_amd
from surf_amd import ShardSpec
from test_denoise_host import assert_images_equal
from test_gpu_aov import read_pfm
from test_nlm_adaptive_host import (LOOP, LOOP_M, NLM_SMALL, check_error_mask, frame_planted, loop_case, mask_cases,
                                    np_error_mask)
from test_nlm_host import np_nlm
from test_robust_host import np_buckets, np_halves
from test_sampled_host import H, W, oracle_samples

pytestmark = pytest.mark.gpu
F = np.float32
SURF_ERR_INVALID = -1


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    surf_amd.load()
    assert surf_amd.device_count() > 0, "no HIP device: -m gpu tests need an MI355X"


def renderer(scene, M, w=W, h=H, **kw):
    r = surf_amd.Renderer(scene, w, h, **kw)
    if M:
        r.set_sample_buckets(M)
    return r


def assert_words_equal(got, want, what):
    assert_images_equal(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32), what)


@pytest.fixture(scope="module")
def ctx(product_scene):
    """A context for the image forms (shared; the tests leave its accumulator alone)."""
    r = surf_amd.Renderer(product_scene, 8, 8)
    assert r.debug_error_mask_time() == [0.0, 0.0]
    yield r
    r.close()


def synthetic(h, w, seed, loud=0.3):
    """Three planes of a made-up w x h frame: colours in 0..1, an err that is tiny except on a `loud` share of the
    pixels, counts in 0..40."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 41, (h, w)).astype(np.float32)
    out = np.ones((h, w, 4), np.float32)
    out[..., :3] = rng.random((h, w, 3), dtype=np.float32)
    err = np.zeros((h, w, 4), np.float32)
    scale = np.where(rng.random((h, w)) < loud, F(0.05), F(1e-5)).astype(np.float32)
    err[..., :3] = rng.random((h, w, 3), dtype=np.float32) * scale[..., None]
    acc = np.concatenate([out[..., :3] * n[..., None], n[..., None]], -1).astype(np.float32)
    return out, err, acc


# ---- 1. the mask kernels ----------------------------------------------------------------------------

def test_mask_image_matches_numpy_and_the_host_twin(ctx):
    cases = mask_cases()
    check_error_mask(ctx.error_mask_image, "device", cases)
    for name, out, err, acc, p in cases:
        (gm, gl), (hm, hl) = ctx.error_mask_image(out, err, acc, **p), surf_amd.error_mask_image_host(out, err, acc, **p)
        assert np.array_equal(gm, hm) and np.array_equal(gl, hl), name


def test_mask_image_tile_edges(ctx):
    """Frames around the 32 x 8 tile with the widest halo, smooth + dilate = 5."""
    s, d = 3, 2
    cases = []
    for w in (31, 32, 33, 65):
        for h in (7, 8, 9, 17):
            out, err, acc = synthetic(h, w, 100 * w + h, loud=0.02)
            cases.append((f"{w}x{h}", out, err, acc, dict(threshold=0.1, min_samples=2, max_samples=36, smooth=s, dilate=d)))
    wants = [np_error_mask(o, e, a, **p) for _, o, e, a, p in cases]
    shares, raws = [m[0].mean() for m in wants], [m[2].mean() for m in wants]
    assert 0.05 < min(shares) and max(shares) < 0.95 and max(raws) < 0.5, (shares, raws)      # sparse raw flags: each one shapes the mask
    check_error_mask(ctx.error_mask_image, "device, tile edges", cases)
    check_error_mask(surf_amd.error_mask_image_host, "host twin, tile edges", cases)


def test_mask_image_large(ctx):
    """2048 x 600 synthetic planes: 1,228,800 pixels, 4,800 compaction blocks, 64 x 75 tiles."""
    h, w = 600, 2048
    out, err, acc = synthetic(h, w, 20, loud=0.02)
    for p in (dict(threshold=0.1, min_samples=8, max_samples=36, smooth=3, dilate=2), dict(threshold=0.1, min_samples=8, max_samples=36, smooth=1, dilate=0),
              dict(threshold=0.1, min_samples=2, max_samples=30, smooth=0, dilate=1)):
        want_mask, want_list, _, _ = np_error_mask(out, err, acc, **p)
        assert 0.05 * h * w < len(want_list) < 0.95 * h * w, (p, len(want_list))
        mask, lst = ctx.error_mask_image(out, err, acc, **p)
        assert np.array_equal(mask, want_mask), (p, int((mask != want_mask).sum()))
        assert len(lst) == len(want_list) and np.array_equal(lst, want_list), p
    ms = ctx.debug_error_mask_time()
    assert len(ms) == 2 and ms[0] > 0 and ms[1] > 0, ms


def test_image_path_needs_no_scene_and_no_buckets():
    lib = surf_amd.load()
    out, err, acc = (np.ascontiguousarray(a) for a in frame_planted())
    h, w = acc.shape[:2]
    hnd = C.c_void_p()
    assert lib.surf_create(0, 8, 8, 0, 8, C.byref(hnd)) == 0
    try:
        kw = dict(threshold=0.05, min_samples=4, max_samples=8, smooth=2, dilate=1)
        p, fp = surf_amd.error_mask_params(**kw), surf_amd.nlm_params()
        mask, n = np.zeros((h, w), np.uint8), C.c_uint32()
        assert lib.surf_mask_from_nlm(hnd, C.byref(fp), C.byref(p), C.byref(n)) == SURF_ERR_INVALID                 # the buckets are off
        args = (out.ctypes.data, err.ctypes.data, acc.ctypes.data)
        assert lib.surf_error_mask_image(hnd, w, h, *args, C.byref(p), mask.ctypes.data, None, C.byref(n)) == 0
        want = np_error_mask(out, err, acc, **kw)
        assert np.array_equal(mask, want[0]) and n.value == len(want[1]) and 0 < n.value < w * h
        assert lib.surf_error_mask_image(hnd, 0, h, *args, C.byref(p), mask.ctypes.data, None, C.byref(n)) == SURF_ERR_INVALID
        bad = surf_amd.error_mask_params(smooth=4)
        assert lib.surf_error_mask_image(hnd, w, h, *args, C.byref(bad), mask.ctypes.data, None, C.byref(n)) == SURF_ERR_INVALID
        got, cnt = np.zeros((8, 8), np.uint8), C.c_uint32()
        assert lib.surf_get_pixel_mask(hnd, got.ctypes.data, C.byref(cnt)) == 0 and got.all() and cnt.value == 64   # the context's mask is left alone
    finally:
        lib.surf_destroy(hnd)


# ---- 2. the context form ----------------------------------------------------------------------------

@pytest.mark.parametrize("M", [2, 4])
def test_mask_from_nlm_on_the_context(product_scene, M):
    samples, _, _ = oracle_samples(16)
    A, B = np_buckets(samples[:8], M)
    out, err, _ = np_nlm(*np_halves(B), **NLM_SMALL)
    r = renderer(product_scene, M)
    try:
        r.render(8, 0)
        p = dict(threshold=0.12, min_samples=4, max_samples=36, smooth=1, dilate=1)
        want_mask, want_list, _, _ = np_error_mask(out, err, A, **p)
        assert 0 < len(want_list) < W * H
        assert r.mask_from_nlm(nlm=NLM_SMALL, **p) == len(want_list)
        m, n = r.pixel_mask()
        assert np.array_equal(m, want_mask) and n == len(want_list)
        assert r.mask_from_nlm(nlm=NLM_SMALL, **{**p, "min_samples": 9}) == W * H                       # below min_samples: every pixel, no mask
        assert r.mask_from_nlm(nlm=NLM_SMALL, **{**p, "max_samples": 8}) == 0                           # at max_samples: none
        assert not r.pixel_mask()[0].any()
        with pytest.raises(surf_amd.SurfError) as e:
            r.mask_from_nlm(nlm=dict(search_radius=11), **p)
        assert e.value.code == SURF_ERR_INVALID and "search_radius" in str(e.value)
        # the device-built list drives a render
        assert r.mask_from_nlm(nlm=NLM_SMALL, **p) == len(want_list)
        r.render(8, 8)
        A2, B2 = np_buckets(samples[8:16], M, A, B, active=want_mask)
        assert_words_equal(r.accumulator(), A2, f"M = {M}: 8 frames under the device-built mask")
        assert_words_equal(r.sample_buckets(), B2, f"M = {M}: buckets, 8 frames under the device-built mask")
    finally:
        r.close()


# ---- 3. the loop ------------------------------------------------------------------------------------

def test_render_adaptive_nlm_matches_the_restatement(product_scene):
    want = loop_case()
    r = renderer(product_scene, LOOP_M)
    try:
        got = r.render_adaptive_nlm(**LOOP)
        assert got["round_active"] == want["round_active"], (got["round_active"], want["round_active"])
        assert (got["rounds"], got["frames"], got["samples"], got["active_last"]) == (want["rounds"], want["frames"], want["samples"], want["active_last"])
        assert got["above"] == want["above"]
        assert F(got["max_error"]).view(np.uint32) == F(want["max_error"]).view(np.uint32), (got["max_error"], want["max_error"])
        assert_words_equal(r.accumulator(), want["acc"], "render_adaptive_nlm: accumulator")
        assert_words_equal(r.sample_buckets(), want["buckets"], "render_adaptive_nlm: buckets")
        m, n = r.pixel_mask()
        assert np.array_equal(m, want["mask"]) and n == want["active_last"]                        # the final mask stays set
        assert_words_equal(got["image"], want["image"], "render_adaptive_nlm: image")
        assert_words_equal(got["err"], want["err"], "render_adaptive_nlm: err")
        assert r.stats()["samples"] == want["samples"]
        with pytest.raises(surf_amd.SurfError) as e:                                                # the accumulator holds samples
            r.render_adaptive_nlm(**LOOP)
        assert e.value.code == SURF_ERR_INVALID and "surf_clear_accumulator" in str(e.value)
        r.clear_accumulator()
        short = r.render_adaptive_nlm(round_cap=2, **LOOP)                                          # round_cap bounds what is written
        assert short["rounds"] == want["rounds"] and short["round_active"] == want["round_active"][:2]
        assert_words_equal(short["image"], want["image"], "render_adaptive_nlm after a clear: image")
    finally:
        r.close()


def test_render_adaptive_nlm_refusals(product_scene):
    plain = surf_amd.Renderer(product_scene, 33, 9)
    try:
        with pytest.raises(surf_amd.SurfError) as e:                                                # buckets off
            plain.render_adaptive_nlm(**LOOP)
        assert e.value.code == SURF_ERR_INVALID and "buckets" in str(e.value)
        with pytest.raises(surf_amd.SurfError) as e:
            plain.mask_from_nlm()
        assert e.value.code == SURF_ERR_INVALID and "buckets" in str(e.value)
    finally:
        plain.close()
    shard = renderer(product_scene, 2, shard=ShardSpec(1, 3, 2))
    try:
        with pytest.raises(surf_amd.SurfError) as e:                                                # a row shard
            shard.render_adaptive_nlm(**LOOP)
        assert e.value.code == SURF_ERR_INVALID and "shard" in str(e.value)
        with pytest.raises(surf_amd.SurfError) as e:
            shard.mask_from_nlm()
        assert e.value.code == SURF_ERR_INVALID and "shard" in str(e.value)
    finally:
        shard.close()


def test_render_adaptive_nlm_stops_when_nothing_is_active(product_scene):
    """A threshold nothing exceeds: the loop ends after min_samples frames with zero rounds."""
    samples, _, _ = oracle_samples(4)
    A, B = np_buckets(samples, 2)
    out, err, _ = np_nlm(*np_halves(B), **NLM_SMALL)
    r = renderer(product_scene, 2)
    try:
        got = r.render_adaptive_nlm(**{**LOOP, "threshold": 1e6})
        assert (got["rounds"], got["frames"], got["active_last"], got["samples"], got["round_active"], got["above"]) == (0, 4, 0, 4 * W * H, [], 0)
        assert_words_equal(r.accumulator(), A, "render_adaptive_nlm that stops at min_samples")
        assert_words_equal(got["image"], out, "render_adaptive_nlm that stops at min_samples: image")
        assert_words_equal(got["err"], err, "render_adaptive_nlm that stops at min_samples: err")
    finally:
        r.close()


# ---- 4. the example ---------------------------------------------------------------------------------

def test_cpp_example_matches_python(product_scene, tmp_path):
    """render_denoised ... 24 2 2: after its other outputs the example clears and runs the loop with the default
    parameters at max_samples 24; PREFIX_nlm_adaptive.pfm is what render_adaptive_nlm returns here.  With NLM = 1
    there is no such file."""
    exe = os.path.join(surf_amd._PKG, "build", "render_denoised")
    word_rows = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    prefix = str(tmp_path / "na")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, str(W), str(H), "2", prefix, "24", "2", "2"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    r = renderer(product_scene, 2)
    try:
        got = r.render_adaptive_nlm(max_samples=24)
    finally:
        r.close()
    assert np.array_equal(word_rows(read_pfm(prefix + "_nlm_adaptive.pfm")), word_rows(got["image"][..., :3]))
    assert f'"nlm_adaptive_frames": {got["frames"]}' in run.stdout and f'"nlm_adaptive_samples": {got["samples"]}' in run.stdout
    assert os.path.exists(prefix + "_nlm.pfm") and os.path.exists(prefix + "_adaptive.pfm")
    plain = str(tmp_path / "plain")
    run = subprocess.run([exe, surf_amd.ASSETS_DIR, "33", "9", "2", plain, "0", "2", "1"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and os.path.exists(plain + "_nlm.pfm") and not os.path.exists(plain + "_nlm_adaptive.pfm")
